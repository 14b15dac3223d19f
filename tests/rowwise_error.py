"""Row-wise error of the fused operator against the fp64 oracle (shared by tests/test_rowwise_error.py, tests/test_gpu_parity.py,
tests/test_gpu_rowwise_parity.py and tools/fuzz_parity.py; CPU only, no test in here).

`rel_err` of tests/conftest.py is one number per tensor.  A fault confined to a few rows, or to rows that are small next to
the others, is diluted in it.  Here every slice of every result -- an output row, a source row, a c_in slice, a c_out column
and a lane of four c_out of dW, a basis column of dA, an element of dbeta -- is held against ITS OWN scale: the square root of the sum of the squared
terms that make it up (what the sum would be with random signs), obtained by running the operator's contraction on squared
operands.  A rounding of relative size eps in every operand puts an error of about eps x that scale into the slice, whatever
the slice's own value and whatever the other slices hold.

Everything is built from the oracle's own tensors in fp64 (`O.get_rot_tensors`: `rel_pts_rel_orient`, `neighbs`; `O.kernel_mlp`),
so F_in != F_out, two clouds, empty samples and unseen sources follow the oracle's layout.  The work goes in chunks of rows: the
[E', C, K] temporary of `O.conv_forward` never exists (rows are sorted by degree, padded to the chunk's largest, and contracted
with batched matrix products).

The stages, with `q` applied to the operands of every product (alpha = nu / F_in):
    T[m,c,k]   = sum_{e in m} q(x)[src e, c] q(phi)[e, k]            phi = GELU(pre), pre = desc A + beta (fp64, not quantised)
    out        = alpha einsum(q(T), q(W))
    grad_T     = alpha einsum(q(go), q(W))
    dW         = alpha einsum(q(T), q(go))
    dx[src e] += einsum(q(grad_T)[m], q(phi)[e])
    dphi[e,k]  = einsum(q(grad_T)[m], q(x)[src e]);   dpre = dphi GELU'(pre);   dA = q(desc)^T q(dpre), dbeta = sum_e q(dpre)
With a row quantiser `q_rows` (the T16 format) the row-sized intermediates T and U[p,o,k] = sum_{e at p} go[m,o] phi[e,k] go
through it, and dx = alpha einsum(q_rows(U), W) is taken from U as the library does in that mode.

TOLERANCES are 8 x the largest ratio the emulation of each arithmetic mode reaches over ROWWISE_CASES + the hub case (both
data kinds where the mode runs both), on the CPU, against the identity emulation (= the fp64 oracle); for the exact-fp32 mode
the emulation is the fp32 oracle and `emulate_fp32_chain` (in-order fp32 sums), whichever is larger.  Reproduce with
    python tests/rowwise_error.py
which prints the table the constants below were copied from.  They are not fitted to the library.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import se3conv_oracle as O  # noqa: E402

D = torch.float64
KEYS = ("out", "dx", "dA", "dbeta", "dW")
ENTRIES = ("out", "dx", "dW_cin", "dW_cout", "dW_lane", "dA", "dbeta")

# seed n_in n_out F_in F_out C_in C_out k [batches]: the smallest shapes that still reach the code that differs
ROWWISE_CASES = [
    (211, 300, None, 2, 2, 32, 32, 16),        # single-wavefront forms
    (212, 400, None, 2, 2, 128, 128, 20),      # wave-pair kernel, two channel tiles, two parameter-gradient blocks
    (64, 450, 450, 6, 2, 64, 8, 12, 2),        # two clouds with holes of both kinds (the geometry of FORM_CASES' seed 64, which
                                               # has them); F_nb = 6: chunk boundaries inside an edge's frames
    (214, 300, 500, 2, 2, 3, 13, 6),           # odd channel counts on the scalar paths
]
HUB_SEED = 215

# Largest ratio of the emulation of each mode per entry over the cases above (python tests/rowwise_error.py), and 8 x that:
# the library also carries the GELU polynomial, fp32 accumulation and the split descriptor (its whole-tensor error is 2.3 x the
# emulation's in the project's records), and the maximum is over about a thousand slices.  One bound per entry, not the
# largest of them for all: dA and dbeta sum over every frame-edge, where one operand's rounding enters many terms with the
# same sign, and sit 2-3 x above the row entries; a common bound would give that room to the rows too.
# "fp32" is the larger of the fp32 oracle and `emulate_fp32_chain` per entry.  The oracle alone (out 4.4e-7) understates the
# mode: its products are blocked sums, the library's are in-order fp32 sums of C K terms in one accumulator.  Measured on the
# MI355X: output row 69 of FORM_CASES' seed 140 (C_in K = 8192 terms, C_out = 2) at 3.96e-6, and the in-order fp32 sum of
# that row's terms on the CPU gives 3.5e-6 for the same row, the blocked sum 1.2e-7.
EMULATED_MAX = {
    "fp32": {"out": 1.39e-06, "dx": 8.83e-07, "dW_cin": 3.07e-07, "dW_cout": 2.36e-07, "dW_lane": 1.03e-06, "dA": 9.03e-07, "dbeta": 8.26e-07},
    "bf16x3": {"out": 6.92e-06, "dx": 6.66e-06, "dW_cin": 3.26e-06, "dW_cout": 3.74e-06, "dW_lane": 1.04e-05, "dA": 1.17e-05, "dbeta": 1.69e-05},
    "bf16x3_t16": {"out": 1.84e-05, "dx": 1.29e-05, "dW_cin": 2.02e-05, "dW_cout": 1.16e-05, "dW_lane": 7.49e-05, "dA": 9.19e-06, "dbeta": 1.20e-05},
}
TOLERANCES = {m: {k: 8.0 * v for k, v in e.items()} for m, e in EMULATED_MAX.items()}


# ------------------------------------------------------------------------------------------------ quantisers
def split16(t):
    """hi = bf16(t), lo = bf16(t - hi), value hi + lo: the 16 significant bits a split-bf16 operand carries."""
    hi = t.to(torch.bfloat16).to(D)
    return hi + (t - hi).to(torch.bfloat16).to(D)


def t16_rows(t):
    """The T16 block format on rows [R, C, K]: four consecutive channels of one basis function share the exponent
    e of their largest magnitude m = f 2^e, f in [0.5, 1); mantissa rint(x 2^-e 32767), value mant 2^e / 32767; the consumer
    splits that value into hi + lo again.  The library writes the format where the row has a multiple of 64 channels."""
    r, c, k = t.shape
    if c % 64:
        return split16(t)  # rows of the mode that are no multiple of 64 channels stay in the formats of bf16x3
    v = t.reshape(r, c // 4, 4, k)
    _, e = torch.frexp(v.abs().amax(2, keepdim=True))
    e = e.clamp(-64, 127)
    mant = torch.round(torch.ldexp(v, -e) * 32767.0).clamp(-32767.0, 32767.0)
    return split16((torch.ldexp(mant, e) / 32767.0).reshape(r, c, k))


def _identity(t):
    return t


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ row chunks
def _chunks(key, n_rows, width, budget=1 << 23):
    """Rows (values of `key`, one per frame-edge) sorted by degree and cut into chunks; yields (rows [R], idx [R, Dmax] edge ids,
    mask [R, Dmax]) with R * Dmax * width and R * width * 32 elements bounded.  Rows without an edge are left out."""
    order = torch.argsort(key, stable=True)
    deg = torch.bincount(key, minlength=n_rows)
    start = torch.cumsum(deg, 0) - deg
    by_deg = torch.argsort(deg, descending=True, stable=True)
    by_deg = by_deg[deg[by_deg] > 0]
    i = 0
    while i < by_deg.numel():
        dmax = int(deg[by_deg[i]])
        r = max(1, min(budget // (dmax * width), budget // (32 * width)))
        rows = by_deg[i:i + r]
        i += r
        ar = torch.arange(dmax)
        mask = ar[None, :] < deg[rows][:, None]
        idx = order[(start[rows][:, None] + ar[None, :]).clamp_max(order.numel() - 1)]
        yield rows, idx, mask


class Operands:
    """The oracle's frame-level tensors of one case in fp64."""

    def __init__(self, c, neighbors, rho, nu):
        t = lambda v: torch.as_tensor(v).detach().to(D)  # noqa: E731  (rho, nu: the fp32 values the oracle is given)
        self.f_in, self.f_out = c["fi"].shape[1], c["fo"].shape[1]
        self.rows_out, self.rows_in = c["pts_out"].shape[0] * self.f_out, c["pts_in"].shape[0] * self.f_in
        rt = O.get_rot_tensors(t(c["pts_in"]), t(c["pts_out"]), t(c["fi"]), t(c["fo"]), neighbors, t(rho), n_rows=self.rows_out)
        self.desc, self.seg, self.src = rt["rel_pts_rel_orient"], rt["neighbs"][:, 0], rt["neighbs"][:, 1]
        self.a, self.b, self.w, self.x, self.go = (t(c[k]) for k in ("a", "b", "w", "x", "go"))
        self.pre = self.desc @ self.a + self.b
        self.phi = O.kernel_mlp(self.desc, self.a, self.b)
        self.alpha = t(nu) / self.f_in


def fp32(t):
    return t.to(torch.float32).to(D)


def _chain_mm(a, b):
    """a @ b with ONE fp32 accumulator per output element, the terms added in order (what a k loop of MFMAs into one
    accumulator tile does): a [R, n] @ b [n, m], or batched a [B, R, n] @ b [B, n, m]."""
    a, b = a.to(torch.float32), b.to(torch.float32)
    acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
    for i in range(a.shape[-1]):
        acc = acc + a[..., i:i + 1] * b[..., i:i + 1, :]
    return acc.to(D)


def _staged(op, x, p, w, go, alpha, desc, dg, q=_identity, q_rows=None, chain=False):
    """The stages of the module docstring on the given operands (the values, or their squares).  chain: the products whose
    output element the library keeps in one accumulator (T and U over a row's edges, out, grad_T and dx over the row's
    values) are summed in fp32 in order; the reductions it splits and re-reduces (dW, dA, dbeta) stay as they are."""
    mm = _chain_mm if chain else torch.matmul
    c_in, kb, c_out = w.shape
    xq, pq, wq, goq = q(x), q(p), q(w), q(go)
    w2 = wq.reshape(c_in * kb, c_out)
    qt = q_rows or q
    out, dx = x.new_zeros(op.rows_out, c_out), x.new_zeros(op.rows_in, c_in)
    dw, dphi = x.new_zeros(c_in * kb, c_out), x.new_zeros(p.shape)
    for rows, idx, mask in _chunks(op.seg, op.rows_out, max(c_in, c_out, kb)):
        m = mask[:, :, None].to(D)
        xp, pp = xq[op.src[idx]] * m, pq[idx] * m                                  # [R, Dmax, C], [R, Dmax, K]
        t = qt(mm(xp.transpose(1, 2), pp)).reshape(rows.numel(), -1)                  # [R, C K]
        out[rows] = alpha * mm(t, w2)
        dw += alpha * (t.t() @ goq[rows])
        gt = q(alpha * mm(goq[rows], w2.t())).reshape(rows.numel(), c_in, kb)
        dphi[idx[mask]] = torch.bmm(xp, gt)[mask]
        if q_rows is None:
            dx.index_add_(0, op.src[idx[mask]], torch.bmm(pp, gt.transpose(1, 2))[mask])
    if q_rows is not None:  # the feature gradient from U, source-major
        wt = wq.permute(2, 1, 0).reshape(c_out * kb, c_in)
        for rows, idx, mask in _chunks(op.src, op.rows_in, max(c_in, c_out, kb)):
            m = mask[:, :, None].to(D)
            u = q_rows(mm((goq[op.seg[idx]] * m).transpose(1, 2), pq[idx] * m))          # [R, C_out, K]
            dx[rows] = alpha * mm(u.reshape(rows.numel(), -1), wt)
    dpre = q(dphi * dg)
    return {"out": out, "dx": dx, "dA": q(desc).t() @ dpre, "dbeta": dpre.sum(0), "dW": dw.reshape(c_in, kb, c_out)}


def emulate(op, q=_identity, q_rows=None, chain=False):
    """The staged fp64 restatement with quantiser q on every product operand; q = identity is the fp64 oracle."""
    return _staged(op, op.x, op.phi, op.w, op.go, op.alpha, op.desc, gelu_grad(op.pre), q, q_rows, chain)


def emulate_fp32_chain(op):
    """fp32 operands, fp32 accumulation in order, the feature gradient from U: the exact-fp32 mode's row products.  The fp32
    oracle's own products go through blocked, vectorised sums and understate what an in-order fp32 sum of thousands of terms
    loses (u sqrt(n) / 2.4 of the random-sign scale: 2e-6 at n = C_in K = 8192)."""
    return emulate(op, fp32, fp32, chain=True)


def emulate_split16(c, neighbors, rho, nu, q=split16, q_rows=None):
    return emulate(Operands(c, neighbors, rho, nu), q, q_rows)


def _scales(op):
    """P2 = phi^2 + pre^2: the pre-activation's own rounding goes through GELU with GELU' <= 1.13."""
    sq = lambda t: t * t  # noqa: E731
    return _staged(op, sq(op.x), sq(op.phi) + sq(op.pre), sq(op.w), sq(op.go), sq(op.alpha), sq(op.desc), sq(gelu_grad(op.pre)))


def scales(c, neighbors, rho, nu):
    """The squared random-sign scale of every element of out / dx / dA / dbeta / dW."""
    return _scales(Operands(c, neighbors, rho, nu))


def reference_and_scales(c, neighbors, rho, nu):
    """(fp64 reference, squared scales) of a case from one set of oracle tensors: what the GPU tests cache per case."""
    op = Operands(c, neighbors, rho, nu)
    return emulate(op), _scales(op)


# ------------------------------------------------------------------------------------------------ the metric
def _as_dict(v):
    return v if isinstance(v, dict) else dict(zip(KEYS, v))


def ratios(got, ref, s2):
    """{entry: max over slices of ||got - ref||_2(slice) / sqrt(sum s2(slice))} for the entries of ENTRIES (out per output row,
    dx per source row, dW per c_in slice, per c_out column and per lane of four consecutive c_out, dA per basis column, dbeta
    per element), "argmax": {entry: flat slice index}, "zeros_exact": every slice whose scale is 0 (an output row without a neighbour, a source without an edge) is
    exactly zero in got.  got / ref: dicts (or tuples in the order of KEYS), a missing or None tensor is left out."""
    got, ref = _as_dict(got), _as_dict(ref)
    slices = {"out": ("out", (1,)), "dx": ("dx", (1,)), "dW_cin": ("dW", (1, 2)), "dW_cout": ("dW", (0, 1)), "dW_lane": ("dW", (3,)),
              "dA": ("dA", (0,)), "dbeta": ("dbeta", ())}
    res, arg, zeros_exact = {}, {}, True
    for entry, (key, dims) in slices.items():
        if got.get(key) is None:
            continue
        g, r = got[key].detach().to("cpu", D), ref[key].detach().to("cpu", D)
        assert g.shape == r.shape == s2[key].shape, (key, g.shape, r.shape, s2[key].shape)
        d2, g2, s = (g - r) ** 2, g * g, s2[key]
        if entry == "dW_lane":  # four consecutive c_out of one (c_in, basis function): the finest slice
            d2, g2, s = (torch.nn.functional.pad(t, (0, (-t.shape[2]) % 4)).reshape(t.shape[0], t.shape[1], -1, 4) for t in (d2, g2, s))
        if dims:
            d2, g2, s = d2.sum(dims), g2.sum(dims), s.sum(dims)
        live = s > 0
        zeros_exact = zeros_exact and bool((g2[~live] == 0).all())
        rat = torch.where(live, torch.sqrt(d2 / torch.where(live, s, torch.ones_like(s))), torch.zeros_like(s))
        res[entry], arg[entry] = float(rat.max()), int(rat.argmax())
    res["argmax"], res["zeros_exact"] = arg, zeros_exact
    return res


def fmt(r):
    return " ".join(f"{k}={r[k]:.2e}@{r['argmax'][k]}" for k in ENTRIES if k in r) + ("" if r["zeros_exact"] else " NONZERO-EMPTY-SLICE")


# ------------------------------------------------------------------------------------------------ cases
def scaled_case(seed, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches=1, per_channel=True, scaled=True):
    """random_case of tests/test_gpu_parity.py with heterogeneous magnitudes: x and grad_out scaled per point by 10^U(-3,3)
    (the same factor for every frame of a point), x also per channel by 10^U(-2,2) where per_channel."""
    from test_gpu_parity import random_case
    c = random_case(seed, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches)
    return scale_case(c, seed, per_channel) if scaled else c


def scale_case(c, seed, per_channel=True):
    g = torch.Generator().manual_seed(seed + 100003)
    f_in, f_out = c["fi"].shape[1], c["fo"].shape[1]
    sx = 10.0 ** (torch.rand(c["pts_in"].shape[0], generator=g) * 6 - 3)
    sg = 10.0 ** (torch.rand(c["pts_out"].shape[0], generator=g) * 6 - 3)
    sc = 10.0 ** (torch.rand(c["x"].shape[1], generator=g) * 4 - 2)
    c = dict(c)
    c["x"] = c["x"] * sx.repeat_interleave(f_in)[:, None] * (sc[None, :] if per_channel else 1.0)
    c["go"] = c["go"] * sg.repeat_interleave(f_out)[:, None]
    return c


def hub_case(seed=HUB_SEED, per_channel=True, scaled=True, n=300, hub=220, f=2, c_in=32, c_out=32, k_deg=8):
    """300 points at degree 8 plus one sample with at least 200 neighbours: a query point at the cloud's centre and, in the
    input cloud, a cluster of `hub` points inside its ball -- one row of many 32-edge chunks among rows of one partial chunk.
    Two clouds (the samples are the first n input points + the centre), one batch element, ids sorted: the ball query's contract."""
    from test_gpu_parity import random_case
    c = random_case(seed, n, None, f, f, c_in, c_out, k_deg)
    g = torch.Generator().manual_seed(seed + 7)
    centre = torch.full((1, 3), 0.5)
    d = torch.nn.functional.normalize(torch.randn(hub, 3, generator=g), dim=1) * (0.9 * c["r"] * torch.rand(hub, 1, generator=g) ** (1 / 3))
    c["pts_in"] = torch.cat((c["pts_in"], centre + d))
    c["pts_out"] = torch.cat((c["pts_in"][:n], centre))
    c["bid_in"], c["bid_out"] = torch.zeros(n + hub, dtype=torch.int32), torch.zeros(n + 1, dtype=torch.int32)
    c["fi"], c["fo"] = O.random_frames(n + hub, f, g), O.random_frames(n + 1, f, g)
    c["x"], c["go"] = torch.randn((n + hub) * f, c_in, generator=g), torch.randn((n + 1) * f, c_out, generator=g)
    return scale_case(c, seed, per_channel) if scaled else c


def rowwise_cases():
    """(name, builder(per_channel, scaled)) of the cases of tests/test_gpu_rowwise_parity.py."""
    named = [(f"seed{case[0]}", (lambda pc=True, sc=True, case=case: scaled_case(*case, per_channel=pc, scaled=sc)))
             for case in ROWWISE_CASES]
    return named + [("hub", lambda pc=True, sc=True: hub_case(per_channel=pc, scaled=sc))]


def graph_of(c):
    """The oracle's edges and the (fp32) normalisers the parity tests give the operator."""
    nb, ends = O.ball_query(c["pts_in"], c["pts_out"], c["bid_in"], c["bid_out"], c["r"])
    return nb, ends, torch.tensor(1.0 / c["r"]), torch.tensor(ends.shape[0] / max(nb.shape[0], 1))


MODE_QUANTISERS = {"bf16x3": (split16, None), "bf16x3_t16": (split16, t16_rows)}


def emulated_table(out=print):
    """{mode: {entry: largest ratio}} of every mode's emulation over the cases and data kinds: the source of EMULATED_MAX."""
    worst = {m: {} for m in ("fp32", "bf16x3", "bf16x3_t16")}
    for name, make in rowwise_cases():
        for per_channel in (True, False):
            c = make(per_channel)
            nb, _, rho, nu = graph_of(c)
            op = Operands(c, nb, rho, nu)
            ref, s2 = emulate(op), _scales(op)
            runs = {"fp32": O.conv_forward_backward(c["pts_in"], c["pts_out"], c["fi"], c["fo"], nb, c["x"], c["a"], c["b"], c["w"],
                                                    rho, nu, c["go"])}
            runs["fp32 chain"] = emulate_fp32_chain(op)
            for mode, (q, q_rows) in MODE_QUANTISERS.items():
                if mode == "bf16x3_t16" and per_channel:
                    continue  # one exponent per four channels: per-channel scaling loses small channels by design
                runs[mode] = emulate(op, q, q_rows)
            for mode, got in runs.items():
                r = ratios(got, ref, s2)
                for k in ENTRIES:
                    worst[mode.split()[0]][k] = max(worst[mode.split()[0]].get(k, 0.0), r[k])
                out(f"{name:8s} {'point+channel' if per_channel else 'point':13s} {mode:10s} {fmt(r)}")
    for mode, e in worst.items():
        out(f'    "{mode}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in e.items()) + "},")
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    emulated_table()
