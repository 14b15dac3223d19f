"""include/se3conv_pne.h restated in numpy float64, with a scale per element (shared by tests/test_pne_reference.py,
tests/test_gpu_pne.py and tests/test_gpu_pne_hostile_memory.py; a helper module, CPU only, no test in here).

The entry points: se3_pne_embed_fwd / se3_pne_embed_bwd (all eight kinds) and se3_neigh_max_fwd / se3_neigh_max_bwd
(csrc/pne.hip), as the header words them.  Inputs are the fp32 arrays widened to float64.

Every function returns values and scales.  A scale has the shape of its value and says what an error of that element is
divided by (`worst`): the size of the terms the element is made of, carried through every step by
    scale(f(x1, x2, ...)) = |f| + sum_i |df/dx_i| scale(x_i)
so that an element that is small next to the terms it is the difference of, or that sits on a steep part of its activation,
is held to its own size.  The rules beyond that:
    x_src - y_smp      one rounding of the exact difference of two fp32 inputs: scale |r|
    max(1 - t, 0)      scale 1 + scale(t) where the ramp is on (or within rounding of its foot), 0 behind it: a kernel point
                       farther than sigma adds exactly nothing
    box                a one-hot row is exact; where a second kernel point is within rounding of the nearest (their squared
                       distances closer than 4e-6 of their scales) the edge's scale is +inf -- either choice is legitimate.  An
                       exact tie has no such window: the lowest index, as the header says
    relu'              scale |g| where z is within rounding of 0, else exact
    a sum over edges   fp64 in the kernel, so the terms' own errors are what is left: the random-sign scale
                       sqrt(sum of squared term scales), as tests/rowwise_passes_reference.py takes it, or the magnitude of the
                       sum itself where that is larger
    the fp32 chains    (v of max fwd, dphi, dG) sum of |terms|
`arg` is an INPUT of `max_bwd`, so the backward pass of a kernel is held against the restatement of ITS choice; `hold_max_fwd`
holds the choice itself by value (near-ties may differ, exact ties go to the lowest index).

`T=F` runs the same functions with every step in numpy float32 (the chunk sums of the embedding's backward: float64, rounded
to float32 once, as the header has them; the chains: in-order float32 products and sums, no fma).  BOUNDS is 8 x the largest
error / scale of that emulation against the float64 values over EMBED_CASES and MAX_CASES -- the margin of tests/rowwise_error.py: it covers
the device's erff / expf / sinf, contraction into fma and a maximum over many more elements.  It is computed here, from the
emulation and the float64 values alone; nothing of it is fitted to what the library returns.  `python tests/pne_reference.py`
prints the table.
"""
import functools

import numpy as np
from scipy.special import erf

D, F = np.float64, np.float32
KINDS = {"mlp_linear": 0, "mlp_relu": 1, "mlp_gelu": 2, "mlp_sin": 3, "mlp_softmax": 4, "kp_gauss": 5, "kp_linear": 6, "kp_box": 7}
CHUNK = 1024        # SE3_PNE_CHUNK
MAX_KPTS = 64       # SE3_PNE_MAX_KPTS
SQRT_HALF, INV_SQRT_2PI = 0.70710678118654752440, 0.39894228040143267794
ENTRIES = ("phi", "dA", "dbeta", "out", "dphi", "dG")


def is_kp(kind):
    return kind.startswith("kp_")


def worst(got, want, scale):
    """Largest |got - want| / scale; an element of scale 0 must be met exactly (else inf), one of scale inf is free."""
    err = np.abs(np.asarray(got, D) - np.asarray(want, D))
    scale = np.broadcast_to(np.asarray(scale, D), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isinf(scale), 0.0, ratio)
    return float(ratio.max()) if ratio.size else 0.0


def _chan(total, term_scale, axis=0):
    return np.maximum(np.sqrt((np.asarray(term_scale, D) ** 2).sum(axis)), np.abs(total))


# ------------------------------------------------------------------------------------------------------------ embedding
def embed_inputs(pts, samples, neighbors, rho, kind, kpts=None, sigma=1.0, T=D):
    """`in [E,J']` of the projection and its scale."""
    x, y = np.asarray(pts).astype(T), np.asarray(samples).astype(T)
    nb = np.asarray(neighbors).reshape(-1, 2)
    r = (x[nb[:, 1]] - y[nb[:, 0]]) * T(rho)
    if not is_kp(kind):
        return r, np.abs(r).astype(D)
    kp = np.asarray(kpts).astype(T)
    u = r[:, None, :] - kp[None]
    su = np.abs(r).astype(D)[:, None, :] + np.abs(kp).astype(D)[None]
    d2 = u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1] + u[..., 2] * u[..., 2]
    sd2 = d2.astype(D) + 2.0 * (np.abs(u).astype(D) * su).sum(-1)
    if kind == "kp_box":
        first = np.argmin(d2, axis=1)                                   # the first minimum: the lowest index on a tie
        c = np.zeros(d2.shape, T)
        c[np.arange(d2.shape[0]), first] = 1
        dmin, smin = d2.astype(D).min(1, keepdims=True), np.take_along_axis(sd2, first[:, None], 1)
        near = (d2.astype(D) - dmin <= 4e-6 * (sd2 + smin)) & (d2.astype(D) != dmin)
        sc = np.where(near.any(1, keepdims=True), np.inf, c.astype(D))
        return c, sc
    root = np.sqrt(d2)
    t = root / T(sigma)
    with np.errstate(divide="ignore", invalid="ignore"):
        st = np.where(root > 0, t.astype(D) + sd2 / (2.0 * root.astype(D) * sigma), np.sqrt(sd2) / sigma)
    if kind == "kp_gauss":
        c = np.exp(-(t * t) * T(0.5))
        return c, c.astype(D) * (1.0 + t.astype(D) * st)
    c = np.maximum(T(1) - t, T(0))
    return c, np.where(1.0 - t.astype(D) > -1e-4 * (1.0 + st), 1.0 + st, 0.0)


def _pre_activation(inp, s_in, A, beta, T):
    A, beta = np.asarray(A).astype(T), np.asarray(beta).astype(T).reshape(-1)
    z = np.broadcast_to(beta, (inp.shape[0], beta.shape[0])).copy()
    for j in range(inp.shape[1]):
        z = z + inp[:, j, None] * A[j][None]
    absA = np.abs(A).astype(D)
    with np.errstate(invalid="ignore"):
        prod = np.where(absA[None] > 0, s_in[:, :, None] * absA[None], 0.0)     # (inf * 0 = 0: an absent term)
    return z, np.abs(beta).astype(D)[None] + prod.sum(1)


def _gelu_parts(z):
    cdf = z.dtype.type(0.5) * (z.dtype.type(1) + erf(z * z.dtype.type(SQRT_HALF)))
    pdf = np.exp(-(z * z) * z.dtype.type(0.5)) * z.dtype.type(INV_SQRT_2PI)
    return cdf, pdf


def _activation(kind, z, sz):
    zd = z.astype(D)
    if kind == "mlp_relu":
        return np.maximum(z, 0), np.where(zd > -1e-5 * sz, np.abs(zd) + sz, 0.0)
    if kind == "mlp_gelu":
        cdf, pdf = _gelu_parts(z)
        phi = z * cdf
        return phi, np.abs(phi).astype(D) + np.abs((cdf + z * pdf).astype(D)) * sz
    if kind == "mlp_sin":
        phi = np.sin(z)
        return phi, np.abs(phi).astype(D) + np.abs(np.cos(zd)) * sz
    if kind == "mlp_softmax":
        e = np.exp(z - z.max(1, keepdims=True))
        s = np.zeros((z.shape[0], 1), z.dtype)
        for k in range(z.shape[1]):
            s = s + e[:, k:k + 1]
        phi = e / s
        pd = phi.astype(D)
        return phi, pd * (1.0 + sz + (pd * sz).sum(1, keepdims=True))
    return z, sz.copy()      # linear and the kernel-point kinds


def embed_fwd(pts, samples, neighbors, rho, kind, A, beta, kpts=None, sigma=1.0, T=D):
    """`phi [E,K]`, its scale, and what the backward pass recomputes."""
    inp, s_in = embed_inputs(pts, samples, neighbors, rho, kind, kpts, sigma, T)
    z, sz = _pre_activation(inp, s_in, A, beta, T)
    phi, s_phi = _activation(kind, z, sz)
    return phi, s_phi, {"in": inp, "s_in": s_in, "z": z, "sz": sz}


def _chain(kind, g, z, sz, phi, s_phi, mean_term=True):
    """gz and its scale.  `mean_term=False`: the softmax backward without `q` (a planted fault)."""
    T = g.dtype.type
    gd, zd = np.abs(g).astype(D), z.astype(D)
    if kind == "mlp_relu":
        return np.where(z > 0, g, T(0)), np.where(np.abs(zd) <= 1e-5 * sz, gd, 0.0)
    if kind == "mlp_gelu":
        cdf, pdf = _gelu_parts(z)
        return g * (cdf + z * pdf), gd * (np.abs((cdf + z * pdf).astype(D)) + np.abs((pdf * (T(2) - z * z)).astype(D)) * sz)
    if kind == "mlp_sin":
        return g * np.cos(z), gd * (np.abs(np.cos(zd)) + np.abs(np.sin(zd)) * sz)
    if kind == "mlp_softmax":
        q = np.zeros((z.shape[0], 1), g.dtype)
        for k in range(z.shape[1]):
            q = q + g[:, k:k + 1] * phi[:, k:k + 1]
        if not mean_term:
            q = q * T(0)
        sq = (gd * s_phi).sum(1, keepdims=True)
        return phi * (g - q), s_phi * np.abs((g - q).astype(D)) + phi.astype(D) * (gd + sq)
    return g, np.zeros(g.shape, D)


def embed_bwd(grad_phi, pts, samples, neighbors, rho, kind, A, beta, kpts=None, sigma=1.0, T=D, mean_term=True):
    """`(dA, dbeta), (scale of dA, scale of dbeta)`: chunks of CHUNK edges, fp64 sums whatever T is."""
    g = np.asarray(grad_phi).astype(T)
    phi, s_phi, rec = embed_fwd(pts, samples, neighbors, rho, kind, A, beta, kpts, sigma, T)
    gz, s_gz = _chain(kind, g, rec["z"], rec["sz"], phi, s_phi, mean_term)
    inp, s_in = rec["in"], rec["s_in"]
    j, k = inp.shape[1], gz.shape[1]
    dA, dbeta = np.zeros((j, k), D), np.zeros(k, D)
    for c0 in range(0, inp.shape[0], CHUNK):
        dA += inp[c0:c0 + CHUNK].astype(D).T @ gz[c0:c0 + CHUNK].astype(D)
        dbeta += gz[c0:c0 + CHUNK].astype(D).sum(0)
    agz = np.abs(gz).astype(D)
    with np.errstate(invalid="ignore"):
        term = np.where(agz[:, None, :] > 0, s_in[:, :, None] * agz[:, None, :], 0.0) + np.abs(inp).astype(D)[:, :, None] * s_gz[:, None, :]
    s_dA = _chan(dA, term)
    s_dbeta = _chan(dbeta, s_gz + agz)
    if T is F:
        dA, dbeta = dA.astype(F), dbeta.astype(F)
    return (dA, dbeta), (s_dA, s_dbeta)


# ------------------------------------------------------------------------------------------------------ max aggregation
def _starts(ends):
    ends = np.asarray(ends, np.int64)
    return np.concatenate([[0], ends[:-1]]).astype(np.int64), ends


def edge_values(phi, G, neighbors, T=D):
    """`v [E,C_out]` of every edge and its scale."""
    phi, G = np.asarray(phi).astype(T), np.asarray(G).astype(T)
    src = np.asarray(neighbors).reshape(-1, 2)[:, 1]
    v = np.zeros((phi.shape[0], G.shape[2]), T)
    sv = np.zeros(v.shape, D)
    for k in range(phi.shape[1]):
        v = v + phi[:, k, None] * G[src, k, :]
        sv += np.abs(phi[:, k, None].astype(D) * G[src, k, :].astype(D))
    return v, sv


def max_fwd(phi, G, neighbors, ends, T=D):
    """`out [M,C_out]`, `arg [M,C_out]`, the scale of out (that of the winning edge's value)."""
    v, sv = edge_values(phi, G, neighbors, T)
    starts, ends = _starts(ends)
    m, c = ends.shape[0], v.shape[1]
    out, arg, s_out = np.zeros((m, c), T), np.full((m, c), -1, np.int32), np.zeros((m, c), D)
    for i in range(m):
        if ends[i] > starts[i]:
            a = starts[i] + np.argmax(v[starts[i]:ends[i]], axis=0)      # the first maximum: the lowest edge index
            arg[i], out[i], s_out[i] = a, v[a, np.arange(c)], sv[a, np.arange(c)]
    return out, arg, s_out


def max_bwd(grad_out, arg, phi, G, neighbors, ends, T=D):
    """`(dphi, dG), (their scales)` for the choice `arg`."""
    g, phi, G = np.asarray(grad_out).astype(T), np.asarray(phi).astype(T), np.asarray(G).astype(T)
    nb = np.asarray(neighbors).reshape(-1, 2)
    smp, src = nb[:, 0], nb[:, 1]
    arg = np.asarray(arg)
    e, k = phi.shape
    c = G.shape[2]
    won = (arg[smp] == np.arange(e)[:, None]) if e else np.zeros((0, c), bool)
    w = np.where(won, g[smp], T(0)) if e else np.zeros((0, c), T)
    dphi, s_dphi = np.zeros((e, k), T), np.zeros((e, k), D)
    for o in range(c):
        dphi = dphi + w[:, o, None] * G[src, :, o]
        s_dphi += np.abs(w[:, o, None].astype(D) * G[src, :, o].astype(D))
    dG, s_dG = np.zeros(G.shape, T), np.zeros(G.shape, D)
    for kk in range(k):
        np.add.at(dG[:, kk, :], src, w * phi[:, kk, None])               # unbuffered: ascending edge order
        np.add.at(s_dG[:, kk, :], src, np.abs(w.astype(D) * phi[:, kk, None].astype(D)))
    return (dphi, dG), (s_dphi, s_dG)


def hold_max_fwd(out, arg, phi, G, neighbors, ends, bound):
    """What a kernel's `out` / `arg` must satisfy, by value: raises AssertionError naming the first violation, returns the
    largest error ratio of `out`.
      * a sample without edges: out is +0.0 (bits), arg -1;
      * arg names an edge of the sample, and out is the float64 value of THAT edge within bound x its scale;
      * that value is within bound x (its scale + the scale of the float64 winner) of the float64 maximum;
      * no edge of the sample BEFORE the chosen one has the chosen one's source and bit-identical phi row (an exact tie goes
        to the lowest index)."""
    out, arg = np.asarray(out), np.asarray(arg)
    v, sv = edge_values(phi, G, neighbors)
    _, best, _ = max_fwd(phi, G, neighbors, ends)
    starts, ends = _starts(ends)
    nb = np.asarray(neighbors).reshape(-1, 2)
    phi_bits = np.ascontiguousarray(np.asarray(phi, F)).view(np.int32)
    m, c = out.shape
    cols = np.arange(c)
    ratio = 0.0
    for i in range(m):
        if ends[i] == starts[i]:
            assert not out[i].view(np.int32).any() and (arg[i] == -1).all(), f"sample {i} has no edge: out {out[i][:4]}, arg {arg[i][:4]}"
            continue
        a = arg[i].astype(np.int64)
        assert ((a >= starts[i]) & (a < ends[i])).all(), f"sample {i}: arg outside its edges [{starts[i]}, {ends[i]})"
        r = worst(out[i], v[a, cols], sv[a, cols])
        assert r <= bound, f"sample {i}: out is not the value of its arg ({r:.3g} > {bound:.3g})"
        ratio = max(ratio, r)
        slack = bound * (sv[a, cols] + sv[best[i], cols])
        assert (v[a, cols] >= v[best[i], cols] - slack).all(), f"sample {i}: the chosen edge is not a maximum"
        for e in np.unique(a):
            same = [x for x in range(starts[i], e) if nb[x, 1] == nb[e, 1] and np.array_equal(phi_bits[x], phi_bits[e])]
            assert not same, f"sample {i}: edge {e} chosen, the identical edge {same[0]} comes first"
    return ratio


# ------------------------------------------------------------------------------------------- cases and the error scale
def graph(rng, n_src, degrees):
    """`neighbors [E,2]`, `ends [M]` of samples with the given edge counts, sources drawn at random."""
    smp = np.repeat(np.arange(len(degrees)), degrees)
    src = rng.integers(0, n_src, smp.shape[0])
    return np.stack([smp, src], 1).astype(np.int32), np.cumsum(degrees).astype(np.int32)


def kernel_set(rng, j):
    """`j` kernel points inside the unit ball (the geometry of a test needs no icosahedron)."""
    p = rng.standard_normal((j, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0.2, 0.7, (j, 1))
    p[-1] = 0
    return p.astype(F)


def embed_case(seed, kind, k, j=13, n_src=90, degrees=None):
    """A neighbourhood with samples of 0 and 1 edges and a hub of more than 64 and more than CHUNK edges; the biases and the
    output gradient differ in magnitude per channel."""
    rng = np.random.default_rng(seed)
    degrees = [0, 1, CHUNK + 77, 5, 0, 12, 3] if degrees is None else degrees
    nb, ends = graph(rng, n_src, degrees)
    pts, samples = rng.uniform(-1, 1, (n_src, 3)).astype(F), rng.uniform(-0.3, 0.3, (len(degrees), 3)).astype(F)
    n_in = j if is_kp(kind) else 3
    mag = (10.0 ** rng.permutation(np.linspace(-2, 1, k))).astype(F)
    case = {"kind": kind, "pts": pts, "samples": samples, "neighbors": nb, "ends": ends, "rho": F(0.8),
            "A": rng.uniform(-1, 1, (n_in, k)).astype(F) * np.sqrt(1.0 / n_in).astype(F), "beta": rng.uniform(-0.5, 0.5, k).astype(F),
            "kpts": kernel_set(rng, j) if is_kp(kind) else None, "sigma": {"kp_gauss": 0.3, "kp_linear": 0.4}.get(kind, 1.0),
            "grad_phi": (rng.standard_normal((nb.shape[0], k)) * mag).astype(F)}
    if kind == "kp_box":
        # edge 0 (of sample 1, which has no other) lies exactly between kernel points 2 and 5, nearer than any other (the
        # random ones are at least 0.2 from the origin, the origin itself is 0.03125 away): the lower index wins
        case["rho"] = F(1.0)
        case["samples"][nb[0, 0]], case["pts"][nb[0, 1]] = 0, (0.0, 0.03125, 0.0)
        case["kpts"][2], case["kpts"][5] = (0.015625, 0.03125, 0.0), (-0.015625, 0.03125, 0.0)
        case["tie"] = (0, 2, 5)
    return case


def embed_args(case, T=D):
    return dict(pts=case["pts"], samples=case["samples"], neighbors=case["neighbors"], rho=case["rho"], kind=case["kind"],
                A=case["A"], beta=case["beta"], kpts=case["kpts"], sigma=case["sigma"], T=T)


def max_case(seed, k, c_out, n_src=40, degrees=None):
    """phi, G of uneven magnitude per channel; samples of 0 and 1 edges, a hub of more than 64 edges, a source (0) that wins in
    many samples (its G rows are the largest), and in sample 3 two bit-identical edges (an exact tie)."""
    rng = np.random.default_rng(seed)
    degrees = [0, 1, 150, 6, 9, 0, 4, 7, 5] if degrees is None else degrees
    nb, ends = graph(rng, n_src, degrees)
    e = nb.shape[0]
    mag = (10.0 ** rng.permutation(np.linspace(-2, 1, c_out))).astype(F)
    phi = rng.standard_normal((e, k)).astype(F)
    G = (rng.standard_normal((n_src, k, c_out)) * mag).astype(F)
    starts = np.concatenate([[0], ends[:-1]])
    for i, d in enumerate(degrees):        # the hub source: the first edge of every larger sample, with a dominant positive value
        if d >= 4:
            nb[starts[i], 1] = 0
    G[0] = np.abs(G[0]) * 3
    phi[nb[:, 1] == 0] = np.abs(phi[nb[:, 1] == 0])
    tie = None
    if len(degrees) > 3 and degrees[3] >= 4:
        s3 = int(starts[3])
        nb[s3 + 2], phi[s3 + 2] = nb[s3], phi[s3]                      # the exact tie: edges s3 and s3 + 2, both of source 0
        tie = (3, s3, s3 + 2)
    return {"phi": phi, "G": G, "neighbors": nb, "ends": ends, "tie": tie,
            "grad_out": (rng.standard_normal((len(degrees), c_out)) * mag[::-1]).astype(F)}


EMBED_CASES = [("mlp_linear", 5, 13), ("mlp_relu", 8, 13), ("mlp_gelu", 32, 13), ("mlp_sin", 64, 13), ("mlp_softmax", 5, 13),
               ("mlp_softmax", 32, 13), ("kp_gauss", 8, 13), ("kp_gauss", 32, 55), ("kp_linear", 5, 55), ("kp_linear", 64, 13),
               ("kp_box", 32, 13), ("kp_box", 8, 55)]
MAX_CASES = [(5, 3), (8, 24), (32, 72), (64, 24)]      # (K, C_out)


def emulated_max():
    """Largest error / scale of the float32 emulation against the float64 values, per entry, over the cases above."""
    table = dict.fromkeys(ENTRIES, 0.0)
    for i, (kind, k, j) in enumerate(EMBED_CASES):
        case = embed_case(100 + i, kind, k, j)
        phi, s_phi, _ = embed_fwd(**embed_args(case))
        table["phi"] = max(table["phi"], worst(embed_fwd(**embed_args(case, F))[0], phi, s_phi))
        (dA, db), (s_dA, s_db) = embed_bwd(case["grad_phi"], **embed_args(case))
        (eA, eb), _ = embed_bwd(case["grad_phi"], **embed_args(case, F))
        table["dA"], table["dbeta"] = max(table["dA"], worst(eA, dA, s_dA)), max(table["dbeta"], worst(eb, db, s_db))
    for i, (k, c) in enumerate(MAX_CASES):
        case = max_case(200 + i, k, c)
        v, sv = edge_values(case["phi"], case["G"], case["neighbors"])
        table["out"] = max(table["out"], worst(edge_values(case["phi"], case["G"], case["neighbors"], F)[0], v, sv))
        _, arg, _ = max_fwd(case["phi"], case["G"], case["neighbors"], case["ends"])
        args = (case["grad_out"], arg, case["phi"], case["G"], case["neighbors"], case["ends"])
        (dphi, dG), (s_dphi, s_dG) = max_bwd(*args)
        (ephi, eG), _ = max_bwd(*args, T=F)
        table["dphi"], table["dG"] = max(table["dphi"], worst(ephi, dphi, s_dphi)), max(table["dG"], worst(eG, dG, s_dG))
    return table


@functools.lru_cache(maxsize=None)
def bounds():
    """8 x `emulated_max()`, computed once per process."""
    return {k: 8.0 * v for k, v in emulated_max().items()}


if __name__ == "__main__":
    for name, value in emulated_max().items():
        print(f"{name:6s} emulated {value:.3g}  bound {8 * value:.3g}")
