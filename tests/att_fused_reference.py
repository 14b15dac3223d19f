"""include/se3conv_att_fused.h restated in numpy float64, with a scale per element (shared by tests/test_att_fused_reference.py,
tests/test_gpu_att_fused.py and tests/test_gpu_att_fused_hostile_memory.py; a helper module, CPU only, no test in here).

The entry points: se3_att_fused_fwd / se3_att_fused_bwd (csrc/att_fused.hip), as the header words them: the attention of
MultiHeadAttLayer / LoRAttConvLayer on per-edge scalars, without the aggregate `T [N, 2V, K]`.  Inputs are the fp32 arrays
widened to float64.

Every output comes with a scale of its own shape, under the rules of tests/basis_att_reference.py: the sum of the absolute
values of the terms an element is made of, each term with the scales of its factors,
    scale(f(x1, x2, ...)) = |f| + sum_i |df/dx_i| scale(x_i),
so an element that is small next to the terms it is the difference of is held to the size of those terms, an element with no
term at all (`out` of an edge-less sample, `dxv` / `dxq` of a source without incoming edges) has the scale 0 and must be met
exactly, the softmax carries `att (1 + scale(s) + sum_k att scale(s))`, every stored product carries TINY (the smallest normal
fp32), and `dpe` -- summed in fp64 by the kernel -- the random-sign scale of its terms or the magnitude of the sum where that is
larger.  `att` is an input of the backward call; the restatement feeds it the float64 `att` WITH its scale.

`T_=F` runs the same steps in numpy float32 in the header's order: the chains over the channels of a head, over a sample's
edges (ascending edge order) and over a source's entries (the order of the transposed list) one float32 product and one
float32 addition at a time (no fma), the trees in the header's pairwise order, the chunk sums of `dpe` in float64 over float32
products and rounded once.  `bounds()` is 8 x the largest error / scale of that emulation against the float64 values over CASES:
the project's margin (tests/rowwise_error.py), which covers the device's expf, the fma's and a maximum over more elements.  It
is computed here from the emulation and the float64 values alone; nothing of it is fitted to what the library returns.
`python tests/att_fused_reference.py` prints the table.

`fault=` plants the errors tests/test_att_fused_reference.py must catch.
"""
import functools

import numpy as np

from basis_att_reference import MAX_BASIS, TINY, tree, worst  # noqa: F401  (one tree_k, one `worst` for both headers)

D, F = np.float64, np.float32
CHUNK = 256         # SE3_ATT_FUSED_CHUNK
SLAB = 64           # SE3_ATT_FUSED_SLAB
ENTRIES = ("att", "out", "dphi", "dx", "dpe")
FAULTS = ("scores_without_pe", "value_query_swapped", "dkey_without_pe", "dphi_without_ds_c", "edge_ids_ignored",
          "edgeless_att_zero", "dpe_missing_chunk")


# ------------------------------------------------------------------------------------------------------------- graphs
def transpose(nbr, n):
    """`t_samples [E]`, `t_ends [N]`, `t_edge_ids [E]` as se3_csr_transpose gives them: grouped by source, a group in ascending
    sample order (the edges of one sample that share a source in ascending edge order)."""
    nbr = np.asarray(nbr).reshape(-1, 2)
    order = np.argsort(nbr[:, 1], kind="stable")
    t_ends = np.cumsum(np.bincount(nbr[:, 1], minlength=n)).astype(np.int32)
    return nbr[order, 0].astype(np.int32), t_ends, order.astype(np.int32)


def graph(seed, n, max_degree, hub=0, repeats=True):
    """`neighbors [E,2]` (sample, source) grouped by sample and `ends [N]` (inclusive) of one cloud of `n` points with degrees
    drawn from 0 .. max_degree, and in it, wherever `n` allows: an edge-less sample (sample 1), sources without an incoming
    edge (the last point, and point 1), a self edge (sample 0), a source repeated inside one sample (sample 2), and -- `hub` > 0
    -- one sample (n // 2) of `hub` edges.  `max_degree == 0`: no edge at all.  `repeats=False`: no sample lists a source twice,
    as in a neighbourhood query's list -- se3_csr_transpose orders a source's entries by sample and leaves the order of such
    twins to the run, so two transpositions of a list without them are equal and the sums over them have one order."""
    rng = np.random.default_rng(seed)
    if n == 0 or max_degree == 0:
        return np.zeros((0, 2), np.int32), np.zeros(n, np.int32)
    deg = rng.integers(0, max_degree + 1, n)
    deg[0] = max(deg[0], 1)
    if n > 1:
        deg[1] = 0
    if n > 3:
        deg[2] = max(deg[2], 2)
    if hub and n > 4:
        deg[n // 2] = hub
    allowed = np.array([p for p in range(n) if n < 4 or p not in (1, n - 1)])
    rows = []
    for s in range(n):
        src = rng.choice(allowed, deg[s], replace=repeats)
        if s == 0 and 0 not in src[1:]:
            src[0] = 0
        elif s == 0:
            src = np.concatenate([[0], src[src != 0]])[:deg[s]] if not repeats else np.concatenate([[0], src[1:]])
        if s == 2 and n > 3 and repeats:
            src[1] = src[0]
        rows += [(s, p) for p in src]
    nbr = np.array(rows, np.int32).reshape(-1, 2)
    return nbr, np.cumsum(deg).astype(np.int32)


def _rank(index):
    """Position of every entry inside its group, for a non-decreasing `index`."""
    index = np.asarray(index, np.int64)
    first = np.searchsorted(index, index, side="left")
    return np.arange(index.shape[0]) - first


def chain(index, terms, n):
    """`out[index[j]] += terms[j]` for ascending j, one addition at a time in the dtype of `terms`; `index` non-decreasing."""
    out = np.zeros((n,) + terms.shape[1:], terms.dtype)
    if terms.shape[0] == 0:
        return out
    rank = _rank(index)
    for r in range(int(rank.max()) + 1):
        m = rank == r
        out[index[m]] = out[index[m]] + terms[m]
    return out


def _heads(a, h):
    """[..., V] -> [..., H, D]"""
    return a.reshape(a.shape[:-1] + (h, a.shape[-1] // h))


def _head_chain(p, q):
    """sum over the last axis of p * q ([..., H, D]), ascending, one product and one addition at a time in their dtype."""
    out = np.zeros(p.shape[:-1], p.dtype)
    for j in range(p.shape[-1]):
        out = out + p[..., j] * q[..., j]
    return out


def both(case, T_=D, fault=None):
    """Forward and backward of a case: values and scales of `att [N,K,H]`, `out [N,V]`, `dphi [E,K]`, `dx [N,3V]`, `dpe [K,V]`."""
    dt = T_
    h = case["heads"]
    phi, x, pe, g = (np.asarray(case[k]).astype(dt) for k in ("phi", "x", "pe", "grad_out"))
    nbr, ends = np.asarray(case["neighbors"]).reshape(-1, 2), np.asarray(case["ends"])
    n, v = x.shape[0], x.shape[1] // 3
    (e, k), d = phi.shape, v // h
    assert x.shape[1] == 3 * v and v % h == 0 and pe.shape == (k, v) and ends.shape == (n,) and nbr.shape[0] == e
    smp, src = nbr[:, 0].astype(np.int64), nbr[:, 1].astype(np.int64)
    assert (np.diff(smp) >= 0).all() and np.array_equal(np.cumsum(np.bincount(smp, minlength=n)), ends)
    xv, xq, key = x[:, :v], x[:, v:2 * v], x[:, 2 * v:]
    if fault == "value_query_swapped":
        xv, xq = xq, xv
    A = lambda a: np.abs(a).astype(D)
    # ---- forward
    c = _head_chain(_heads(xq[src], h), _heads(key[smp], h))                              # [E,H]
    s_c = (_heads(A(xq)[src], h) * _heads(A(key)[smp], h)).sum(-1)
    sc = chain(smp, phi[:, :, None] * c[:, None, :], n)                                     # [N,K,H]
    s_sc = chain(smp, A(phi)[:, :, None] * s_c[:, None, :], n)
    pet = _heads(pe, h)                                                                      # [K,H,D]
    t = _head_chain(np.broadcast_to(pet[None], (n, k, h, d)), np.broadcast_to(_heads(key, h)[:, None], (n, k, h, d)))
    s_t = (A(pet)[None] * _heads(A(key), h)[:, None]).sum(-1)
    if fault != "scores_without_pe":
        sc = sc + t
    s_sc = s_sc + s_t
    sk = sc.transpose(0, 2, 1)                                                               # [N,H,K]: the softmax over the last axis
    w = np.exp(sk - sk.max(-1, keepdims=True)) if n else sk
    att = (w / tree(w)[..., None]).transpose(0, 2, 1) if n else sc                          # [N,K,H]
    if fault == "edgeless_att_zero":
        att = att * (np.bincount(smp, minlength=n) > 0)[:, None, None]
    pa = att.astype(D)
    s_att = pa * (1.0 + s_sc + (pa * s_sc).sum(1, keepdims=True)) + TINY
    a = tree((phi[:, :, None] * att[smp]).transpose(0, 2, 1))                                # [E,H]
    s_a = (A(phi)[:, :, None] * (pa + s_att)[smp]).sum(1) + k * TINY
    out = chain(smp, np.repeat(a, d, 1) * xv[src], n)
    s_out = chain(smp, np.repeat(s_a, d, 1) * A(xv)[src] + TINY, n)
    # ---- backward, sample-major (att as the forward pass gave it: in float64 with its scale)
    sa = s_att if dt is D else np.zeros_like(s_att)
    da = _head_chain(_heads(g[smp], h), _heads(xv[src], h))                                  # [E,H]
    s_da = (_heads(A(g)[smp], h) * _heads(A(xv)[src], h)).sum(-1)
    datt = chain(smp, phi[:, :, None] * da[:, None, :], n)                                   # [N,K,H]
    s_datt = chain(smp, A(phi)[:, :, None] * s_da[:, None, :], n)
    q = tree((att * datt).transpose(0, 2, 1))                                                # [N,H]
    ad = A(datt)
    s_q = (sa * ad + pa * s_datt + pa * ad).sum(1)
    diff = datt - q[:, None, :]
    ds = att * diff
    s_ds = A(ds) + sa * A(diff) + pa * (s_datt + s_q[:, None, :])
    dc = tree((phi[:, :, None] * ds[smp]).transpose(0, 2, 1))                                # [E,H]
    s_dc = (A(phi)[:, :, None] * s_ds[smp]).sum(1) + k * TINY
    dphi = np.zeros((e, k), dt)
    for hh in range(h):
        dphi = dphi + att[smp][:, :, hh] * da[:, hh, None]
        if fault != "dphi_without_ds_c":
            dphi = dphi + ds[smp][:, :, hh] * c[:, hh, None]
    s_dphi = ((pa + sa)[smp] * s_da[:, None, :] + s_ds[smp] * s_c[:, None, :]).sum(-1) + TINY
    r = chain(smp, np.repeat(dc, d, 1) * xq[src], n)
    u = tree(np.repeat(ds, d, 2).transpose(0, 2, 1) * pe.T[None])                            # [N,V]
    dkey = r if fault == "dkey_without_pe" else r + u
    s_dkey = chain(smp, np.repeat(s_dc, d, 1) * A(xq)[src], n) + (np.repeat(s_ds, d, 2) * A(pe)[None]).sum(1) + k * TINY
    # ---- dpe: fp32 products, fp64 sums per chunk, the chunks in ascending order
    prod = np.repeat(ds, d, 2) * key[:, None, :]                                             # [N,K,V]
    s_prod = np.repeat(s_ds, d, 2) * A(key)[:, None, :] + TINY
    total = np.zeros((k, v), D)
    starts = list(range(0, n, CHUNK))
    for c0 in (starts[:-1] if fault == "dpe_missing_chunk" else starts):
        total += prod[c0:c0 + CHUNK].astype(D).sum(0)
    s_dpe = np.maximum(np.sqrt((s_prod ** 2).sum(0)), np.abs(total))
    dpe = total.astype(F) if dt is F else total
    # ---- backward, source-major: the order of the transposed list
    ts, te, tid = case.get("transposition") or transpose(nbr, n)
    ts, tid = np.asarray(ts, np.int64), np.asarray(tid, np.int64)
    tsrc = np.repeat(np.arange(n), np.diff(np.concatenate([[0], np.asarray(te, np.int64)])))
    pick = np.arange(e) if fault == "edge_ids_ignored" else tid
    dxv = chain(tsrc, np.repeat(a[pick], d, 1) * g[ts], n)
    dxq = chain(tsrc, np.repeat(dc[pick], d, 1) * key[ts], n)
    s_dxv = chain(tsrc, np.repeat(s_a[tid], d, 1) * A(g)[ts] + TINY, n)
    s_dxq = chain(tsrc, np.repeat(s_dc[tid], d, 1) * A(key)[ts] + TINY, n)
    if fault == "value_query_swapped":
        dxv, dxq, s_dxv, s_dxq = dxq, dxv, s_dxq, s_dxv
    return ({"att": att, "out": out, "dphi": dphi, "dx": np.concatenate([dxv, dxq, dkey], 1), "dpe": dpe},
            {"att": s_att, "out": s_out, "dphi": s_dphi, "dx": np.concatenate([s_dxv, s_dxq, s_dkey], 1), "dpe": s_dpe})


# ------------------------------------------------------------------------------------------- cases and the error scale
def case(seed, n, v, heads, k, max_degree, hub=0, kind="uneven", repeats=True):
    """`phi [E,K]`, `x [N,3V]`, `pe [K,V]`, `grad_out [N,V]` and the graph of `graph(seed, n, max_degree, hub)`.
      uneven   magnitudes that differ per point and per channel (two decades each)
      large    queries and keys scaled so that the scores spread to about +-80: exp(s) overflows without the maximum"""
    rng = np.random.default_rng(seed)
    nbr, ends = graph(seed, n, max_degree, hub, repeats)
    e, d = nbr.shape[0], v // heads
    phi = (rng.standard_normal((e, k)) * 10.0 ** rng.uniform(-1, 0.5, (e, 1))).astype(F)
    x = (rng.standard_normal((n, 3 * v)) * 10.0 ** rng.uniform(-1, 0.5, (n, 1)) * 10.0 ** rng.uniform(-1, 0.5, (1, 3 * v))).astype(F)
    bound = np.sqrt(1.0 / v)
    pe = rng.uniform(-bound, bound, (k, v)).astype(F)
    g = (rng.standard_normal((n, v)) * 10.0 ** rng.uniform(-2, 1, (1, v))).astype(F)
    if kind == "large":
        phi = rng.standard_normal((e, k)).astype(F)
        x = rng.standard_normal((n, 3 * v)).astype(F)
        deg = max(float(np.bincount(nbr[:, 0], minlength=n).mean()), 1.0)
        x[:, v:] *= np.float32(np.sqrt(40.0 / np.sqrt(d * deg)))
    return {"phi": phi, "x": x, "pe": pe, "grad_out": g, "neighbors": nbr, "ends": ends, "heads": heads, "kind": kind}


#        (N, V, H, K, max degree, hub, kind)
CASES = [(1, 8, 2, 8, 1, 0, "uneven"), (70, 64, 64, 16, 5, 0, "uneven"), (CHUNK + 1, 32, 4, 8, 9, 0, "uneven"),
         (40, 72, 8, 64, 12, 700, "uneven"), (300, 16, 1, 32, 8, 0, "large"), (33, 12, 2, 5, 6, 0, "uneven"),
         (37, 12, 2, 8, 6, 0, "uneven"), (130, 64, 4, 32, 10, 0, "uneven")]


def emulated_max():
    """Largest error / scale of the float32 emulation against the float64 values, per entry, over CASES."""
    table = dict.fromkeys(ENTRIES, 0.0)
    for i, args in enumerate(CASES):
        c = case(500 + i, *args)
        want, scale = both(c)
        got, _ = both(c, F)
        for name in ENTRIES:
            table[name] = max(table[name], worst(got[name], want[name], scale[name]))
    return table


@functools.lru_cache(maxsize=None)
def bounds():
    """8 x `emulated_max()`, computed once per process."""
    return {k: 8.0 * v for k, v in emulated_max().items()}


if __name__ == "__main__":
    for name, value in emulated_max().items():
        print(f"{name:5s} emulated {value:.3g}  bound {8 * value:.3g}")
