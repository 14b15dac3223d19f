"""include/se3conv_basis_att.h restated in numpy float64, with a scale per element (shared by tests/test_basis_att_reference.py,
tests/test_gpu_basis_att.py and tests/test_gpu_basis_att_hostile_memory.py; a helper module, CPU only, no test in here).

The entry points: se3_basis_att_fwd / se3_basis_att_bwd (csrc/basis_att.hip), as the header words them.  Inputs are the fp32
arrays widened to float64.

Every function returns values and scales, under the rules of tests/pne_reference.py.  A scale has the shape of its value and
says what an error of that element is divided by (`worst`): the size of the terms the element is made of, carried through
every step by
    scale(f(x1, x2, ...)) = |f| + sum_i |df/dx_i| scale(x_i)
so that an element that is small next to the terms it is the difference of is held to its own size.  The rules beyond that:
    the fp32 chains    (s, datt, and the trees out, q, dkey) sum of |terms|, each term with the scales of its factors
    softmax            att (1 + scale(s) + sum_k att scale(s)), as pne_reference has it for `mlp_softmax`, plus TINY
    underflow          every stored product carries TINY, the smallest normal fp32, in its scale (a tree over k: K x TINY): with
                       scores 160 apart the float64 att is 1e-70, which no fp32 holds -- it is 0 or a denormal there, and so is
                       what is multiplied by it
    the sum over points (dpe) fp64 in the kernel, so the terms' own errors are what is left: the random-sign scale
                       sqrt(sum of squared term scales), or the magnitude of the sum itself where that is larger
`att` is an input of the backward call; the restatement feeds it the float64 `att` WITH its scale, so the library's own `att`
(within bound x that scale of it) is covered by what the scales carry.

`T=F` runs the same steps in numpy float32 (the chunk sums of dpe: float64 over the float32 dTq, rounded to float32 once, as the
header has them; the chains: in-order float32 products and sums, no fma; the trees: the header's pairwise order).  `bounds()`
is 8 x the largest error / scale of that emulation against the float64 values over CASES -- the margin of
tests/rowwise_error.py: it covers the device's expf, contraction into fma and a maximum over many more elements.  It is computed
here, from the emulation and the float64 values alone; nothing of it is fitted to what the library returns.
`python tests/basis_att_reference.py` prints the table.

`fault=` plants the errors tests/test_basis_att_reference.py must catch.
"""
import functools

import numpy as np

D, F = np.float64, np.float32
CHUNK = 256         # SE3_BASIS_ATT_CHUNK
MAX_BASIS = 64      # SE3_BASIS_ATT_MAX_BASIS
TINY = 2.0 ** -126  # the smallest normal fp32
ENTRIES = ("att", "out", "dT", "dkey", "dpe")
FAULTS = ("softmax_range", "pe_on_value", "dpe_missing_chunk", "dkey_without_pe", "neighbour_key")


def worst(got, want, scale):
    """Largest |got - want| / scale; an element of scale 0 must be met exactly (else inf)."""
    err = np.abs(np.asarray(got, D) - np.asarray(want, D))
    scale = np.broadcast_to(np.asarray(scale, D), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0


def tree(x):
    """`tree_k` of the header over the last axis, in the dtype of `x`."""
    k = x.shape[-1]
    p = 1
    while p < k:
        p *= 2
    if p > k:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (p - k,), x.dtype)], -1)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _split(T, key, pe, heads, dtype):
    T, key, pe = np.asarray(T).astype(dtype), np.asarray(key).astype(dtype), np.asarray(pe).astype(dtype)
    n, v2, k = T.shape
    v = v2 // 2
    pe = pe.reshape(k, v)
    assert v2 == 2 * v and v % heads == 0 and key.shape == (n, v)
    return T[:, :v], T[:, v:], key, pe.T, n, v, k, v // heads


def _per_channel(x_hk, d):
    """[N,H,K] -> [N,V,K]: the row of its head for every channel."""
    return np.repeat(x_hk, d, axis=1)


def fwd(T, key, pe, heads, T_=D, fault=None):
    """`{"att": [N,K,H], "out": [N,V]}`, the scales of both, and what the backward pass takes up."""
    dt = T_
    tv, tq, key, pet, n, v, k, d = _split(T, key, pe, heads, dt)
    if fault == "neighbour_key":
        key = np.roll(key, 1, axis=0)
    a = tq + pet[None]
    s = np.zeros((n, heads, k), dt)
    for j in range(d):
        idx = np.arange(heads) * d + j
        s = s + a[:, idx, :] * key[:, idx, None]
    sz = ((np.abs(tq).astype(D) + np.abs(pet).astype(D)[None]) * np.abs(key).astype(D)[:, :, None]).reshape(n, heads, d, k).sum(2)
    if fault == "softmax_range":      # head 0: the last basis function is left out of the maximum and the denominator
        part = s[:, 0, :max(k - 1, 1)]
        e0 = np.exp(s[:, 0] - part.max(-1, keepdims=True))
        den0 = tree(np.exp(part - part.max(-1, keepdims=True)))
    e = np.exp(s - s.max(-1, keepdims=True))
    den = tree(e)
    if fault == "softmax_range":
        e[:, 0], den[:, 0] = e0, den0
    att = e / den[..., None]
    pa = att.astype(D)
    s_att = pa * (1.0 + sz + (pa * sz).sum(-1, keepdims=True)) + TINY
    val = tv + pet[None] if fault == "pe_on_value" else tv
    out = tree(val * _per_channel(att, d))
    s_out = (np.abs(tv).astype(D) * _per_channel(pa + s_att, d)).sum(-1) + k * TINY
    return ({"att": att.transpose(0, 2, 1), "out": out}, {"att": s_att.transpose(0, 2, 1), "out": s_out})


def bwd(grad_out, T, key, pe, att, s_att, heads, T_=D, fault=None):
    """`{"dT": [N,2V,K], "dkey": [N,V], "dpe": [K,V]}` and their scales, for `att [N,K,H]` with the scale `s_att` (None: exact)."""
    dt = T_
    tv, tq, key, pet, n, v, k, d = _split(T, key, pe, heads, dt)
    if fault == "neighbour_key":
        key = np.roll(key, 1, axis=0)
    g = np.asarray(grad_out).astype(dt)
    w = np.asarray(att).astype(dt).transpose(0, 2, 1)
    pa = w.astype(D)
    sa = np.zeros(pa.shape, D) if s_att is None else np.asarray(s_att, D).transpose(0, 2, 1)
    datt = np.zeros((n, heads, k), dt)
    for j in range(d):
        idx = np.arange(heads) * d + j
        datt = datt + g[:, idx, None] * tv[:, idx, :]
    ag, akey = np.abs(g).astype(D), np.abs(key).astype(D)
    s_datt = (ag[:, :, None] * np.abs(tv).astype(D)).reshape(n, heads, d, k).sum(2)
    q = tree(w * datt)
    ad = np.abs(datt).astype(D)
    s_q = (sa * ad + pa * s_datt + pa * ad).sum(-1)
    diff = datt - q[..., None]
    ds = w * diff
    s_ds = np.abs(ds).astype(D) + sa * np.abs(diff).astype(D) + pa * (s_datt + s_q[..., None])
    w_i, ds_i, s_ds_i = _per_channel(w, d), _per_channel(ds, d), _per_channel(s_ds, d)
    dtv, s_dtv = g[:, :, None] * w_i, ag[:, :, None] * _per_channel(pa + sa, d) + TINY
    dtq, s_dtq = ds_i * key[:, :, None], akey[:, :, None] * s_ds_i + TINY
    dkey = tree(ds_i * (tq if fault == "dkey_without_pe" else tq + pet[None]))
    s_dkey = (s_ds_i * (np.abs(tq).astype(D) + np.abs(pet).astype(D)[None])).sum(-1) + k * TINY
    total = np.zeros((v, k), D)
    starts = list(range(0, n, CHUNK))
    for c0 in (starts[:-1] if fault == "dpe_missing_chunk" else starts):
        total += dtq[c0:c0 + CHUNK].astype(D).sum(0)
    s_dpe = np.maximum(np.sqrt((s_dtq ** 2).sum(0)), np.abs(total))
    dpe = total.T.astype(F) if dt is F else total.T
    return ({"dT": np.concatenate([dtv, dtq], 1), "dkey": dkey, "dpe": dpe},
            {"dT": np.concatenate([s_dtv, s_dtq], 1), "dkey": s_dkey, "dpe": s_dpe.T})


def both(case, T_=D, fault=None):
    """Forward and backward of a case: values and scales of all five entries."""
    val, sc = fwd(case["T"], case["key"], case["pe"], case["heads"], T_, fault)
    s_att = sc["att"] if T_ is D else None
    bv, bs = bwd(case["grad_out"], case["T"], case["key"], case["pe"], val["att"], s_att, case["heads"], T_, fault)
    return {**val, **bv}, {**sc, **bs}


# ------------------------------------------------------------------------------------------- cases and the error scale
def case(seed, n, v, heads, k, kind="uneven"):
    """`T [N,2V,K]`, `key [N,V]`, `pe [K,V]`, `grad_out [N,V]`.
      uneven   magnitudes that differ per point and per channel (two decades each)
      large    keys scaled so that the scores spread to about +-80 (standard deviation 40): exp(s) overflows without the maximum
      zero     as uneven, and point n // 2 has T = 0 and key = 0: its att is exactly 1 / K"""
    rng = np.random.default_rng(seed)
    d = v // heads
    m_pt = 10.0 ** rng.uniform(-1, 1, (n, 1, 1))
    m_ch = 10.0 ** rng.uniform(-1, 1, (1, 2 * v, 1))
    T = (rng.standard_normal((n, 2 * v, k)) * m_pt * m_ch).astype(F)
    key = (rng.standard_normal((n, v)) * 10.0 ** rng.uniform(-1, 0.5, (1, v))).astype(F)
    bound = np.sqrt(1.0 / v)
    pe = rng.uniform(-bound, bound, (k, v)).astype(F)
    g = (rng.standard_normal((n, v)) * 10.0 ** rng.uniform(-2, 1, (1, v))).astype(F)
    if kind == "large":
        T = rng.standard_normal((n, 2 * v, k)).astype(F)
        key = (rng.standard_normal((n, v)) * (40.0 / np.sqrt(d))).astype(F)
    if kind == "zero" and n:
        T[n // 2], key[n // 2] = 0, 0
    return {"T": T, "key": key, "pe": pe, "grad_out": g, "heads": heads, "kind": kind}


#        (N, V, H, K, kind)
CASES = [(1, 6, 3, 5, "uneven"), (CHUNK + 1, 32, 4, 8, "uneven"), (70, 64, 64, 16, "zero"), (40, 72, 8, 64, "uneven"),
         (2 * CHUNK + 37, 16, 1, 32, "uneven"), (33, 12, 2, 12, "zero"), (50, 16, 4, 16, "large"), (20, 8, 2, 8, "large")]


def emulated_max():
    """Largest error / scale of the float32 emulation against the float64 values, per entry, over CASES."""
    table = dict.fromkeys(ENTRIES, 0.0)
    for i, (n, v, h, k, kind) in enumerate(CASES):
        c = case(300 + i, n, v, h, k, kind)
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
