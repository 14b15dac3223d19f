"""The row-wise and pooling passes of include/se3conv.h restated in numpy float64, with a scale per element (shared by
tests/test_rowwise_passes_reference.py and tests/test_gpu_rowwise_passes.py; a helper module, CPU only, no test in here).

The passes: se3_bn_fwd / se3_bn_bwd / se3_affine_act / se3_skip_fwd / se3_skip_bwd / se3_bias_gelu_bwd /
se3_channel_sums_padded / se3_linear_wgrad (csrc/glue.hip) and se3_segment_pool / se3_segment_unpool / se3_frame_pool /
se3_frame_unpool (csrc/geometry.hip), as the header words them.  Inputs are the fp32 arrays widened to float64 and every sum is
a float64 `sum`.

Every pass returns {entry: (value, scale)}.  `scale` has the shape of `value`: the sum of the absolute values of the terms
that make the element up -- what an error is divided by (`worst`), so that an element that is small next to its neighbours, or
next to the terms it is the difference of, is held to its own size.  Which terms each scale has is said at the pass.  The
rules they share:
    x - mean              counts as |x| + |mean| where the mean is a RESULT (batch norm: the saved mean is an fp32 value, so
                          the difference carries eps |mean| whatever the kernel does; without the term a plain fp32 evaluation
                          of dx sits at 1.1e-4 for mean/std = 1e3 and 4.7e-2 for 1e4, with it at rounding size)
                          and as |x - center| where the centre is an INPUT (se3_affine_act: the difference of two fp32 inputs
                          is one rounding of the exact result -- the claim of affine_act_kernel's comment; with |x| + |center|
                          the un-centred form x * scale + (shift - center * scale) would pass at any mean/std)
    0.5 (1 + erf)         counts as 0.5 + 0.5 |erf|
    a channel sum         the random-sign scale sqrt(sum of squared term scales), as tests/rowwise_error.py takes it, or the
                          magnitude of the sum itself where that is larger (terms of one sign: the fp32 store alone rounds by
                          eps |sum|)
`scale = None`: an integer result or an exact identity, compared by bits (`arg`, the value a max / min pool selects, the rows
of a sum / max / min unpool, dy = g of the skip, num_batches_tracked).

`emulate_fp32` runs the same functions with every row-wise step in numpy float32 (channel sums: float64, rounded to float32
once; se3_linear_wgrad and the avg / sum pools: in-order float32 sums).  EMULATED_MAX is the largest error / scale of that
emulation against the float64 reference per entry over the cases below, BOUNDS is 8 x that -- the margin of
tests/rowwise_error.py: it covers the device's erff / __expf, contraction into fma, another summation order and a maximum
over up to 1e7 elements.  Reproduce the table with
    python tests/rowwise_passes_reference.py
The bounds come from the emulation and the reference alone; they are not fitted to what the library returns.
"""
import math

import numpy as np
from scipy.special import erf

D, F = np.float64, np.float32
POOL_AVG, POOL_MAX, POOL_MIN, POOL_SUM = 0, 1, 2, 3
MODE_NAMES = {POOL_AVG: "avg", POOL_MAX: "max", POOL_MIN: "min", POOL_SUM: "sum"}
EPS = F(1e-5)
MOMENTUM = F(0.2)

# Largest error / scale of `emulate_fp32` per entry over the cases of this module (python tests/rowwise_passes_reference.py
# prints them), and 8 x that.
EMULATED_MAX = {
    "affine": 1.54e-07, "gelu": 2.48e-07,
    "bn_mean": 5.96e-08, "bn_invstd": 5.87e-08, "bn_y": 2.17e-07, "bn_running_mean": 1.38e-07, "bn_running_var": 1.39e-07,
    "bn_dx": 2.71e-07, "bn_dgamma": 1.39e-07, "bn_dbeta": 5.94e-08,
    "skip_out": 1.57e-07, "skip_dx": 1.07e-07, "skip_dgamma": 1.54e-07,
    "gelu_dz": 2.01e-07, "gelu_dbias": 1.74e-07, "channel_sums": 5.94e-08,
    "wgrad": 9.30e-07,
    "seg_avg": 2.53e-07, "seg_sum": 2.56e-07, "seg_unpool_avg": 5.73e-08,
    "frame_avg": 1.40e-07, "frame_sum": 1.40e-07, "frame_unpool_avg": 3.97e-08,
}
BOUNDS = {k: 8.0 * v for k, v in EMULATED_MAX.items()}


# ------------------------------------------------------------------------------------------------ helpers
def _w(a, T):
    return None if a is None else np.asarray(a).astype(T)


def _chan(sum64, term_scale):
    """Value and scale of a channel sum: sqrt(sum of squared term scales), or |sum| where that is larger."""
    return np.maximum(np.sqrt((np.asarray(term_scale, D) ** 2).sum(0)), np.abs(sum64))


def _vec(v, c, fill, T):
    return np.full(c, fill, T) if v is None else _w(v, T)


def gate_factor(gate, keep):
    """The drop-path factor per batch element, always float32: gate itself (keep == 0), or from the draws u
    floor(float32(keep) + u) * float32(1 / keep) -- what torch's float32 add / floor / div and the kernel compute."""
    gate = np.asarray(gate, F)
    if keep == 0:
        return gate
    return (np.floor(F(keep) + gate) * F(1.0 / keep)).astype(F)


def gate_factor_f64(gate, keep):
    """The planted fault: the same in double precision."""
    return np.floor(D(F(keep)) + np.asarray(gate, F).astype(D)) * (1.0 / D(F(keep)))


def row_factor(gate, keep, row_batch, rows):
    """[rows, 1] float32 factor of every row (1 without a gate)."""
    if gate is None:
        return np.ones((rows, 1), F)
    return gate_factor(gate, keep)[np.asarray(row_batch, np.int64)].reshape(rows, 1)


# ------------------------------------------------------------------------------------------------ batch norm
def bn_fwd(x, weight, bias, running_mean, running_var, eps=EPS, momentum=MOMENTUM, T=D):
    """se3_bn_fwd.  T = float64: the reference.  T = float32: the emulation (statistics in float64 rounded once, the apply
    pass y = (x - mean) * (weight * invstd) + bias in float32).
    Scales: mean  the channel-sum scale of x over N;  invstd  itself (a function of float64 sums, rounded once);
    y  (|x| + |mean|) invstd |weight| + |bias|;  running_*  |(1 - m) old| + |m new|."""
    rows, c = x.shape
    x64 = _w(x, D)
    n = float(max(rows, 1))
    mu = x64.sum(0) / n
    var = ((x64 - mu) ** 2).sum(0) / n                      # biased, centred: a constant channel has exactly 0
    invstd = 1.0 / np.sqrt(var + D(F(eps)))
    unbiased = var * n / (n - 1.0) if rows > 1 else var     # bn_finalize_kernel: one row keeps the biased variance
    m = T(F(momentum))
    mean_t, invstd_t = mu.astype(T), invstd.astype(T)
    w, b = _vec(weight, c, 1.0, T), _vec(bias, c, 0.0, T)
    y = (_w(x, T) - mean_t) * (w * invstd_t) + b
    out = {"bn_mean": (mean_t, _chan(x64.sum(0), np.abs(x64)) / n), "bn_invstd": (invstd_t, invstd),
           "bn_y": (y, (np.abs(x64) + np.abs(mu)) * invstd * np.abs(_w(w, D)) + np.abs(_w(b, D)))}
    if running_mean is not None:
        rm, rv = _w(running_mean, T), _w(running_var, T)
        out["bn_running_mean"] = ((T(1) - m) * rm + m * mean_t, np.abs((1.0 - D(m)) * _w(rm, D)) + np.abs(D(m) * mu))
        out["bn_running_var"] = ((T(1) - m) * rv + m * unbiased.astype(T), np.abs((1.0 - D(m)) * _w(rv, D)) + np.abs(D(m) * unbiased))
    return out


def bn_bwd(dy, x, mean, invstd, gamma, T=D, present=None, mean_term=True):
    """se3_bn_bwd from the saved mean / invstd.  `present`: the N of 1 / N (the planted fault passes the launched rows).
    `mean_term = False`: xhat_s = |x - mean| invstd -- not a scale anything is held to, only the figure that shows what the fp32
    saved mean costs dx at a large mean / std (profiles/rowwise_passes.txt).
    Scales: dbeta  channel sum of |dy|;  dgamma  channel sum of |dy| xhat_s, xhat_s = (|x| + |mean|) invstd;
    dx  |gamma| invstd (|dy| + scale(dbeta) / N + xhat_s scale(dgamma) / N)."""
    rows, c = x.shape
    n = rows if present is None else present
    mean_t, is_t = _w(mean, T), _w(invstd, T)
    ga = _vec(gamma, c, 1.0, T)
    xhat = (_w(x, T) - mean_t) * is_t
    dy64 = _w(dy, D)
    dbeta64, dgamma64 = dy64.sum(0), (dy64 * _w(xhat, D)).sum(0)
    xhat_s = (np.abs(_w(x, D)) + np.abs(_w(mean, D)) if mean_term else np.abs(_w(x, D) - _w(mean, D))) * _w(invstd, D)
    s_dbeta, s_dgamma = _chan(dbeta64, np.abs(dy64)), _chan(dgamma64, np.abs(dy64) * xhat_s)
    dbeta, dgamma = dbeta64.astype(T), dgamma64.astype(T)
    inv_n = T(1) / T(max(n, 1))
    dx = (ga * is_t) * (_w(dy, T) - dbeta * inv_n - xhat * (dgamma * inv_n))
    s_dx = np.abs(_w(ga, D)) * _w(invstd, D) * (np.abs(dy64) + s_dbeta / max(n, 1) + xhat_s * s_dgamma / max(n, 1))
    return {"bn_dx": (dx, s_dx), "bn_dgamma": (dgamma, s_dgamma), "bn_dbeta": (dbeta, s_dbeta)}


# ------------------------------------------------------------------------------------------------ affine + activation
def affine_act(x, center, scale, shift, act, T=D, centred=True):
    """se3_affine_act: act((x - center) * scale + shift), act 0 none / 1 exact-erf GELU; any vector may be None.
    `centred = False`: the planted fault x * scale + (shift - center * scale).
    Scales: t = |x - center| |scale| + |shift| (the centre is an input);  GELU: scale(t) (0.5 + 0.5 |erf|)."""
    rows, c = x.shape
    ce, sc, sh = _vec(center, c, 0.0, T), _vec(scale, c, 1.0, T), _vec(shift, c, 0.0, T)
    t = (_w(x, T) - ce) * sc + sh if centred else _w(x, T) * sc + (sh - ce * sc)
    s_t = np.abs(_w(x, D) - _w(ce, D)) * np.abs(_w(sc, D)) + np.abs(_w(sh, D))
    if act == 0:
        return {"affine": (t, s_t)}
    e = erf(t * T(math.sqrt(0.5)))
    return {"gelu": (T(0.5) * t * (T(1) + e), s_t * (0.5 + 0.5 * np.abs(_w(e, D))))}


def bias_gelu_bwd(g, z, bias, T=D):
    """se3_bias_gelu_bwd: dz = g GELU'(z + bias), GELU'(t) = 0.5 (1 + erf(t / sqrt 2)) + t phi(t); dbias = sum dz.
    Scales: dz  |g| (0.5 + 0.5 |erf| + |t| phi(t));  dbias  channel sum of scale(dz)."""
    rows, c = z.shape
    t = _w(z, T) + _vec(bias, c, 0.0, T)
    e = erf(t * T(math.sqrt(0.5)))
    phi = np.exp(T(-0.5) * t * t) * T(1.0 / math.sqrt(2.0 * math.pi))
    dz = _w(g, T) * (T(0.5) * (T(1) + e) + t * phi)
    s_dz = np.abs(_w(g, D)) * (0.5 + 0.5 * np.abs(_w(e, D)) + np.abs(_w(t, D)) * _w(phi, D))
    dbias64 = _w(dz, D).sum(0)
    return {"gelu_dz": (dz, s_dz), "gelu_dbias": (dbias64.astype(T), _chan(dbias64, s_dz))}


# ------------------------------------------------------------------------------------------------ skip + drop path
def skip_fwd(x, y, gamma, factor=None, T=D):
    """se3_skip_fwd: out = x gamma factor(row) + y; `factor` [rows, 1] float32 (`row_factor`) or None.
    Scale: |x gamma factor| + |y|."""
    f = 1.0 if factor is None else _w(factor, T)
    out = _w(x, T) * _w(gamma, T).reshape(1, -1) * f + _w(y, T)
    f64 = 1.0 if factor is None else _w(factor, D)
    return {"skip_out": (out, np.abs(_w(x, D) * _w(gamma, D).reshape(1, -1) * f64) + np.abs(_w(y, D)))}


def skip_bwd(g, x, gamma, factor=None, T=D):
    """se3_skip_bwd: dx = g gamma factor, dgamma = sum_r g x factor, dy = g (by bits).
    Scales: dx  itself;  dgamma  channel sum of |g x factor|."""
    f = 1.0 if factor is None else _w(factor, T)
    dx = _w(g, T) * _w(gamma, T).reshape(1, -1) * f
    terms = _w(_w(g, T) * _w(x, T) * f, D)
    dgamma64 = terms.sum(0)
    return {"skip_dx": (dx, np.abs(_w(dx, D))), "skip_dgamma": (dgamma64.astype(T), _chan(dgamma64, np.abs(terms))),
            "skip_dy": (np.asarray(g, F), None)}


def channel_sums(x, T=D):
    """se3_channel_sums_padded over the present rows.  Scale: the channel sum of |x|."""
    x64 = _w(x, D)
    s = x64.sum(0)
    return {"channel_sums": (s.astype(T), _chan(s, np.abs(x64)))}


def linear_wgrad(grad_y, x, T=D):
    """se3_linear_wgrad: grad_w[n_out, n_in] = grad_y^T x.  Scale: |grad_y|^T |x|.  T = float32: one accumulator, rows in order."""
    gy64, x64 = _w(grad_y, D), _w(x, D)
    scale = np.abs(gy64).T @ np.abs(x64)
    if T is D:
        return {"wgrad": (gy64.T @ x64, scale)}
    acc = np.zeros((grad_y.shape[1], x.shape[1]), F)
    gy, xf = np.asarray(grad_y, F), np.asarray(x, F)
    for r in range(x.shape[0]):
        acc += gy[r][:, None] * xf[r][None, :]
    return {"wgrad": (acc, scale)}


# ------------------------------------------------------------------------------------------------ pooling
def _first_extremum(block, mode):
    """block [k, c] in pooling order -> (value [c], position [c]): the first extremum wins; a later value replaces only on
    strict > / <, so -0.0 and +0.0 tie and a NaN never replaces (a leading NaN therefore stays)."""
    acc, best = block[0].copy(), np.zeros(block.shape[1], np.int64)
    for j in range(1, block.shape[0]):
        v = block[j]
        with np.errstate(invalid="ignore"):
            better = v > acc if mode == POOL_MAX else v < acc
        acc = np.where(better, v, acc)
        best = np.where(better, j, best)
    return acc, best


def _inorder_sum(block, T):
    return block.astype(D).sum(0) if T is D else np.add.accumulate(block.astype(F), axis=0, dtype=F)[-1]


def _segments(groups, c, mode, T, prefix, src):
    """groups: one id array per output row (pooling order); src [n, c] float32."""
    n_out = len(groups)
    if mode in (POOL_MAX, POOL_MIN):
        out, arg = np.zeros((n_out, c), F), np.full((n_out, c), -1, np.int32)
        for i, ids in enumerate(groups):
            if len(ids):
                v, pos = _first_extremum(np.asarray(src, F)[ids], mode)
                out[i], arg[i] = v, np.asarray(ids)[pos]
        return {f"{prefix}_{MODE_NAMES[mode]}": (out, None), f"{prefix}_{MODE_NAMES[mode]}_arg": (arg, None)}
    out, scale = np.zeros((n_out, c), T), np.zeros((n_out, c), D)
    for i, ids in enumerate(groups):
        if len(ids):
            block = np.asarray(src, F)[ids]
            k = T(len(ids)) if mode == POOL_AVG else T(1)
            out[i] = _inorder_sum(block, T) / k
            scale[i] = np.abs(block.astype(D)).sum(0) / D(k)
    return {f"{prefix}_{MODE_NAMES[mode]}": (out, scale)}


def _cell_groups(sorted_ids, cell_ends):
    ends = np.asarray(cell_ends, np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    return [np.asarray(sorted_ids, np.int64)[s:e] for s, e in zip(starts, ends)]


def segment_pool(src, sorted_ids, cell_ends, mode, T=D):
    """se3_segment_pool over the cells sorted_ids[cell_ends[i - 1] : cell_ends[i]].  avg / sum: scale = sum |v| (/ count);
    max / min: the selected value and `arg` (the ROW id of the first extremum in sorted_ids order) by bits."""
    return _segments(_cell_groups(sorted_ids, cell_ends), src.shape[1], mode, T, "seg", src)


def frame_pool(x, frames, mode, T=D):
    """se3_frame_pool over the rows point * F + frame; `arg` is the winning FRAME (the first one)."""
    n = x.shape[0] // frames
    res = _segments([np.arange(p * frames, (p + 1) * frames) for p in range(n)], x.shape[1], mode, T, "frame", x)
    key = f"frame_{MODE_NAMES[mode]}_arg"
    if key in res:
        res[key] = ((res[key][0] - np.arange(n, dtype=np.int32)[:, None] * frames).astype(np.int32), None)
    return res


def _unpool(vals, owner, count, arg_hit, mode, T, prefix):
    """out[row] = vals[owner[row]] (sum), / count (avg), or where the row is the one `arg` names (max / min, zeros elsewhere:
    +0.0 by bits)."""
    v = np.asarray(vals, F)[owner]
    name = f"{prefix}_unpool_{MODE_NAMES[mode]}"
    if mode == POOL_AVG:
        k = np.asarray(count)[owner].reshape(-1, 1)
        return {name: (v.astype(T) / k.astype(T), np.abs(v.astype(D)) / k.astype(D))}
    if mode in (POOL_MAX, POOL_MIN):
        v = np.where(arg_hit, v, F(0))
    return {name: (v.astype(F), None)}


def segment_unpool(vals, cell_ids, cell_ends, arg, mode, T=D):
    """se3_segment_unpool: rows <- their cell's row.  avg: scale |v| / count; the other modes by bits."""
    cell_ids = np.asarray(cell_ids, np.int64)
    ends = np.asarray(cell_ends, np.int64)
    count = ends - np.concatenate([[0], ends[:-1]])
    hit = None if arg is None else np.asarray(arg)[cell_ids] == np.arange(cell_ids.shape[0])[:, None]
    return _unpool(vals, cell_ids, count, hit, mode, T, "seg")


def frame_unpool(grad_out, arg, frames, mode, T=D):
    """se3_frame_unpool: the F rows of a point <- the point's row."""
    n = grad_out.shape[0]
    owner = np.repeat(np.arange(n), frames)
    hit = None if arg is None else np.asarray(arg)[owner] == np.tile(np.arange(frames), n)[:, None]
    return _unpool(grad_out, owner, np.full(n, frames), hit, mode, T, "frame")


def emulate_fp32(fn, *args, **kw):
    """The same pass with every row-wise step in numpy float32."""
    return fn(*args, T=F, **kw)


# ------------------------------------------------------------------------------------------------ comparison
def worst(got, ref, scale):
    """(largest |got - ref| / scale, its index).  Where the scale is 0 the element must be the reference's exactly; a
    non-finite element where the reference is finite counts as infinitely wrong."""
    got, ref, scale = np.asarray(got, D), np.asarray(ref, D), np.asarray(scale, D)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    if got.size == 0:
        return 0.0, ()
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got) | ~np.isfinite(ref), ratio, np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    return got.shape == ref.shape and got.dtype == ref.dtype and got.tobytes() == ref.tobytes()


def compare(got, ref, what="", bounds=None):
    """`got` {entry: array} against `ref` {entry: (value, scale)}: every entry of `got` within BOUNDS[entry] of its scale, or
    equal by bits where the scale is None.  Returns {entry: ratio}; raises with the entry, the worst element and its ratio."""
    bounds = BOUNDS if bounds is None else bounds
    ratios = {}
    for entry, g in got.items():
        value, scale = ref[entry]
        g = np.asarray(g)
        if scale is None:
            if not same_bits(g, value):
                bad = np.argwhere(np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(value).view(np.uint32)) \
                    if g.shape == value.shape and g.dtype == value.dtype and g.itemsize == 4 else []
                at = tuple(int(i) for i in bad[0]) if len(bad) else ()
                raise AssertionError(f"{what} {entry}: not the reference by bits, first at (row, channel) {at}: "
                                     f"{g[at] if at else g.shape} != {value[at] if at else value.shape} ({len(bad)} elements)")
            ratios[entry] = 0.0
            continue
        r, at = worst(g, value, scale)
        ratios[entry] = r
        if not r <= bounds[entry]:
            raise AssertionError(f"{what} {entry}: error / scale {r:.3e} > {bounds[entry]:.3e} at (row, channel) {at}: "
                                 f"{g[at]!r} against {np.asarray(value)[at]!r}, scale {np.asarray(scale)[at]:.3e}")
    return ratios


def fmt(ratios):
    return " ".join(f"{k}={v:.2e}" for k, v in ratios.items())


# ------------------------------------------------------------------------------------------------ the cases
# (c, vec, rows per sweep of row_walk): scalar with 256 rows; scalar, 1 idle thread; scalar, one row, 126 idle; scalar, one
# row, 1 idle; vector, the workload's width; vector, 4 rows; vector, 3 rows and 61 idle; vector, one row, 1 idle; vector, one
# row, every thread
GLUE_LAYOUTS = [(1, 1, 256), (3, 1, 85), (130, 1, 1), (255, 1, 1), (64, 4, 16), (256, 4, 4), (260, 4, 3), (1020, 4, 1),
                (1024, 4, 1)]
PAST_CAP = (1024, 260, 64, 3)   # one size past the cap of 1024 blocks each: 8192 rpb + rpb + 1 rows
KEEPS = (0.7, 0.5, 0.9)
N_BATCH, EMPTY_BATCH = 5, 3
# the empty element's draw per keep: 0, the largest float32 below 1, the predecessor twice -- never the two the case is about
_DRAW_ROLL = {0.7: 0, 0.5: 4, 0.9: 1}


def glue_cases():
    """(c, rows): every layout at 1, rpb, rpb + 1 and 8 rpb + 1 rows (the first size with two blocks), four of them past the
    cap."""
    out = []
    for c, _, rpb in GLUE_LAYOUTS:
        sizes = sorted({1, rpb, rpb + 1, 8 * rpb + 1})
        if c in PAST_CAP:
            sizes.append(8192 * rpb + rpb + 1)
        out += [(c, r) for r in sizes]
    return out


def gate_draws(keep):
    """Five draws, one per batch element: 1 - float32(keep) (keep + u = 1 exactly: factor 1 / keep); its float32 predecessor
    (the float32 sum is a round-to-even tie; the answer is whatever float32 addition gives); the predecessor twice; 0; the
    largest float32 below 1 -- rolled so that the empty element gets one of the last three."""
    u0 = F(1) - F(keep)
    u1 = np.nextafter(u0, F(0))
    u = np.array([u0, u1, np.nextafter(u1, F(0)), F(0), np.nextafter(F(1), F(0))], F)
    order = [0, 1, 2, 3, 4] if _DRAW_ROLL[keep] == 0 else ([0, 1, 2, 4, 3] if _DRAW_ROLL[keep] == 4 else [0, 1, 3, 2, 4])
    u = u[order]
    assert u[EMPTY_BATCH] not in (u0, u1)
    return u


def _frames_of(rows):
    return 3 if rows % 3 == 0 else (2 if rows % 2 == 0 else 1)


def row_batch_ids(rows):
    """(row_batch [rows] int32, F): per-row batch ids of rows / F points over 5 elements, element 3 empty, F in {1, 2, 3}."""
    f = _frames_of(rows)
    pts = rows // f
    live = [b for b in range(N_BATCH) if b != EMPTY_BATCH]
    cuts = [pts * (i + 1) // len(live) for i in range(len(live))]
    sizes = np.diff([0] + cuts)
    pid = np.repeat(np.array(live, np.int32), sizes)
    return np.repeat(pid, f).astype(np.int32), f


def glue_data(c, rows, seed=0):
    """The fp32 inputs of one glue case.  Rows scaled by 10^U(-3, 3) and channels by 10^U(-2, 2); for batch norm and the
    channel sums the per-row scaling goes on dy only, and the batch-norm x gets a mean / std ratio per channel from
    {0, 1, 1e2, 1e3}, one constant channel (variance exactly 0) and one channel with a single outlier row at 1e4 std."""
    rng = np.random.default_rng(1000 * c + rows % 1000 + seed)
    row_s = 10.0 ** rng.uniform(-3, 3, (rows, 1))
    ch_s = 10.0 ** rng.uniform(-2, 2, (1, c))
    d = {"c": c, "rows": rows}
    d["x"] = (rng.standard_normal((rows, c)) * row_s * ch_s).astype(F)
    d["y"] = (rng.standard_normal((rows, c)) * row_s * ch_s).astype(F)
    d["g"] = (rng.standard_normal((rows, c)) * row_s * 10.0 ** rng.uniform(-2, 2, (1, c))).astype(F)
    d["z"] = (rng.standard_normal((rows, c)) * row_s * ch_s).astype(F)
    ratio = rng.choice([0.0, 1.0, 1e2, 1e3], (1, c))
    bx = (rng.standard_normal((rows, c)) + ratio) * ch_s
    if c >= 3:
        d["constant_channel"], d["outlier_channel"] = c // 2, c - 1
        bx[:, c // 2] = (ratio[0, c // 2] if ratio[0, c // 2] else 1.0) * ch_s[0, c // 2]
        bx[rows // 2, c - 1] = (ratio[0, c - 1] + 1e4) * ch_s[0, c - 1]
    d["bn_x"] = bx.astype(F)
    d["bn_ratio"] = ratio[0]
    for k in ("weight", "bias", "gamma", "running_mean", "gelu_bias"):
        d[k] = rng.standard_normal(c).astype(F)
    d["running_var"] = (rng.random(c) + 0.5).astype(F)
    d["row_batch"], d["frames"] = row_batch_ids(rows)
    return d


# (rows, n_in, n_out, why).  gemm_tn_splits (csrc/gemm.hip) gives min(512 / tiles, ceil(rows / 256)) row ranges of
# ceil(rows / splits) rows rounded up to even, tiles = ceil(n_out / 128) ceil(n_in / 64).
WGRAD_CASES = [
    (1, 32, 5, "one row: one range, an odd row count (the kernel pairs rows)"),
    (255, 13, 130, "one range just under 256 rows; two tiles along n_out, widths no multiple of a tile"),
    (256, 64, 64, "one range of exactly 256 rows"),
    (257, 64, 128, "the smallest row count whose last range is shorter than the others: 2 ranges of 130 and 127 rows"),
    (512, 64, 64, "the smallest row count with one range per 256 rows and more than one of them: 2 x 256"),
    (513, 32, 5, "3 ranges, the odd quotient 171 rounded up to 172: the last has 169 rows"),
    (777, 130, 13, "3 tiles along n_in, 4 ranges of 196, 196, 196 and 189 rows"),
    (4099, 128, 64, "17 ranges of 242 rows, the last of 227; the shape of a block's first linear layer"),
]


def gemm_tn_splits(m, ka, n):
    """csrc/gemm.hip, for operands within one launch's reach (all of WGRAD_CASES)."""
    tiles = ((ka + 127) // 128) * ((n + 63) // 64)
    return max(1, min(max(512 // tiles, 1), (m + 255) // 256))


def wgrad_ranges(rows, n_in, n_out):
    s = gemm_tn_splits(rows, n_out, n_in)
    chunk = (rows + s - 1) // s
    chunk += chunk & 1
    return [max(0, min(chunk, rows - i * chunk)) for i in range(s)]


def wgrad_data(rows, n_in, n_out):
    rng = np.random.default_rng(rows + n_in)
    row_s = 10.0 ** rng.uniform(-3, 3, (rows, 1))
    x = rng.standard_normal((rows, n_in)) * row_s * 10.0 ** rng.uniform(-2, 2, (1, n_in))
    gy = rng.standard_normal((rows, n_out)) * 10.0 ** rng.uniform(-3, 3, (rows, 1)) * 10.0 ** rng.uniform(-2, 2, (1, n_out))
    return gy.astype(F), x.astype(F)


SEG_CHANNELS = (1, 3, 64, 65)
FRAME_CASES = [(f, c) for f in (1, 2, 3, 4) for c in (1, 7, 64)]
FRAME_POINTS = 257
KINDS = ("uneven", "ties")
TIE_VALUES = np.array([-1.0, -0.0, 0.0, 1.0], F)


def segment_level(seed=7):
    """One level built by hand: cells of 1, 2 and 3 rows (40 each, shuffled) and one hub cell of 5 000 rows; the point ids of
    a cell are not contiguous and not ascending (a random permutation of the rows), so "first in sorted_ids order" and "lowest
    row id" are different rows.  -> n, sorted_ids, cell_ends, cell_ids (all int32)."""
    rng = np.random.default_rng(seed)
    sizes = np.array([1, 2, 3] * 40 + [5000])
    rng.shuffle(sizes)
    n = int(sizes.sum())
    sorted_ids = rng.permutation(n).astype(np.int32)
    cell_ends = np.cumsum(sizes).astype(np.int32)
    cell_ids = np.empty(n, np.int32)
    cell_ids[sorted_ids] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return n, sorted_ids, cell_ends, cell_ids


def pool_data(rows, c, kind, seed=0):
    """`uneven`: rows scaled by 10^U(-3, 3), channels by 10^U(-2, 2).  `ties`: drawn from {-1, -0.0, +0.0, 1} with weights
    0.1, 0.4, 0.4, 0.1 (two rows then tie in 2/3 of the channels; with equal weights in 3/8 only)."""
    rng = np.random.default_rng(17 * rows + c + seed)
    if kind == "ties":
        return TIE_VALUES[rng.choice(4, (rows, c), p=[0.1, 0.4, 0.4, 0.1])]
    return (rng.standard_normal((rows, c)) * 10.0 ** rng.uniform(-3, 3, (rows, 1)) * 10.0 ** rng.uniform(-2, 2, (1, c))).astype(F)


def frame_data(frames, c, kind, seed=0):
    """The two kinds, and `equal`: every frame of a point holds the same row (input features replicated over the frames)."""
    if kind == "equal":
        return np.repeat(pool_data(FRAME_POINTS, c, "uneven", seed), frames, axis=0)
    return pool_data(FRAME_POINTS * frames, c, kind, seed)


def tied_fraction(src, groups, mode):
    """Share of the (group, channel) pairs of groups with >= 2 rows whose extremum is reached more than once."""
    tied = total = 0
    for ids in groups:
        if len(ids) >= 2:
            b = np.asarray(src, D)[ids]
            ext = b.max(0) if mode == POOL_MAX else b.min(0)
            tied += int(((b == ext).sum(0) > 1).sum())
            total += b.shape[1]
    return tied / max(total, 1)


# ------------------------------------------------------------------------------------------------ every pass of a case
def glue_reference(d, T=D, only=None):
    """Every glue pass on the data of one case -> {label: {entry: (value, scale)}}; the same calls the GPU test makes."""
    rows = d["rows"]
    res = {}
    fwd = bn_fwd(d["bn_x"], d["weight"], d["bias"], d["running_mean"], d["running_var"], T=T)
    res["bn_fwd"] = fwd
    ref_fwd = fwd if T is D else bn_fwd(d["bn_x"], d["weight"], d["bias"], d["running_mean"], d["running_var"])
    mean32, invstd32 = ref_fwd["bn_mean"][0].astype(F), ref_fwd["bn_invstd"][0].astype(F)   # the saved statistics, as inputs
    res["bn_bwd"] = bn_bwd(d["g"], d["bn_x"], mean32, invstd32, d["weight"], T=T)
    # eval-mode batch norm: center = the mean, scale = weight / sqrt(var + eps), shift = bias
    ev_scale = (d["weight"].astype(D) * invstd32.astype(D)).astype(F)
    res["bn_eval"] = affine_act(d["bn_x"], mean32, ev_scale, d["bias"], 0, T=T)
    res["affine_scale_only"] = affine_act(d["x"], None, d["weight"], None, 0, T=T)
    res["gelu_bias"] = affine_act(d["z"], None, None, d["gelu_bias"], 1, T=T)
    res["gelu_all"] = affine_act(d["z"], d["running_mean"], d["weight"], d["gelu_bias"], 1, T=T)
    res["gelu_none"] = affine_act(d["z"], None, None, None, 1, T=T)
    res["gelu_bwd"] = bias_gelu_bwd(d["g"], d["z"], d["gelu_bias"], T=T)
    res["gelu_bwd_no_bias"] = bias_gelu_bwd(d["g"], d["z"], None, T=T)
    res["channel_sums"] = channel_sums(d["g"], T=T)
    for label, gate, keep in skip_forms(d):
        f = row_factor(gate, keep, d["row_batch"], rows) if gate is not None else None
        res[label] = dict(skip_fwd(d["x"], d["y"], d["gamma"], f, T=T), **skip_bwd(d["g"], d["x"], d["gamma"], f, T=T))
    return res


def skip_forms(d):
    """(label, gate, keep): no gate; the gate as factor (built from the draws of keep 0.7); the draws with each keep."""
    forms = [("skip_plain", None, 0.0), ("skip_factor", gate_factor(gate_draws(0.7), 0.7), 0.0)]
    return forms + [(f"skip_draws_{k}", gate_draws(k), k) for k in KEEPS]


def pool_reference(T=D):
    """Every pooling case -> {label: {entry: (value, scale)}} with its gradient pass (the incoming gradient is `pool_data` of
    the output shape)."""
    res = {}
    n, sorted_ids, cell_ends, cell_ids = segment_level()
    for c in SEG_CHANNELS:
        for kind in KINDS:
            src, gr = pool_data(n, c, kind), pool_data(len(cell_ends), c, "uneven", 1)
            for mode in MODE_NAMES:
                fw = segment_pool(src, sorted_ids, cell_ends, mode, T=T)
                arg = fw.get(f"seg_{MODE_NAMES[mode]}_arg", (None,))[0]
                res[f"seg c={c} {kind} {MODE_NAMES[mode]}"] = dict(fw, **segment_unpool(gr, cell_ids, cell_ends, arg, mode, T=T))
    for f, c in FRAME_CASES:
        for kind in KINDS + ("equal",):
            x, gr = frame_data(f, c, kind), pool_data(FRAME_POINTS, c, "uneven", 1)
            for mode in MODE_NAMES:
                fw = frame_pool(x, f, mode, T=T)
                arg = fw.get(f"frame_{MODE_NAMES[mode]}_arg", (None,))[0]
                res[f"frame F={f} c={c} {kind} {MODE_NAMES[mode]}"] = dict(fw, **frame_unpool(gr, arg, f, mode, T=T))
    return res


def ratios_of(emu, ref, into):
    for label, entries in ref.items():
        for entry, (value, scale) in entries.items():
            got = emu[label][entry][0]
            if scale is None:
                assert same_bits(np.asarray(got), np.asarray(value)), (label, entry)
                continue
            r, _ = worst(got, value, scale)
            into[entry] = max(into.get(entry, 0.0), r)
    return into


def emulated_ratios(cases=None, pools=True, wgrad=True, progress=None):
    """Largest error / scale of the float32 emulation against the float64 reference, per entry."""
    out = {}
    for c, rows in (glue_cases() if cases is None else cases):
        d = glue_data(c, rows)
        ratios_of(glue_reference(d, F), glue_reference(d, D), out)
        if progress:
            progress(f"c={c} rows={rows}")
    if wgrad:
        for rows, n_in, n_out, _ in WGRAD_CASES:
            gy, x = wgrad_data(rows, n_in, n_out)
            ratios_of({"w": linear_wgrad(gy, x, T=F)}, {"w": linear_wgrad(gy, x)}, out)
    if pools:
        ratios_of(pool_reference(F), pool_reference(D), out)
    return out


if __name__ == "__main__":
    import sys
    table = emulated_ratios(progress=lambda s: print("  ..", s, file=sys.stderr))
    print("EMULATED_MAX = {")
    for k in sorted(table):
        print(f'    "{k}": {table[k]:.2e},')
    print("}")
