"""The contract of include/se3conv_group_norm.h in numpy (a helper module like global_pool_reference.py, not a conftest):
what `se3_group_norm_fwd` and `se3_group_norm_bwd` compute, operation for operation, so that the kernels can be held to it bit
for bit -- and, beside it, the same formula evaluated in fp64 with two passes (`two_pass_fp64`), which the contract itself is
held to.

Sums: chunk `s` holds the points `[s * CHUNK, (s + 1) * CHUNK)`; the partials of (chunk, element, channel) start at +0.0 and
add the element's rows of the chunk as fp64 in ascending row order; the channel totals add the partials in ascending chunk
order; group totals add channel totals in ascending channel order (group of channel c: c % G).  `np.cumsum` along the row axis
IS the serial order (a reduction could pair the terms).  Every fp32 step is one numpy operation on float32 arrays, which
rounds once; every fp64 step likewise."""
import numpy as np

from global_pool_reference import element_rows, present_points, serial_sum, sized_ids, split, trimmed  # noqa: F401  (shared helpers)

CHUNK = 64     # SE3_GROUP_NORM_CHUNK of the header: changed together with it, or every last bit differs
EPS = np.float32(1e-8)    # what blocks.GroupNormPC passes (layers/GroupNormPC.py:41)
f32, f64 = np.float32, np.float64


def channel_totals(u, v, w, ids, n_batches, frames):
    """`(T1 [B, C], T2 [B, C], counts [B])` of the header's "sum of u, v": T1 = sum (double)u, T2 = sum (double)v * (double)w
    over the rows of each element, chunk by chunk.  `ids` holds the present points only."""
    c = u.shape[1]
    t1, t2 = np.zeros((n_batches, c), f64), np.zeros((n_batches, c), f64)
    counts = np.zeros(n_batches, np.int64)
    prod = v.astype(f64) * w.astype(f64)                                 # (exact: two 24-bit significands)
    for b in range(n_batches):
        pts, rows = element_rows(ids, b, frames)
        counts[b] = pts.shape[0]
        chunk = np.repeat(pts // CHUNK, frames)
        for s in np.unique(chunk):                                       # ascending; an empty chunk would add +0.0
            at = rows[chunk == s]
            t1[b] = t1[b] + serial_sum(u[at].astype(f64))
            t2[b] = t2[b] + serial_sum(prod[at])
    return t1, t2, counts


def group_sums(t, groups, weight=None):
    """`[B, G]`: the channel totals `t [B, C]` (times `weight [C]` as fp64, one product each) added per group in ascending c."""
    nb, c = t.shape
    out = np.zeros((nb, groups), f64)
    for ch in range(c):
        term = t[:, ch] if weight is None else weight[ch].astype(f64) * t[:, ch]
        out[:, ch % groups] = out[:, ch % groups] + term
    return out


def _rows(ids, n_rows, n_batches, frames, n_valid):
    """Per feature row: whether it belongs to an element, and that element (0 where it does not)."""
    present = present_points(n_rows, n_valid)
    ids = np.where(np.arange(n_rows) < present, ids, -1)                 # (no absent id is looked at)
    ok = (ids >= 0) & (ids < n_batches)
    return np.repeat(ok, frames), np.repeat(np.where(ok, ids, 0), frames), present


def _xhat(x, mean, invstd, b, groups):
    slot = np.arange(x.shape[1]) % groups
    d = x - mean[b][:, slot]                                            # fp32 subtraction
    return d * invstd[b][:, slot]                                       # fp32 product


def forward(x, gamma, beta, batch_ids, n_batches, groups, eps=EPS, frames=1, n_valid=None):
    """`(y [n_rows * frames, C], save_mean [B, G], save_invstd [B, G])`, all float32."""
    x = np.ascontiguousarray(x, dtype=f32)
    gamma, beta = np.asarray(gamma, f32).reshape(-1), np.asarray(beta, f32).reshape(-1)
    ids = np.asarray(batch_ids)
    n_rows, c = ids.shape[0], x.shape[1]
    assert x.shape[0] == n_rows * frames and c % groups == 0
    live, b, present = _rows(ids, n_rows, n_batches, frames, n_valid)
    xs = np.where(live[:, None], x, f32(0))                              # (absent rows may hold anything: they enter nothing)
    t1, t2, counts = channel_totals(xs, xs, xs, ids[:present], n_batches, frames)
    s1, s2 = group_sums(t1, groups), group_sums(t2, groups)
    n = (counts * frames * (c // groups)).astype(f64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s1 / n
        var = np.maximum(s2 / n - mean * mean, 0.0)
        invstd = 1.0 / np.sqrt(var + f64(f32(eps)))
    has = (counts > 0)[:, None]
    save_mean = np.where(has, mean, 0.0).astype(f32)
    save_invstd = np.where(has, invstd, 0.0).astype(f32)
    xhat = _xhat(xs, save_mean, save_invstd, b, groups)
    y = xhat * gamma[None, :] + beta[None, :]                            # fp32 product, then fp32 addition
    return np.where(live[:, None], y, f32(0)).astype(f32), save_mean, save_invstd


def backward(dy, x, gamma, save_mean, save_invstd, batch_ids, n_batches, groups, frames=1, n_valid=None):
    """`(dx [n_rows * frames, C], dgamma [C], dbeta [C])`, all float32."""
    x, dy = np.ascontiguousarray(x, dtype=f32), np.ascontiguousarray(dy, dtype=f32)
    gamma = np.asarray(gamma, f32).reshape(-1)
    ids = np.asarray(batch_ids)
    n_rows, c = ids.shape[0], x.shape[1]
    live, b, present = _rows(ids, n_rows, n_batches, frames, n_valid)
    xs, gs = np.where(live[:, None], x, f32(0)), np.where(live[:, None], dy, f32(0))
    xhat = _xhat(xs, save_mean, save_invstd, b, groups)
    t1, t2, counts = channel_totals(gs, gs, xhat, ids[:present], n_batches, frames)
    dbeta, dgamma = serial_sum(t1).astype(f32), serial_sum(t2).astype(f32)     # ascending b
    n = (counts * frames * (c // groups)).astype(f64)[:, None]
    has = (counts > 0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(has, group_sums(t1, groups, gamma) / n, 0.0).astype(f32)
        q = np.where(has, group_sums(t2, groups, gamma) / n, 0.0).astype(f32)
    slot = np.arange(c) % groups
    gd = gamma[None, :] * gs
    t = gd - a[b][:, slot]
    xq = xhat * q[b][:, slot]
    u = t - xq
    dx = save_invstd[b][:, slot] * u
    return np.where(live[:, None], dx, f32(0)).astype(f32), dgamma, dbeta


def two_pass_fp64(x, gamma, beta, batch_ids, n_batches, groups, dy, eps=EPS):
    """The reference's formula (layers/GroupNormPC.py:41-57, frames = 1, every id in range) in fp64 with the mean taken
    first and the variance from the centred values, and its analytic gradients: `(y, dx, dgamma, dbeta)` as fp64."""
    x, dy = np.asarray(x, f64), np.asarray(dy, f64)
    gamma, beta = np.asarray(gamma, f64).reshape(-1), np.asarray(beta, f64).reshape(-1)
    ids = np.asarray(batch_ids)
    c = x.shape[1]
    slot = np.arange(c) % groups
    xhat, invstd_rows = np.zeros_like(x), np.zeros_like(x)
    for b in range(n_batches):
        rows = np.flatnonzero(ids == b)
        for j in range(groups):
            v = x[np.ix_(rows, np.flatnonzero(slot == j))]
            if not v.size:
                continue
            d = v - v.mean()
            r = 1.0 / np.sqrt((d * d).mean() + f64(f32(eps)))
            xhat[np.ix_(rows, np.flatnonzero(slot == j))] = d * r
            invstd_rows[np.ix_(rows, np.flatnonzero(slot == j))] = r
    y = xhat * gamma + beta
    dxhat = dy * gamma
    dx = np.zeros_like(x)
    for b in range(n_batches):
        rows = np.flatnonzero(ids == b)
        for j in range(groups):
            at = np.ix_(rows, np.flatnonzero(slot == j))
            if not dxhat[at].size:
                continue
            dx[at] = invstd_rows[at] * (dxhat[at] - dxhat[at].mean() - xhat[at] * (dxhat[at] * xhat[at]).mean())
    return y, dx, (dy * xhat).sum(0), dy.sum(0)


def rel_err(a, b):
    """The project's whole-tensor measure (tests/conftest.py), in fp64."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
