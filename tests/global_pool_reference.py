"""The contract of include/se3conv_global_pool.h in numpy (a helper module like fps_reference.py, not a conftest): what
`se3_global_pool` and `se3_global_unpool` compute, operation for operation, so that the kernels can be held to it bit for bit.

sum / avg: chunk `s` holds the points `[s * CHUNK, (s + 1) * CHUNK)`; the partial sum of (chunk, element, channel) starts at
+0.0 and adds the element's rows of the chunk as fp64 in ascending row order; the total starts at +0.0 and adds the partial
sums in ascending chunk order.  `np.cumsum` along the row axis IS that serial order (a reduction could pair the terms).
max / min: the first row seeds, a later row replaces when it is strictly greater (smaller) -- `pool_extremum_by_rule` says
that as a loop, `global_pool` as the closed form of it (ties to the lowest row; a NaN never replaces and is never replaced)."""
import numpy as np

CHUNK = 128    # SE3_GLOBAL_POOL_CHUNK of the header: changed together with it, or every last bit differs
AVG, MAX, MIN, SUM = 0, 1, 2, 3
MODES = {"avg": AVG, "max": MAX, "min": MIN, "sum": SUM}


def present_points(n_rows, n_valid):
    return n_rows if n_valid is None else min(max(int(n_valid), 0), n_rows)


def element_rows(ids, b, frames):
    """Ascending: the points of element `b` and the feature rows they own."""
    pts = np.flatnonzero(ids == b)
    rows = (pts[:, None] * frames + np.arange(frames)[None, :]).reshape(-1)
    return pts, rows


def serial_sum(v):
    """+0.0, then the rows of fp64 `v [R, C]` added one after the other."""
    return np.cumsum(np.vstack([np.zeros((1, v.shape[1])), v]), axis=0)[-1]


def pool_extremum_by_rule(v, rows, is_max):
    """The rule itself, row by row: `(best [C], arg [C])` of `v [R, C]` whose rows have the indices `rows`."""
    best, arg = v[0].copy(), np.full(v.shape[1], rows[0], dtype=np.int32)
    for i in range(1, v.shape[0]):
        better = v[i] > best if is_max else v[i] < best
        best, arg = np.where(better, v[i], best), np.where(better, rows[i], arg).astype(np.int32)
    return best, arg


def pool_extremum(v, rows, is_max):
    """The same without the loop: a NaN seed stays; otherwise the first occurrence of the extremum of the non-NaN values."""
    worst = -np.inf if is_max else np.inf
    w = np.where(np.isnan(v), np.float32(worst), v)
    at = np.argmax(w, axis=0) if is_max else np.argmin(w, axis=0)      # (first occurrence)
    at = np.where(np.isnan(v[0]), 0, at)
    return v[at, np.arange(v.shape[1])], rows[at].astype(np.int32)


def global_pool(x, batch_ids, n_batches, mode, frames=1, n_valid=None):
    """`(out [B, C] float32, arg [B, C] int32, counts [B] int32)`; `arg` is all -1 for sum / avg."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ids = np.asarray(batch_ids)
    n_rows, c = ids.shape[0], x.shape[1]
    assert x.shape[0] == n_rows * frames
    present = present_points(n_rows, n_valid)
    ids = ids[:present]                                                 # (no absent id is looked at)
    out = np.zeros((n_batches, c), dtype=np.float32)
    arg = np.full((n_batches, c), -1, dtype=np.int32)
    counts = np.zeros(n_batches, dtype=np.int32)
    for b in range(n_batches):
        pts, rows = element_rows(ids, b, frames)
        counts[b] = pts.shape[0]
        if not pts.shape[0]:
            continue                                                    # +0.0, -1, 0
        if mode in (MAX, MIN):
            out[b], arg[b] = pool_extremum(x[rows], rows, mode == MAX)
            continue
        chunk = np.repeat(pts // CHUNK, frames)
        total = np.zeros(c, dtype=np.float64)
        for s in np.unique(chunk):                                      # ascending; an empty chunk would add +0.0
            total = total + serial_sum(x[rows[chunk == s]].astype(np.float64))
        out[b] = total.astype(np.float32) if mode == SUM else (total / np.float64(int(counts[b]) * frames)).astype(np.float32)
    return out, arg, counts


def global_unpool(vals, batch_ids, arg, counts, mode, frames=1, n_valid=None):
    """`out [n_rows * frames, C]` float32."""
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    ids = np.asarray(batch_ids)
    n_rows, (n_batches, c) = ids.shape[0], vals.shape
    present = present_points(n_rows, n_valid)
    ids = np.where(np.arange(n_rows) < present, ids, -1)                # (no absent id is looked at)
    live = np.repeat((ids >= 0) & (ids < n_batches), frames)            # per row: a present point of an element
    b = np.repeat(np.where((ids >= 0) & (ids < n_batches), ids, 0), frames)
    v = vals[b]
    if mode == AVG:
        v = v / np.where(live, np.asarray(counts)[b] * frames, 1).astype(np.float32)[:, None]
    elif mode in (MAX, MIN):
        v = np.where(np.asarray(arg)[b] == np.arange(n_rows * frames)[:, None], v, np.float32(0))
    return np.where(live[:, None], v, np.float32(0)).astype(np.float32)


def trimmed(x, batch_ids, frames, n_valid):
    """The arrays that hold only the present rows."""
    p = present_points(np.asarray(batch_ids).shape[0], n_valid)
    return np.asarray(x)[:p * frames], np.asarray(batch_ids)[:p]


def sized_ids(sizes, seed=None):
    """int32 ids of `len(sizes)` elements with `sizes[b]` points each, sorted -- or shuffled with `seed`."""
    ids = np.repeat(np.arange(len(sizes), dtype=np.int32), np.asarray(sizes, dtype=np.int64))
    if seed is not None:
        np.random.default_rng(seed).shuffle(ids)
    return ids


def split(points, n_batches, empty=None):
    """`points` points over `n_batches` elements in uneven shares, element `empty` without any."""
    live = [b for b in range(n_batches) if b != empty]
    w = np.array([1 + (7 * b) % 5 for b in live], dtype=np.float64)
    share = np.floor(points * w / w.sum()).astype(np.int64)
    share[0] += points - share.sum()
    sizes = np.zeros(n_batches, dtype=np.int64)
    sizes[live] = share
    return sizes
