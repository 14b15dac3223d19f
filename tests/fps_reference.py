"""The contract of include/se3conv_fps.h in numpy fp32 (a helper module like seeded_params.py, not a conftest): what
`se3_fps` must reproduce bit for bit.

Every product and every sum is one `np.float32` operation in the stated order -- `((dx*dx) + (dy*dy)) + (dz*dz)` --, `mind`
starts at +inf, a picked row is marked and never chosen again, and the next pick is the unmarked row with the largest
`mind`, the lowest row on ties (`np.argmax` returns the first maximum)."""
import numpy as np

F = np.float32


def sample_count(n_b: int, ratio) -> int:
    """min(n_b, (int)ceilf((float)n_b * ratio)) with the fp32 product."""
    return min(int(n_b), int(np.ceil(F(n_b) * F(ratio))))


def first_pick(n_b: int, u) -> int:
    """min(max((int)floorf(u * n_b), 0), n_b - 1) with the fp32 product."""
    return min(max(int(np.floor(F(u) * F(n_b))), 0), n_b - 1)


def dist2(pts, p):
    """d(i, p) for every row i: fp32, every operation rounded on its own."""
    d = pts - pts[p]                       # float32 - float32: one rounding per component
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    return (xx + yy) + zz


def fps_element(pts, m: int, first: int):
    """`m` picks of one element: (row ids inside the element, d2_at_pick)."""
    pts = np.ascontiguousarray(pts, dtype=F)
    assert pts.dtype == F and m <= len(pts)
    mind = np.full(len(pts), np.inf, dtype=F)
    marked = np.zeros(len(pts), dtype=bool)
    ids, d2 = np.empty(m, dtype=np.int32), np.empty(m, dtype=F)
    p, at = first, F(np.inf)
    for j in range(m):
        ids[j], d2[j] = p, at
        marked[p] = True
        if j + 1 == m:
            break
        mind = np.fmin(mind, dist2(pts, p))        # fminf: a NaN distance leaves mind as it is
        cand = np.where(marked, F(-1.0), mind)   # marked rows lose against every distance (all are >= 0)
        p = int(np.argmax(cand))                 # first maximum = lowest row
        at = cand[p]
    return ids, d2


def fps_reference(pts, batch_ids, ratio, n_batches: int, start_u=None):
    """(ids [M] int32 rows of `pts` in pick order, element after element; d2_at_pick [M] float32; starts [n_batches + 1]
    int32) for sorted `batch_ids` inside [0, n_batches)."""
    pts = np.ascontiguousarray(pts, dtype=F)
    batch_ids = np.asarray(batch_ids)
    assert np.all(np.diff(batch_ids) >= 0) and (len(batch_ids) == 0 or (batch_ids[0] >= 0 and batch_ids[-1] < n_batches))
    lo = np.searchsorted(batch_ids, np.arange(n_batches + 1), side="left")
    ids, d2, starts = [], [], [0]
    for b in range(n_batches):
        r0, n_b = int(lo[b]), int(lo[b + 1] - lo[b])
        m = sample_count(n_b, ratio)
        if m:
            first = 0 if start_u is None else first_pick(n_b, start_u[b])
            e_ids, e_d2 = fps_element(pts[r0:r0 + n_b], m, first)
            ids.append(e_ids + np.int32(r0))
            d2.append(e_d2)
        starts.append(starts[-1] + m)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dtype=dt)
    return cat(ids, np.int32), cat(d2, F), np.asarray(starts, dtype=np.int32)


def lattice(n: int = 8):
    """The n x n x n integer lattice as float32 rows (ties everywhere: every distance is a small integer)."""
    g = np.arange(n, dtype=F)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def duplicates(rows: int = 64, positions: int = 5, seed: int = 3):
    """`rows` rows that sit on `positions` distinct positions (every position is used)."""
    rng = np.random.default_rng(seed)
    where = rng.standard_normal((positions, 3)).astype(F)
    which = np.concatenate([np.arange(positions), rng.integers(0, positions, rows - positions)])
    return where[rng.permutation(which)]
