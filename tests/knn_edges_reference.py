"""numpy restatement of the two contracts of include/se3conv_knn_edges.h (a helper module like padded_cases.py, not a
conftest): the brute-force k-NN between two clouds, per batch element, ordered by (fp32 squared distance, source index),
and the edge list / ends / info of an id table with truncation.

Test clouds live on a lattice, coordinates i/4 with i in 0 ... 15: every difference is a multiple of 1/4 below 4, every
square a multiple of 1/16 below 16 and every sum of three a multiple of 1/16 below 48 -- all exact in fp32 whatever the
order of the additions and whether a multiply-add is fused.  The (distance, index) order, with plenty of ties, is therefore
checked exactly."""
import numpy as np

LATTICE = 16


def lattice_cloud(sizes, seed):
    """`sizes[b]` lattice points in batch element b (0: an empty element): float32 [n,3], sorted int32 batch ids [n]."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    pts = (rng.integers(0, LATTICE, size=(n, 3)).astype(np.float32) / np.float32(4.0)).astype(np.float32)
    bid = np.repeat(np.arange(len(sizes), dtype=np.int32), np.asarray(sizes, dtype=np.int64))
    return pts, bid


def squared_distances(src_pts, q, dtype=np.float32):
    """`dx*dx + dy*dy + dz*dz` of every source to the query `q`, every operation rounded to `dtype`."""
    d = src_pts.astype(dtype) - q.astype(dtype)[None, :]
    return ((d[:, 0] * d[:, 0]).astype(dtype) + (d[:, 1] * d[:, 1]).astype(dtype)).astype(dtype) + (d[:, 2] * d[:, 2]).astype(dtype)


def knn_pair(src_pts, src_bid, q_pts, q_bid, k, dtype=np.float32, order="lexsort"):
    """[n_q, k] int32: the k nearest sources of every query inside its batch element, ascending (squared distance, source
    index), -1 where the element has fewer than k sources.  `order`: "lexsort" on (distance, index), or "stable" -- a
    stable argsort of the distances of the candidates in ascending index order, the second formulation."""
    out = np.full((q_pts.shape[0], k), -1, dtype=np.int32)
    for i in range(q_pts.shape[0]):
        cand = np.nonzero(src_bid == q_bid[i])[0]
        if cand.size == 0:
            continue
        d = squared_distances(src_pts[cand], q_pts[i], dtype)
        if order == "lexsort":
            best = cand[np.lexsort((cand, d))]
        else:
            best = cand[np.argsort(d, kind="stable")]
        m = min(k, best.size)
        out[i, :m] = best[:m]
    return out


def knn_pair_padded(src_pts, src_bid, q_pts, q_bid, k, rows_q):
    """The table of the padded query: `knn_pair` on the present rows, -1 in the rows behind them."""
    out = np.full((rows_q, k), -1, dtype=np.int32)
    out[:q_pts.shape[0]] = knn_pair(src_pts, src_bid, q_pts, q_bid, k)
    return out


def edges(ids, capacity, n_valid=None):
    """(neighbors [min(E, capacity), 2] int32, ends [n_rows] int32, info [2]) of the table `ids` [n_rows, k]: row r lists
    (r, ids[r, j]) for the j in front of its first negative entry; rows from `n_valid` on have no edges."""
    n_rows, k = ids.shape
    valid = n_rows if n_valid is None else max(0, min(int(n_valid), n_rows))
    pairs, ends = [], np.zeros(n_rows, dtype=np.int64)
    total = 0
    for r in range(n_rows):
        if r < valid:
            for j in range(k):
                if ids[r, j] < 0:
                    break
                pairs.append((r, int(ids[r, j])))
                total += 1
        ends[r] = total
    nb = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)[:capacity]
    info = np.asarray([total, 1 if total > capacity else 0], dtype=np.int32)
    return nb, np.minimum(ends, capacity).astype(np.int32), info
