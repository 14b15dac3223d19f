"""GPU: the device entry points of include/se3conv_knn_edges.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py)
-- the policy of tests/test_gpu_padded_hostile_memory.py: the clouds, the id tables, every output and the workspace (sized to
exactly the query's value) come from an arena, so the absent rows hold the arena's fill (NaN points, batch id -1, id -1); no
band byte changes, the results are those of the numpy reference whatever the workspace held, every output byte is a result
or the stated pad, and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import hostile_memory
import knn_edges_reference as R
from hostile_memory import Arena, in_arena
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_knn_edges.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_knn_query_pair_padded": ["test_pair_query", "test_pair_query_then_edges"],
    "se3_knn_edges_bounded": ["test_pair_query_then_edges", "test_edges_of_tables"],
}
SRC, QUERY = (50, 0, 100), (30, 60, 0)      # per batch element: one with queries but no source, one with sources but no query
ROWS_SRC, ROWS_Q = 256, 128


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the second registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_knn_edges.h", _lib.KNN_EDGES_SIGNATURES)


@pytest.fixture(scope="module")
def clouds():
    ps, bs = R.lattice_cloud(SRC, 1)
    pq, bq = R.lattice_cloud(QUERY, 2)
    return ps, bs, pq, bq


def guarded(request, workspace_fill, workspace):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=workspace)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def arena_clouds(arena, clouds):
    ps, bs, pq, bq = clouds
    out = in_arena(arena, t(ps), ROWS_SRC), in_arena(arena, t(bs), ROWS_SRC), in_arena(arena, t(pq), ROWS_Q), in_arena(arena, t(bq), ROWS_Q)
    assert torch.isnan(out[0][ps.shape[0]:]).all() and bool((out[3][pq.shape[0]:] == -1).all())
    return out


@pytest.mark.parametrize("k", [8, 64])
def test_pair_query(ops, clouds, request, k):
    ps, bs, pq, bq = clouds
    want = R.knn_pair_padded(ps, bs, pq, bq, k, ROWS_Q)
    with guarded(request, 0xFF, workspace=False) as arena:
        p_s, b_s, p_q, b_q = arena_clouds(arena, clouds)
        ws_, wq_ = arena.place(torch.tensor([ps.shape[0]], dtype=torch.int32)), arena.place(torch.tensor([pq.shape[0]], dtype=torch.int32))
        ids = ops.knn_query_pair(p_s, b_s, p_q, b_q, k, n_valid_src=ws_, n_valid_q=wq_)
        assert np.array_equal(ids.cpu().numpy(), want)                   # (every byte written: the absent rows are -1 by value)
        # no present source: every entry -1, nothing of the source buffers read; no present query: likewise
        zero = arena.place(torch.zeros(1, dtype=torch.int32))
        assert bool((ops.knn_query_pair(p_s, b_s, p_q, b_q, k, n_valid_src=zero, n_valid_q=wq_) == -1).all())
        assert bool((ops.knn_query_pair(p_s, b_s, p_q, b_q, k, n_valid_src=ws_, n_valid_q=zero) == -1).all())
        # one word only: the other cloud is whole (its buffer then holds only present rows)
        whole_q = arena.place(t(pq)), arena.place(t(bq))
        ids_q = ops.knn_query_pair(p_s, b_s, *whole_q, k, n_valid_src=ws_)
        assert np.array_equal(ids_q.cpu().numpy(), want[:pq.shape[0]])


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_pair_query_then_edges(ops, clouds, request, workspace_fill):
    ps, bs, pq, bq = clouds
    k = 16
    table = R.knn_pair_padded(ps, bs, pq, bq, k, ROWS_Q)
    e = int(R.edges(table, ROWS_Q * k, pq.shape[0])[2][0])
    assert 0 < e < pq.shape[0] * k
    with guarded(request, workspace_fill, workspace=True) as arena:
        p_s, b_s, p_q, b_q = arena_clouds(arena, clouds)
        ws_, wq_ = arena.place(torch.tensor([ps.shape[0]], dtype=torch.int32)), arena.place(torch.tensor([pq.shape[0]], dtype=torch.int32))
        ids = ops.knn_query_pair(p_s, b_s, p_q, b_q, k, n_valid_src=ws_, n_valid_q=wq_)
        for cap in (ROWS_Q * k, e + 77, e, e - 1, e // 2, 0):
            nb, ends, info = ops.knn_edges_bounded(ids, cap, n_valid=wq_)
            w_nb, w_ends, w_info = R.edges(table, cap, pq.shape[0])
            kept = min(e, cap)
            assert info.tolist() == w_info.tolist() == [e, int(e > cap)]
            assert np.array_equal(ends.cpu().numpy(), w_ends) and np.array_equal(nb[:kept].cpu().numpy(), w_nb)
            assert Arena.holds_fill(nb[kept:])                           # rows [E, capacity): the stated untouched region
            across_fills(("pair", cap), workspace_fill, (nb[:kept], ends, info))


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_edges_of_tables(ops, request, workspace_fill):
    """Tables placed in the arena directly: the rows behind the word hold valid-looking ids, which must not be listed."""
    rng = np.random.default_rng(5)
    n_rows, k = 300, 8
    table = np.full((n_rows, k), -1, dtype=np.int32)
    for r in range(n_rows):
        m = int(rng.integers(0, k + 1))
        table[r, :m] = rng.integers(0, 1000, size=m)
    with guarded(request, workspace_fill, workspace=True) as arena:
        ids = arena.place(t(table))
        for valid in (n_rows, 257, 256, 1, 0):
            w = arena.place(torch.tensor([valid], dtype=torch.int32))
            e = int(R.edges(table, n_rows * k, valid)[2][0])
            for cap in sorted({n_rows * k, e, max(e - 1, 0), 0}):
                nb, ends, info = ops.knn_edges_bounded(ids, cap, n_valid=w)
                w_nb, w_ends, w_info = R.edges(table, cap, valid)
                kept = min(e, cap)
                assert info.tolist() == w_info.tolist()
                assert np.array_equal(ends.cpu().numpy(), w_ends) and np.array_equal(nb[:kept].cpu().numpy(), w_nb)
                assert Arena.holds_fill(nb[kept:])
                across_fills(("table", valid, cap), workspace_fill, (nb[:kept], ends, info))
        # without a word every row is present; no rows at all: info = (0, 0) and nothing else is touched
        nb, ends, info = ops.knn_edges_bounded(ids, n_rows * k)
        assert info.tolist() == R.edges(table, n_rows * k)[2].tolist()
        nb, ends, info = ops.knn_edges_bounded(arena.alloc((0, k), torch.int32), 9)
        assert info.tolist() == [0, 0] and ends.numel() == 0 and Arena.holds_fill(nb)
