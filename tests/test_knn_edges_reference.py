"""CPU: the numpy reference of tests/knn_edges_reference.py against a second formulation of the k-NN order, the exactness of
the lattice clouds the GPU tests use, and the edge builder on hand-written tables."""
import numpy as np
import pytest

import knn_edges_reference as R

# (source sizes, query sizes) per batch element: the layouts of tests/test_gpu_knn_edges.py
LAYOUTS = [((50, 0, 100), (30, 60, 0)), ((5, 0, 145), (30, 60, 0))]


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
@pytest.mark.parametrize("k", [1, 8, 16, 32, 64])
def test_lexsort_and_stable_argsort_give_the_same_tables(layout, k):
    src, q = LAYOUTS[layout]
    ps, bs = R.lattice_cloud(src, 1)
    pq, bq = R.lattice_cloud(q, 2)
    a = R.knn_pair(ps, bs, pq, bq, k)
    b = R.knn_pair(ps, bs, pq, bq, k, order="stable")
    assert np.array_equal(a, b)
    # what the table must look like: valid prefix, ids of the query's element, -1 exactly where the element is too small
    per_element = np.bincount(bs, minlength=len(src))
    for i in range(pq.shape[0]):
        m = min(k, per_element[bq[i]])
        assert (a[i, :m] >= 0).all() and (a[i, m:] == -1).all() and (bs[a[i, :m]] == bq[i]).all()
        assert len(set(a[i, :m].tolist())) == m


@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_fp32_and_fp64_squared_distances_agree_bit_for_bit_on_the_lattice(layout):
    src, q = LAYOUTS[layout]
    ps, _ = R.lattice_cloud(src, 1)
    pq, _ = R.lattice_cloud(q, 2)
    ties = 0
    for i in range(pq.shape[0]):
        d32, d64 = R.squared_distances(ps, pq[i], np.float32), R.squared_distances(ps, pq[i], np.float64)
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64)
        assert np.array_equal(d64 * 16, np.round(d64 * 16))             # multiples of 1/16
        ties += d64.size - np.unique(d64).size
    assert ties > 1000                                                   # the index half of the order is exercised


def test_fp32_and_fp64_tables_agree_on_the_lattice():
    src, q = LAYOUTS[0]
    ps, bs = R.lattice_cloud(src, 1)
    pq, bq = R.lattice_cloud(q, 2)
    assert np.array_equal(R.knn_pair(ps, bs, pq, bq, 16), R.knn_pair(ps, bs, pq, bq, 16, dtype=np.float64))


T = np.array([[3, 1, -1, -1],      # two edges
              [-1, -1, -1, -1],    # an empty row
              [0, 1, 2, 3],        # a full row
              [2, -1, 7, -1]],     # behind the first negative entry nothing is looked at
             dtype=np.int32)
FULL = [(0, 3), (0, 1), (2, 0), (2, 1), (2, 2), (2, 3), (3, 2)]


def test_edge_builder_on_a_hand_written_table():
    nb, ends, info = R.edges(T, 16)
    assert nb.tolist() == [list(p) for p in FULL] and ends.tolist() == [2, 2, 6, 7] and info.tolist() == [7, 0]
    assert nb.dtype == np.int32 and ends.dtype == np.int32


@pytest.mark.parametrize("capacity,flag", [(7, 0), (6, 1), (0, 1)])
def test_edge_builder_truncates_at_the_capacity(capacity, flag):
    nb, ends, info = R.edges(T, capacity)
    assert nb.tolist() == [list(p) for p in FULL[:capacity]]
    assert ends.tolist() == [min(e, capacity) for e in (2, 2, 6, 7)] and info.tolist() == [7, flag]


def test_edge_builder_with_all_rows_empty_and_with_absent_rows():
    nb, ends, info = R.edges(np.full((3, 4), -1, dtype=np.int32), 5)
    assert nb.shape == (0, 2) and ends.tolist() == [0, 0, 0] and info.tolist() == [0, 0]
    nb, ends, info = R.edges(T, 16, n_valid=2)                          # rows 2 and 3 are absent: flat offsets
    assert nb.tolist() == [[0, 3], [0, 1]] and ends.tolist() == [2, 2, 2, 2] and info.tolist() == [2, 0]
    nb, ends, info = R.edges(T, 16, n_valid=0)
    assert nb.shape == (0, 2) and ends.tolist() == [0] * 4 and info.tolist() == [0, 0]
    nb, ends, info = R.edges(T, 16, n_valid=9)                          # clamped to the row count
    assert info.tolist() == [7, 0]
