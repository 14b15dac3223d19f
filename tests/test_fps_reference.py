"""CPU: the numpy statement of the farthest-point contract (tests/fps_reference.py) has the properties
include/se3conv_fps.h promises -- on the 8x8x8 integer lattice (ties everywhere) and on 64 rows that sit on 5 positions."""
import numpy as np
import pytest

import fps_reference as R

CASES = {"lattice": R.lattice(8), "duplicates": R.duplicates(64, 5)}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("ratio", [1.0, 0.25, 0.013])
@pytest.mark.parametrize("first", [0, 17])
def test_reference_properties(name, ratio, first):
    pts = CASES[name]
    n = len(pts)
    m = R.sample_count(n, ratio)
    assert m == min(n, int(np.ceil(np.float32(n) * np.float32(ratio)))) and 1 <= m <= n
    ids, d2 = R.fps_element(pts, m, first)
    assert ids[0] == first and np.isinf(d2[0])
    assert len(set(ids.tolist())) == m and ids.min() >= 0 and ids.max() < n          # distinct, in range
    assert np.all(np.diff(d2) <= 0)                                                   # non-increasing
    # every pick attains the maximum of mind over the unmarked rows, at the lowest such row
    mind = np.full(n, np.inf, dtype=np.float32)
    marked = np.zeros(n, dtype=bool)
    for j in range(m):
        if j:
            free = np.flatnonzero(~marked)
            top = mind[free].max()
            assert mind[ids[j]] == top == d2[j] and ids[j] == free[mind[free] == top][0] and not marked[ids[j]]
        marked[ids[j]] = True
        d = pts.astype(np.float64) - pts[ids[j]].astype(np.float64)
        # (the lattice's and the duplicates' own distances: exact in fp32 on the lattice, so fp64 agrees there)
        mind = np.fmin(mind, R.dist2(pts, ids[j]))
        if name == "lattice":
            assert np.array_equal(R.dist2(pts, ids[j]), (d * d).sum(1).astype(np.float32))


def test_duplicates_at_ratio_one_are_a_permutation_with_zero_radius_from_the_sixth_pick():
    pts = CASES["duplicates"]
    ids, d2 = R.fps_element(pts, 64, 0)
    assert sorted(ids.tolist()) == list(range(64))
    assert np.all(d2[1:5] > 0) and np.all(d2[5:] == 0)
    assert len({tuple(p) for p in pts[ids[:5]].tolist()}) == 5


def test_batched_reference_counts_starts_and_absent_elements():
    rng = np.random.default_rng(0)
    sizes = [1, 37, 500, 0, 65]
    pts = rng.standard_normal((sum(sizes), 3)).astype(np.float32)
    bid = np.repeat(np.arange(5), sizes).astype(np.int32)
    for ratio in (1.0, 0.25, 0.013):
        ids, d2, starts = R.fps_reference(pts, bid, ratio, 5)
        want = [R.sample_count(n, ratio) for n in sizes]
        assert want[3] == 0 and np.diff(starts).tolist() == want and starts[0] == 0 and len(ids) == len(d2) == starts[-1]
        lo = np.concatenate([[0], np.cumsum(sizes)])
        for b in range(5):
            e = ids[starts[b]:starts[b + 1]]
            assert np.all((e >= lo[b]) & (e < lo[b + 1])) and len(set(e.tolist())) == len(e)
            if len(e):
                assert e[0] == lo[b]
    u = np.array([0.0, 0.5, 0.999, 0.3, 0.25], dtype=np.float32)
    ids, _, starts = R.fps_reference(pts, bid, 0.25, 5, u)
    assert [int(ids[starts[b]] - lo[b]) for b in (0, 1, 2, 4)] == [0, 18, 499, 16]
