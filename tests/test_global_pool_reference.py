"""CPU: tests/global_pool_reference.py, the contract of include/se3conv_global_pool.h in numpy, against what it must agree
with and the properties the header promises."""
import os
import re

import numpy as np
import pytest

import global_pool_reference as R
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def features(rows, c, seed):
    return (np.random.default_rng(seed).standard_normal((rows, c)) * 1.5 + 0.25).astype(np.float32)


def ulp_distance(a, b):
    """Distance in representable float32 values (finite inputs)."""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def test_chunk_is_the_headers_and_the_bindings():
    text = open(os.path.join(ROOT, "include", "se3conv_global_pool.h")).read()
    assert int(re.search(r"#define SE3_GLOBAL_POOL_CHUNK (\d+)", text).group(1)) == R.CHUNK
    assert R.CHUNK & (R.CHUNK - 1) == 0
    from se3conv3d_amd import _lib, ops
    assert _lib.GLOBAL_POOL_CHUNK == R.CHUNK and ops.POOL_MODES == R.MODES


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("shuffled", [False, True])
def test_sums_and_extrema_are_those_of_fp64_scatter_reductions_within_one_ulp(frames, shuffled):
    points, nb, c = 2 * R.CHUNK + 300, 5, 7
    ids = R.sized_ids(R.split(points, nb, empty=2), seed=3 if shuffled else None)
    x = features(points * frames, c, 10 + frames)
    row_ids = np.repeat(ids, frames)
    exact = np.zeros((nb, c))
    np.add.at(exact, row_ids, x.astype(np.float64))
    n = np.bincount(ids, minlength=nb)
    s, _, counts = R.global_pool(x, ids, nb, R.SUM, frames)
    a, arg, _ = R.global_pool(x, ids, nb, R.AVG, frames)
    assert counts.tolist() == n.tolist() and counts[2] == 0 and bool((arg == -1).all())
    assert ulp_distance(s, exact.astype(np.float32)).max() <= 1
    live = n > 0
    assert ulp_distance(a[live], (exact[live] / (n[live, None] * frames)).astype(np.float32)).max() <= 1
    assert not s[2].any() and not a[2].any() and not np.signbit(s[2]).any()
    for mode, at, start in ((R.MAX, np.maximum.at, -np.inf), (R.MIN, np.minimum.at, np.inf)):
        want = np.full((nb, c), start)
        at(want, row_ids, x.astype(np.float64))
        got, arg, _ = R.global_pool(x, ids, nb, mode, frames)
        assert np.array_equal(got[live], want[live].astype(np.float32)) and not got[2].any() and bool((arg[2] == -1).all())
        assert np.array_equal(x[arg[live], np.arange(c)], got[live])                 # arg names a row that holds the value
        assert np.array_equal(row_ids[arg[live]], np.repeat(np.flatnonzero(live)[:, None], c, 1))


def test_closed_form_of_the_extremum_is_the_rule_ties_and_nan_included():
    rng = np.random.default_rng(4)
    v = rng.integers(-3, 4, size=(40, 9)).astype(np.float32)               # many ties
    v[0, 1] = v[5, 2] = v[39, 3] = np.nan                                  # a NaN seed stays, a later NaN never replaces
    v[:, 4] = np.nan
    v[:, 5] = -np.inf
    v[:, 6] = np.inf
    rows = np.sort(rng.choice(1000, size=40, replace=False))
    for is_max in (True, False):
        b0, a0 = R.pool_extremum_by_rule(v, rows, is_max)
        b1, a1 = R.pool_extremum(v, rows, is_max)
        assert np.array_equal(b0, b1, equal_nan=True) and np.array_equal(a0, a1)
        assert np.isnan(b0[1]) and a0[1] == rows[0] and not np.isnan(b0[2]) and not np.isnan(b0[3])
    best, arg = R.pool_extremum(v, rows, True)
    col = v[:, 0]
    assert arg[0] == rows[np.flatnonzero(col == col.max())[0]]             # ties: the lowest row


def test_hierarchy_fixture():
    """The bound test_gpu_hierarchy.py holds the torch path to; the contract's own distance is printed (3.7e-8 when written)."""
    d = np.load(os.path.join(GOLDEN, "hierarchy.npz"))
    f, ids = int(d["frames"]), d["gpool_batch"]
    worst = 0.0
    for method in ("avg", "max"):
        x = d[f"gpool_{method}_x"]
        y = R.global_pool(x, ids, 1, R.MODES[method], f)[0]
        pooled = x.reshape(ids.shape[0], f, -1).max(1)
        y2 = R.global_pool(pooled, ids, 1, R.MODES[method], 1)[0]
        worst = max(worst, float(np.abs(y - d[f"gpool_{method}_y"]).max()), float(np.abs(y2 - d[f"gpool2_{method}_y"]).max()))
        np.testing.assert_allclose(y, d[f"gpool_{method}_y"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(y2, d[f"gpool2_{method}_y"], rtol=0, atol=1e-6)
    print(f"largest distance to the fixture: {worst:.2e}")


@pytest.mark.parametrize("valid", [0, 1, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 77])
def test_padded_equals_trimmed(valid):
    n_rows, nb, c, frames = 2 * R.CHUNK + 500, 4, 5, 2
    ids = R.sized_ids(R.split(n_rows, nb), seed=8)
    x = features(n_rows * frames, c, 9)
    xp, idp = x.copy(), ids.copy()
    xp[valid * frames:], idp[valid:] = np.nan, 0x7fffffff                 # what stands behind the word is not looked at
    xt, idt = R.trimmed(x, ids, frames, valid)
    for mode in range(4):
        got, want = R.global_pool(xp, idp, nb, mode, frames, valid), R.global_pool(xt, idt, nb, mode, frames)
        assert all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want)), mode
        g = features(nb, c, 12)
        back = R.global_unpool(g, idp, got[1], got[2], mode, frames, valid)
        assert np.array_equal(back[:valid * frames].view(np.int32), R.global_unpool(g, idt, want[1], want[2], mode, frames).view(np.int32))
        assert not back[valid * frames:].view(np.int32).any()
    # a word past the buffer is clamped
    assert R.present_points(n_rows, n_rows + 5) == n_rows and R.present_points(n_rows, -3) == 0 and R.present_points(n_rows, None) == n_rows


def test_unsorted_and_out_of_range_ids():
    points, nb, c = R.CHUNK + 200, 3, 4
    ids = R.sized_ids(R.split(points, nb), seed=5)
    assert (np.diff(ids) < 0).any()
    ids[::17] = -1
    ids[5::29] = nb
    x = features(points, c, 6)
    keep = (ids >= 0) & (ids < nb)
    for mode in range(4):
        out, arg, counts = R.global_pool(x, ids, nb, mode)
        assert counts.tolist() == np.bincount(ids[keep], minlength=nb).tolist()
        back = R.global_unpool(features(nb, c, 7), ids, arg, counts, mode)
        assert not back[~keep].view(np.int32).any()                       # a point of no element gets a zero row
        if mode in (R.MAX, R.MIN):
            assert keep[arg].all()
    # the order of the ids does not enter a max, and enters a sum only through the order of its additions
    order = np.argsort(ids, kind="stable")
    s0, s1 = R.global_pool(x, ids, nb, R.SUM)[0], R.global_pool(x[order], ids[order], nb, R.SUM)[0]
    assert ulp_distance(s0, s1).max() <= 1
    assert np.array_equal(R.global_pool(x, ids, nb, R.MAX)[0], R.global_pool(x[order], ids[order], nb, R.MAX)[0])


def test_negative_zero_rows_give_a_positive_zero_sum():
    x = np.full((6, 3), -0.0, dtype=np.float32)
    ids = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    for mode in (R.SUM, R.AVG):
        out = R.global_pool(x, ids, 3, mode)[0]
        assert not out.view(np.int32).any()                              # +0.0 by its bits, the empty element included
    assert np.signbit(R.global_pool(x, ids, 3, R.MAX)[0][:2]).all()       # an extremum is a copy of its row


def test_unpool_is_the_gradient_of_the_pool():
    points, nb, c, frames = 300, 3, 4, 2
    ids = R.sized_ids(R.split(points, nb, empty=1))
    x, g = features(points * frames, c, 1), features(nb, c, 2)
    row_ids = np.repeat(ids, frames)
    for mode in range(4):
        out, arg, counts = R.global_pool(x, ids, nb, mode, frames)
        back = R.global_unpool(g, ids, arg, counts, mode, frames)
        if mode == R.SUM:
            assert np.array_equal(back, g[row_ids])
        elif mode == R.AVG:
            assert np.array_equal(back, g[row_ids] / np.float32(1)  / (counts[row_ids, None] * frames).astype(np.float32))
        else:
            want = np.zeros_like(back)
            live = counts > 0
            want[arg[live], np.arange(c)] = g[live]
            assert np.array_equal(back, want)
