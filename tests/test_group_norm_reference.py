"""CPU: the numpy contract of include/se3conv_group_norm.h (tests/group_norm_reference.py) against the reference's own
`GroupNormPC` (tests/golden/group_norm.npz: forward and autograd gradients from the reference's Python) and against the same
formula in fp64 with two passes -- the bound is the project's fp32 whole-tensor one, `rel_err <= 2e-5` -- and the properties
the header promises of it: padded equals trimmed, an empty element, an id out of range, any order of the ids."""
import os

import numpy as np
import pytest

import group_norm_reference as R
from conftest import GOLDEN

BOUND = 2e-5
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "group_norm.npz"))


def both(x, gamma, beta, ids, nb, groups, g, frames=1, n_valid=None):
    y, mean, invstd = R.forward(x, gamma, beta, ids, nb, groups, R.EPS, frames, n_valid)
    dx, dgamma, dbeta = R.backward(g, x, gamma, mean, invstd, ids, nb, groups, frames, n_valid)
    return {"y": y, "dx": dx, "dgamma": dgamma, "dbeta": dbeta, "mean": mean, "invstd": invstd}


def test_the_fixture_is_the_one_the_issue_describes(fixture):
    ids = fixture["batch"]
    assert ids.shape[0] == 300 and sorted(np.bincount(ids).tolist()) == [47, 123, 130]
    assert fixture["shapes"].tolist() == [[16, 8], [24, 4], [8, 8]]
    assert os.path.getsize(os.path.join(GOLDEN, "group_norm.npz")) < os.path.getsize(os.path.join(GOLDEN, "resnetformer_block.npz"))


@pytest.mark.parametrize("c,groups", [(16, 8), (24, 4), (8, 8)])
def test_contract_matches_the_reference_fixture(fixture, c, groups):
    p = f"c{c}_g{groups}/"
    got = both(fixture[p + "x"], fixture[p + "gamma"], fixture[p + "betas"], fixture["batch"], 3, groups, fixture[p + "g"])
    for ours, theirs in (("y", "y"), ("dx", "dx"), ("dgamma", "dgamma"), ("dbeta", "dbetas")):
        e = R.rel_err(got[ours].reshape(-1), fixture[p + theirs].reshape(-1))
        print(f"C = {c}, G = {groups}: {ours} rel_err {e:.3e} (bound {BOUND:.0e})")
        assert e <= BOUND, (ours, e)


@pytest.mark.parametrize("c,groups", [(16, 8), (24, 4), (8, 8)])
def test_the_fixture_keeps_the_reference_itself_within_the_bound(fixture, c, groups):
    """The reference's fp32 result against the fp64 two-pass evaluation of its own formula."""
    p = f"c{c}_g{groups}/"
    want = R.two_pass_fp64(fixture[p + "x"], fixture[p + "gamma"], fixture[p + "betas"], fixture["batch"], 3, groups, fixture[p + "g"])
    for name, w in zip(("y", "dx", "dgamma", "dbetas"), want):
        e = R.rel_err(fixture[p + name].reshape(-1), w.reshape(-1))
        print(f"C = {c}, G = {groups}: reference's {name} against fp64 {e:.3e}")
        assert e <= BOUND, (name, e)


def planted(seed=5, points=300, c=16, groups=8, ratio=1e3):
    """Unit-variance rows in every group but group 3, whose values sit at `ratio` standard deviations from zero."""
    rng = np.random.default_rng(seed)
    ids = R.sized_ids([130, 47, 123])
    x = rng.standard_normal((points, c))
    for b in range(3):                                                   # exactly unit deviation per element, then the offset
        v = x[ids == b][:, 3::groups]
        x[np.ix_(ids == b, np.arange(c) % groups == 3)] = (v - v.mean()) / v.std() + ratio
    return (x.astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32), ids,
            rng.standard_normal((points, c)).astype(np.float32))


def test_contract_against_fp64_two_pass_with_a_mean_of_a_thousand_standard_deviations():
    """The one-pass variance E[x^2] - E[x]^2 of the contract, taken in fp64, on a group with |mean| / std = 1e3: the
    cancellation costs six of sixteen digits.  What remains is fp32: `save_mean` is rounded to a float, half an ulp of 1000 is
    3.1e-5 standard deviations, one group of eight carries it, so the whole-tensor error is at most 3.1e-5 / sqrt(8) = 1.1e-5
    plus the ordinary fp32 rounding of the row-wise pass."""
    x, gamma, beta, ids, g = planted()
    col = x[ids == 0][:, 3::8].astype(np.float64)
    assert 999 < abs(col.mean()) / col.std() < 1001
    got = both(x, gamma, beta, ids, 3, 8, g)
    want = R.two_pass_fp64(x, gamma, beta, ids, 3, 8, g)
    for name, w in zip(("y", "dx", "dgamma", "dbeta"), want):
        e = R.rel_err(got[name].reshape(-1), w.reshape(-1))
        print(f"planted |mean| / std = 1e3: {name} rel_err {e:.3e} (bound {BOUND:.0e})")
        assert e <= BOUND, (name, e)
    # the fp64 part alone: the saved inverse deviation of the planted group against the two-pass value
    d = col - col.mean()
    assert abs(got["invstd"][0, 3] / (1.0 / np.sqrt((d * d).mean() + 1e-8)) - 1.0) < 1e-6


def case(points, nb, c, frames, seed, empty=None, shuffle=None):
    rng = np.random.default_rng(seed)
    ids = R.sized_ids(R.split(points, nb, empty=empty), seed=shuffle)
    rows = points * frames
    x = (rng.standard_normal((rows, c)) * 1.5 + 0.25).astype(np.float32)
    return (x, rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32), ids,
            rng.standard_normal((rows, c)).astype(np.float32))


@pytest.mark.parametrize("valid", [0, 1, R.CHUNK + 1, 300])
def test_a_padded_call_is_the_trimmed_call_bit_for_bit(valid):
    rows, nb, c, groups, frames = 300, 3, 16, 8, 2
    x, gamma, beta, ids, g = case(rows, nb, c, frames, 11, shuffle=3)
    xt, idt = R.trimmed(x, ids, frames, valid)
    want = both(xt, gamma, beta, idt, nb, groups, g[:valid * frames], frames)
    xp, gp, idp = x.copy(), g.copy(), ids.copy()
    xp[valid * frames:], gp[valid * frames:], idp[valid:] = np.nan, np.nan, 0x7fffffff      # (absent rows hold anything)
    got = both(xp, gamma, beta, idp, nb, groups, gp, frames, n_valid=valid)
    for name in ("y", "dx"):
        assert np.array_equal(bits(got[name][:valid * frames]), bits(want[name])), name
        assert not bits(got[name][valid * frames:]).any(), name                                # +0.0 at absent rows
    for name in ("dgamma", "dbeta", "mean", "invstd"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name


def test_an_empty_element_has_zero_statistics_and_touches_nothing():
    x, gamma, beta, ids, g = case(2 * R.CHUNK + 3, 3, 24, 1, 12, empty=1)
    got = both(x, gamma, beta, ids, 3, 4, g)
    assert not bits(got["mean"][1]).any() and not bits(got["invstd"][1]).any()
    assert np.isfinite(got["y"]).all() and np.isfinite(got["dx"]).all()
    # the same rows as a two-element batch: the other elements' results do not change
    two = both(x, gamma, beta, np.where(ids == 2, 1, ids), 2, 4, g)
    assert np.array_equal(bits(two["y"]), bits(got["y"])) and np.array_equal(bits(two["dx"]), bits(got["dx"]))
    assert np.array_equal(bits(two["dgamma"]), bits(got["dgamma"]))


def test_a_point_with_an_id_out_of_range_gets_zero_rows_and_enters_no_sum():
    points, nb, c, groups, frames = R.CHUNK + 40, 3, 16, 8, 2
    x, gamma, beta, ids, g = case(points, nb, c, frames, 13)
    holes = ids.copy()
    holes[::7], holes[3::11] = -1, nb
    gone = (holes < 0) | (holes >= nb)
    got = both(x, gamma, beta, holes, nb, groups, g, frames)
    rows_gone = np.repeat(gone, frames)
    assert not bits(got["y"])[rows_gone].any() and not bits(got["dx"])[rows_gone].any()
    # the statistics are those of the cloud without these points, up to the order of the chunks they fall into
    keep = np.repeat(~gone, frames)
    want = both(x[keep], gamma, beta, holes[~gone], nb, groups, g[keep], frames)
    np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["y"][keep], want["y"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["dgamma"], want["dgamma"], rtol=1e-5, atol=1e-5)


def test_shuffled_ids_give_the_statistics_of_sorted_ids_up_to_the_order_of_additions():
    points, nb, c, groups, frames = 2 * R.CHUNK + 50, 3, 24, 4, 2
    x, gamma, beta, ids, g = case(points, nb, c, frames, 14)
    perm = np.random.default_rng(15).permutation(points)
    rows = (perm[:, None] * frames + np.arange(frames)[None, :]).reshape(-1)
    a = both(x, gamma, beta, ids, nb, groups, g, frames)
    b = both(x[rows], gamma, beta, ids[perm], nb, groups, g[rows], frames)
    # fp64 sums of a few hundred fp32 values in another order: equal to ~1e-13 before the rounding to float
    np.testing.assert_allclose(b["mean"], a["mean"], rtol=2e-7, atol=1e-9)
    np.testing.assert_allclose(b["invstd"], a["invstd"], rtol=2e-7)
    np.testing.assert_allclose(b["y"], a["y"][rows], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b["dx"], a["dx"][rows], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(b["dgamma"], a["dgamma"], rtol=1e-6, atol=1e-6)


def test_the_chunk_of_the_header_is_the_chunk_here():
    import re
    from se3conv3d_amd import _lib

    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "se3conv_group_norm.h")).read()
    k = int(re.search(r"#define SE3_GROUP_NORM_CHUNK (\d+)", header).group(1))
    assert k == R.CHUNK == _lib.GROUP_NORM_CHUNK and k & (k - 1) == 0
