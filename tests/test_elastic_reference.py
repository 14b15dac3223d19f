"""CPU: tests/elastic_reference.py (the numpy restatement of include/se3conv_elastic.h) against what the reference's own class
did -- tests/golden/elastic_steps.npz, written by tools/gen_golden_elastic.py: input clouds, the raw grids `torch.randn`
returned, and ElasticDistortionAug's output.  The bound is the project's usual one, 8 x the fp32 emulation
`max|restatement fp32 - restatement fp64|` on the same inputs; every misreading of the reference's lines, planted one at a
time, must break it."""
import os

import numpy as np
import pytest

import augment_reference as R
import elastic_reference as E

F = np.float32
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "elastic_steps.npz"))
CLOUDS = range(int(GOLDEN["clouds"]))
GRAN, MAG = GOLDEN["granularity"].tolist(), GOLDEN["magnitude"].tolist()
MISREADINGS = ("no_swap", "align_corners_false", "one_blur_round", "zero_padding", "moved_box", "unmoved")


def case(i):
    pts, out = GOLDEN[f"{i}/pts"], GOLDEN[f"{i}/out"]
    raws = [np.moveaxis(GOLDEN[f"{i}/noise{l}"], 0, -1) for l in range(len(GRAN))]   # [3, nx, ny, nz] -> [nx, ny, nz, 3]
    st = R.stats(pts, np.zeros(len(pts), dtype=np.int32), 1)[1][0]
    return pts, out, raws, st


def run(pts, raws, st, dtype, misreading=None):
    flags = {} if misreading in (None, "one_blur_round") else {misreading: True}
    fields = [E.blur(r, 1 if misreading == "one_blur_round" else 2, dtype) for r in raws]
    return E.distort(pts, st[0:3], st[3:6], fields, MAG, dtype, **flags)


def bound(pts, raws, st):
    return 8.0 * float(np.abs(run(pts, raws, st, F).astype(np.float64) - run(pts, raws, st, np.float64)).max())


@pytest.mark.parametrize("i", CLOUDS)
def test_dims_are_the_shapes_torch_drew(i):
    pts, _, raws, st = case(i)
    assert E.dims_of(st, GRAN).tolist() == [list(r.shape[0:3]) for r in raws]
    table, flag, prefix = E.plan(np.array([len(pts)], dtype=np.int32), st[None], np.zeros((1, R.DRAWS), dtype=F), 1.0, GRAN, 1 << 20)
    assert flag == 0 and table[0, :, 0:3].tolist() == [list(r.shape[0:3]) for r in raws]
    assert table[0, :, 3].tolist() == np.concatenate(([0], np.cumsum([r[..., 0].size for r in raws])[:-1])).tolist()
    assert prefix[-1] == sum(E.tiles_of(r.shape[0:3]) for r in raws)


def test_the_fixture_holds_the_edge_dims():
    shapes = [GOLDEN[f"{i}/noise{l}"].shape[1:] for i in CLOUDS for l in range(len(GRAN))]
    assert (15, 11, 7) in shapes and any(3 in s for s in shapes)                        # the thinnest axis of one cloud: n = 3
    assert [len(GOLDEN[f"{i}/pts"]) for i in CLOUDS][:2] == list(R.GOLDEN_SIZES)
    assert GRAN == [0.1, 0.2, 0.4] and MAG == [0.15, 0.3, 0.6]                           # the ScanNet step


@pytest.mark.parametrize("i", CLOUDS)
def test_restatement_is_the_reference(i):
    pts, out, raws, st = case(i)
    got = run(pts, raws, st, F)
    err, cap = float(np.abs(got.astype(np.float64) - out).max()), bound(pts, raws, st)
    print(f"cloud {i}: |restatement - reference| {err:.3e}, bound {cap:.3e}, ratio to the emulation {8 * err / cap:.2f}, "
          f"largest displacement {float(np.abs(out - pts).max()):.3f}")
    assert got.dtype == F and cap > 0 and err <= cap
    assert float(np.abs(out - pts).max()) > 0.05                                         # (something was displaced at all)


@pytest.mark.parametrize("misreading", MISREADINGS)
@pytest.mark.parametrize("i", CLOUDS)
def test_planted_misreadings_break_the_bound(i, misreading):
    pts, out, raws, st = case(i)
    err = float(np.abs(run(pts, raws, st, F, misreading).astype(np.float64) - out).max())
    assert err > bound(pts, raws, st), misreading


def test_blur_is_the_contracts_formula():
    """One pass on a line of ones: 1/3 + 1/3 at the ends (a zero outside), the three-term sum inside, in the stated order."""
    t = F(1.0 / 3.0)
    v = np.ones((4, 1, 1, 1), dtype=F)
    w = np.pad(v, [(1, 1), (0, 0), (0, 0), (0, 0)])
    x_pass = ((w[0:4] * t) + (w[1:5] * t)) + (w[2:6] * t)
    assert x_pass[:, 0, 0, 0].tolist() == [(F(0) * t + t) + t, (t + t) + t, (t + t) + t, (t + t) + F(0) * t]
    rng = np.random.default_rng(0)
    raw = rng.standard_normal((5, 4, 3, 3)).astype(F)
    once = E.blur(raw, 1)
    by_hand = raw.copy()
    for a in range(3):
        pad = [(0, 0)] * 4
        pad[a] = (1, 1)
        w = np.pad(by_hand, pad)
        sl = lambda s: tuple(slice(s, s + by_hand.shape[a]) if k == a else slice(None) for k in range(4))  # noqa: E731
        by_hand = ((w[sl(0)] * t) + (w[sl(1)] * t)) + (w[sl(2)] * t)
    assert np.array_equal(once.view(np.uint32), by_hand.view(np.uint32))
    # interior variance of two rounds on white noise: (19/81)^3
    big = E.blur(rng.standard_normal((24, 24, 24, 3)), 2, np.float64)[4:-4, 4:-4, 4:-4]
    assert abs(float(big.var()) / (19.0 / 81.0) ** 3 - 1.0) < 0.25


def test_hashed_normals_are_keyed_by_element_and_octave():
    a = E.hashed_normals(5, 3, 1, 2, (4, 3, 3))
    assert a.shape == (4, 3, 3, 3) and a.dtype == F
    assert np.array_equal(a.reshape(-1, 3), R.gaussian(int(R.h(5, 3, 1 * E.MAX_OCTAVES + 2)), 0, np.arange(36)))
    for other in ((6, 3, 1, 2), (5, 4, 1, 2), (5, 3, 2, 2), (5, 3, 1, 1)):
        assert not np.array_equal(a, E.hashed_normals(*other, (4, 3, 3)))
    # a larger grid of the same entry is another field cell by cell only through q: the prefix of local indices is shared
    assert np.array_equal(E.hashed_normals(5, 3, 1, 2, (8, 3, 3)).reshape(-1, 3)[:36], a.reshape(-1, 3))


def test_plan_rules():
    g = [0.5, 1.0]
    st = np.zeros((5, 12), dtype=F)
    st[:, 3:6] = [[1.0, 2.0, 0.4]] * 5
    st[3, 3] = np.inf
    counts = np.array([10, 0, 10, 10, 10], dtype=np.int32)
    draws = np.zeros((5, R.DRAWS), dtype=F)
    draws[2, 0] = 0.9                                                                   # closed by the gate
    cells = 5 * 7 * 3 + 4 * 5 * 3
    table, flag, prefix = E.plan(counts, st, draws, 0.5, g, 2 * cells)
    assert flag == 2 and table[:, 0, 3].tolist() == [0, -1, -1, -1, cells] and table[4, 1, 3] == cells + 105
    assert table[0, :, 0:3].tolist() == [[5, 7, 3], [4, 5, 3]] and not table[[1, 2, 3], :, 0:3].any()
    assert prefix.tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 2, 3, 4]
    table, flag, _ = E.plan(counts, st, draws, 0.5, g, 2 * cells - 1)                   # one cell short: the last element stays out
    assert flag == 3 and table[:, :, 3].tolist() == [[0, 105], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
    assert table[4, :, 0:3].tolist() == [[5, 7, 3], [4, 5, 3]]                          # (its dims are still told)
    table, flag, _ = E.plan(counts, st, draws, 0.5, g, 0)
    assert flag == 3 and (table[:, :, 3] == -1).all()
