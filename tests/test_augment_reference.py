"""CPU: the numpy restatement of include/se3conv_augment.h (tests/augment_reference.py) against what the reference's own
augmentation classes returned (tests/golden/augment_steps.npz, tools/gen_golden_augment.py), fed the numbers the classes drew.

Removing steps and the noise are held exactly (masks, surviving rows, the clipped sum).  Affine steps are held PER ELEMENT
against the element's own scale `sqrt(sum_i (x_i M_ij)^2 + t_j^2)`, the way tests/rowwise_error.py holds the operator: the
reference of the comparison is the restatement run in fp64 throughout, the bound of a case is 8 x the largest ratio the
restatement run in fp32 reaches against it IN THAT CASE, with a floor of one fp32 rounding (2^-24) under the emulation
(python tests/test_augment_reference.py prints the table that profiles/augment.txt holds) -- never a figure of the library.  The planted faults at the end are the ones a whole-tensor norm
lets through.  The elastic step is not implemented, so neither its cases nor its planted fault (the x/z swap) are here."""
import os

import numpy as np
import pytest

import augment_reference as R
from conftest import GOLDEN

F = np.float32
AFFINE_CASES = ("rot_z", "rot_x_fixed", "rot_y_small", "rot3d", "rot3d_axis1", "center", "linear_single", "linear_channels", "mirror",
                "translation", "stdnorm")
FACTOR = 8.0
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "augment_steps.npz")) as z:
        return {k: z[k] for k in z.files}


def batch_of(golden, case):
    """The case's two clouds as one batch: pts, ids, extra, per-element records."""
    recs = [{k: golden[f"{case}/{i}/{k}"] for k in ("pts", "extra", "out", "extra_out", "rand", "randn", "randint")} for i in range(len(R.GOLDEN_SIZES))]
    ids = np.concatenate([np.full(len(r["pts"]), i, dtype=np.int32) for i, r in enumerate(recs)])
    return np.concatenate([r["pts"] for r in recs]), ids, np.concatenate([r["extra"] for r in recs]), recs


def draws_of(kind, consts, recs):
    """The recorded numbers of the classes in the columns the header gives them (column 0, the gate, stays 0: open)."""
    d = np.zeros((len(recs), R.DRAWS), dtype=F)
    for b, r in enumerate(recs):
        u = r["rand"]
        if kind in ("rot_axis", "rot_3d") and u.size:
            d[b, 1] = u[0]
        elif kind == "linear":
            if consts[4]:
                d[b, 1], d[b, 4] = u[0], u[1]
            else:
                d[b, 1:4], d[b, 4:7] = u[0:3], u[3:6]
        elif kind in ("mirror", "translation"):
            d[b, 1:4] = u[0:3]
        elif kind == "crop_box":
            d[b, 1:7] = u[0:6]
        elif kind == "crop_pts" and r["randint"].size:
            n = len(r["pts"])
            d[b, 1] = F((int(r["randint"][0]) + 0.5) / n)
            assert int(np.floor(d[b, 1] * F(n))) == int(r["randint"][0])
    return d


def run_affine(golden, case, dtype, **fault):
    """(table, out, extra_out) of the restated stats -> affine_step -> apply in `dtype`."""
    cfg = R.GOLDEN_CASES[case]
    pts, ids, extra, recs = batch_of(golden, case)
    nb = len(recs)
    table = R.identity(nb, dtype)
    for b in range(nb):   # (the fixed-angle case took the next epoch's value for its second cloud)
        kind, consts, prob, _, _ = R.spec_of(cfg, 1 if (cfg.get("p_angle_values") is not None and b == 1) else 0)
        draws = draws_of(kind, consts, recs)
        counts, st = R.stats(pts, ids, nb, None, None, fault.get("unbiased", True), dtype) if kind in R.NEEDS_STATS else (None, None)
        normals = [r["randn"] for r in recs] if (kind == "rot_3d" and consts[0] < 0) else None
        table[b] = R.affine_step(kind, consts, prob, draws, R.identity(nb, dtype), counts, st, normals=normals)[b]
    return table, R.apply(pts, ids, nb, table, dtype=dtype), R.apply(extra, ids, nb, table, dtype=dtype)


def element_scales(x, ids, table):
    x64, m = x.astype(np.float64), table.astype(np.float64)[ids]
    mm, t = m[:, 0:9].reshape(-1, 3, 3), m[:, 9:12]
    return np.sqrt(((x64[:, :, None] * mm) ** 2).sum(1) + t * t)


def ratio(a, b, s):
    live = s > 0
    assert np.array_equal(a[~live], b[~live])
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64))[live] / s[live]).max()) if live.any() else 0.0


def affine_table(golden):
    """{case: (emulation, reference vs fp64, restatement vs reference)} for points and extra tensor together."""
    rows = {}
    for case in AFFINE_CASES:
        pts, ids, extra, recs = batch_of(golden, case)
        t64, o64, e64 = run_affine(golden, case, np.float64)
        t32, o32, e32 = run_affine(golden, case, F)
        flag = R.GOLDEN_CASES[case]["p_apply_extra_tensors"][0]
        ref_o, ref_e = np.concatenate([r["out"] for r in recs]), np.concatenate([r["extra_out"] for r in recs])
        s_o, s_e = element_scales(pts, ids, t64), element_scales(extra, ids, t64)
        emu, ref, got = ratio(o32, o64, s_o), ratio(ref_o, o64, s_o), ratio(o32, ref_o, s_o)
        if flag:
            emu, ref, got = max(emu, ratio(e32, e64, s_e)), max(ref, ratio(ref_e, e64, s_e)), max(got, ratio(e32, ref_e, s_e))
        else:
            assert np.array_equal(ref_e, extra)
        rows[case] = (emu, ref, got)
    return rows


@pytest.fixture(scope="module")
def table(golden):
    return affine_table(golden)


def bound_of(emu):
    """8 x the case's own emulation, with a floor of one fp32 rounding of the element's scale under it: a case whose fp32 run
    happens to round nowhere (emulation 0) still leaves the reference its last bit."""
    return FACTOR * max(emu, FLOOR)


def test_affine_steps_per_element_against_the_reference(table):
    for case, (emu, ref, got) in table.items():
        bound = bound_of(emu)
        print(f"{case:16s} emulation {emu:.2e}  reference {ref:.2e}  restatement vs reference {got:.2e}  bound {bound:.2e}")
        assert ref <= bound and got <= bound, (case, emu, ref, got, bound)


def test_exact_steps_are_exact(table):
    """A mirror multiplies by +-1: nothing rounds, in either run."""
    assert table["mirror"] == (0.0, 0.0, 0.0)


def test_noise_is_the_clipped_scaled_sum(golden):
    cfg = R.GOLDEN_CASES["noise"]
    for r in batch_of(golden, "noise")[3]:
        y, e = R.add_noise(r["pts"], r["randn"].reshape(-1, 3), cfg["p_stddev"], cfg["p_clip"])
        assert np.array_equal(y, r["out"]) and np.array_equal(r["extra_out"], r["extra"])
        assert float(np.abs(e).max()) == float(F(cfg["p_clip"])) and (np.abs(e) < F(cfg["p_clip"])).any()   # the clip was reached


def removed(golden, case, **fault):
    cfg = R.GOLDEN_CASES[case]
    pts, ids, extra, recs = batch_of(golden, case)
    kind, consts, prob, _, _ = R.spec_of(cfg)
    draws = draws_of(kind, consts, recs)
    st = R.stats(pts, ids, len(recs))[1]
    if kind == "drop":   # the recorded uniform numbers stand where the hashed ones would
        mask = (np.concatenate([r["rand"] for r in recs]) > F(consts[0])).astype(np.uint8)
    else:
        mask = R.keep_mask(kind, consts, prob, pts, ids, len(recs), draws, st, **fault)
    sel, n_out, counts, _ = R.compact(mask, ids, len(recs))
    return R.gather(pts, sel)[:n_out], R.gather(extra, sel)[:n_out], counts, recs


@pytest.mark.parametrize("case", ["drop_remove", "crop_box", "crop_pts"])
def test_removing_steps_keep_exactly_the_reference_rows(golden, case):
    got, got_extra, counts, recs = removed(golden, case)
    assert counts.tolist() == [len(r["out"]) for r in recs] and 0 < counts.min() and counts.sum() < sum(R.GOLDEN_SIZES)
    assert np.array_equal(got, np.concatenate([r["out"] for r in recs]))
    assert np.array_equal(got_extra, np.concatenate([r["extra_out"] for r in recs]))


def test_crop_pts_count_is_the_reference_count(golden):
    recs = batch_of(golden, "crop_pts")[3]
    assert [len(r["out"]) for r in recs] == [min(60, int(n * 0.8)) for n in R.GOLDEN_SIZES] == [60, 60]
    assert R.crop_pts_count(70, [0, 0.8]) == 56 and R.crop_pts_count(70, [60, 1.0]) == 60 and R.crop_pts_count(10, [60, 1.0]) == 10


def test_statistics_are_torch_statistics(golden):
    import torch
    pts, ids, _, recs = batch_of(golden, "stdnorm")
    counts, st = R.stats(pts, ids, len(recs))
    for b, r in enumerate(recs):
        p = torch.from_numpy(r["pts"]).double()
        want = torch.cat((p.amin(0), p.amax(0), p.mean(0), p.std(0))).numpy()
        assert counts[b] == len(r["pts"]) and np.array_equal(st[b, 0:6], want[0:6].astype(F))
        assert np.abs(st[b, 6:12] - want[6:12]).max() <= 1.5 * np.spacing(np.abs(want[6:12]).astype(F)).max()
    # chunks: an element longer than two chunks, the same bits whatever stands behind the count
    rng = np.random.default_rng(3)
    big = rng.standard_normal((2 * R.CHUNK + 37, 3)).astype(F)
    ids = np.zeros(len(big), dtype=np.int32)
    a = R.stats(big, ids, 1)[1]
    b = R.stats(np.concatenate((big, np.full((5, 3), np.nan, dtype=F))), np.concatenate((ids, ids[:5])), 1, n_valid=len(big))[1]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.allclose(a[0, 9:12], big.astype(np.float64).std(0, ddof=1), rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------ planted faults
def test_planted_population_variance_is_caught(golden, table):
    bound = bound_of(table["stdnorm"][0])
    pts, ids, _, recs = batch_of(golden, "stdnorm")
    t64, o64, _ = run_affine(golden, "stdnorm", np.float64)
    _, bad, _ = run_affine(golden, "stdnorm", F, unbiased=False)
    ref = np.concatenate([r["out"] for r in recs])
    whole = np.linalg.norm(bad.astype(np.float64) - ref) / np.linalg.norm(ref)
    assert whole < 1e-2                                             # what a loose whole-tensor norm would wave through
    assert ratio(bad, ref, element_scales(pts, ids, t64)) > 100 * bound


def test_planted_gate_per_batch_is_caught():
    draws = np.zeros((2, R.DRAWS), dtype=F)
    draws[:, 0], draws[:, 1] = (0.2, 0.9), (0.3, 0.6)
    kind, consts, _, _, _ = R.spec_of({"name": "RotationAug", "p_axis": 2})
    good = R.affine_step(kind, consts, 0.5, draws, R.identity(2))
    bad = R.affine_step(kind, consts, 0.5, draws, R.identity(2), per_batch_gate=True)
    assert np.array_equal(good[1], R.identity(2)[1]) and not np.array_equal(good[0], R.identity(2)[0])   # element 1's gate is closed
    assert np.array_equal(bad[0], good[0]) and not np.array_equal(bad[1], good[1])
    # at the gate itself: u == p applies (`<=`)
    draws[:, 0] = (0.5, np.nextafter(F(0.5), F(1)))
    edge = R.affine_step(kind, consts, 0.5, draws, R.identity(2))
    assert not np.array_equal(edge[0], R.identity(2)[0]) and np.array_equal(edge[1], R.identity(2)[1])


def box_with_points_on_its_faces():
    """A cloud whose AABB is the drawn box (size draw 1 -> the box is the whole extent): the extreme points lie ON the faces."""
    rng = np.random.default_rng(5)
    pts = rng.random((80, 3)).astype(F)
    ids = np.zeros(80, dtype=np.int32)
    draws = np.zeros((1, R.DRAWS), dtype=F)
    draws[0, 1:4] = 0.999
    kind, consts, prob, _, _ = R.spec_of({"name": "CropBoxAug", "p_min_crop_size": 0.5, "p_max_crop_size": 3.0})
    return kind, consts, prob, pts, ids, draws, R.stats(pts, ids, 1)[1]


def test_planted_strict_box_face_is_caught():
    kind, consts, prob, pts, ids, draws, st = box_with_points_on_its_faces()
    good = R.keep_mask(kind, consts, prob, pts, ids, 1, draws, st)
    bad = R.keep_mask(kind, consts, prob, pts, ids, 1, draws, st, strict_upper=True)
    assert good.all()                                               # both faces belong to the box
    assert 1 <= (good != bad).sum() <= 3 and not bad[pts.argmax(0)].any()


def lattice_cloud(n=125):
    """Integer lattice points (as tests/knn_edges_reference.py builds its ties): many equal distances to any anchor."""
    g = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(F)
    return np.ascontiguousarray(g[np.random.default_rng(9).permutation(n)])


def test_planted_tie_order_is_caught():
    pts, ids = lattice_cloud(), np.zeros(125, dtype=np.int32)
    draws = np.zeros((1, R.DRAWS), dtype=F)
    draws[0, 1] = 0.5
    kind, consts, prob, _, _ = R.spec_of({"name": "CropPtsAug", "p_max_pts": 40, "p_crop_ratio": 1.0})
    good = R.keep_mask(kind, consts, prob, pts, ids, 1, draws)
    bad = R.keep_mask(kind, consts, prob, pts, ids, 1, draws, ties_to_highest=True)
    assert good.sum() == bad.sum() == 40 and not np.array_equal(good, bad)
    d = R.dist2(pts, pts[62])
    thr = np.sort(d)[39]
    at = np.flatnonzero(d == thr)
    assert len(at) > 1 and good[at].sum() < len(at)                 # the threshold IS tied, and cut
    assert good[at].tolist() == sorted(good[at].tolist(), reverse=True)   # the kept ties are the lowest rows


def test_scene_by_scene_keeps_every_tensor_on_its_own_rows():
    """Rotation on both extras, a crop on the first only, another rotation on both: the second extra keeps ALL its rows and is
    rotated twice, row by row, with its own scene's angles (CropPtsAug.py:67-69 leaves an unflagged tensor at its length)."""
    rng = np.random.default_rng(11)
    pts = rng.random((90, 3)).astype(F)
    ids = np.repeat(np.arange(3, dtype=np.int32), 30)
    e0, e1 = rng.standard_normal((90, 3)).astype(F), rng.standard_normal((90, 3)).astype(F)
    cfgs = [{"name": "RotationAug", "p_axis": 2, "p_apply_extra_tensors": [True, True]},
            {"name": "CropPtsAug", "p_crop_ratio": 0.5, "p_apply_extra_tensors": [True, False]},
            {"name": "RotationAug", "p_axis": 0, "p_apply_extra_tensors": [True, True]}]
    draws = rng.random((len(cfgs), 3, R.DRAWS)).astype(F)
    out = R.scene_by_scene(cfgs, pts, ids, 3, draws, seed_eff=7, extras=[e0, e1])
    assert [len(p) for p in out["pts"]] == [15, 15, 15] and [len(t) for t in out["extras"][0]] == [15] * 3 and [len(t) for t in out["extras"][1]] == [30] * 3
    for b in range(3):
        za = R.axis_rotation(2, np.float64(draws[0, b, 1]) * (2 * np.pi), np.float64)
        xa = R.axis_rotation(0, np.float64(draws[2, b, 1]) * (2 * np.pi), np.float64)
        assert np.allclose(out["extras"][1][b], e1[ids == b].astype(np.float64) @ za @ xa, atol=1e-5)
        assert np.allclose(out["extras"][0][b], (e0.astype(np.float64) @ za @ xa)[out["orig"][b]], atol=1e-5)
        assert np.allclose(out["pts"][b], (pts.astype(np.float64) @ za @ xa)[out["orig"][b]], atol=1e-5) and (ids[out["orig"][b]] == b).all()
    with pytest.raises(ValueError, match="rows, the points' mask"):           # a later mask on the tensor that was left out
        R.scene_by_scene(cfgs + [{"name": "CropPtsAug", "p_crop_ratio": 0.5, "p_apply_extra_tensors": [False, True]}], pts, ids, 3,
                         rng.random((4, 3, R.DRAWS)).astype(F), extras=[e0, e1])


if __name__ == "__main__":
    with np.load(os.path.join(GOLDEN, "augment_steps.npz")) as z:
        g = {k: z[k] for k in z.files}
    t = affine_table(g)
    print(f"bound per case = {FACTOR} x max(emulation, 2^-24)")
    for case, (emu, ref, got) in t.items():
        print(f"{case:16s} emulation {emu:.2e}  reference {ref:.2e}  restatement vs reference {got:.2e}")
