"""GPU: the entry points of include/se3conv_augment.h and `se3conv3d_amd.augment` against the numpy restatement
(tests/augment_reference.py), at shapes chosen for the kernels' edges (tests/augment_cases.py): elements of 0 (in the middle),
1, 63, 64, 65, 257 and 2 * SE3_AUG_CHUNK + 37 rows in one batch, trimmed and inside larger buffers whose absent rows are filled
both hostile ways of tests/padded_cases.py.

What is exact is compared bit for bit: statistics, every table entry that is not the rounding of a fp64 cosine or sine, the
rows `se3_aug_apply` writes from the device's own table, masks, indices and counts.  The rotation entries are held to one fp32
rounding (the device's fp64 cos / sin may differ from numpy's in the last fp64 bit).  The Gaussian numbers are held per element
against the fp64 restatement at 8 x what the restatement run in fp32 reaches (the ratio is printed).  The elastic step is not
implemented; it has no test here."""
import numpy as np
import pytest
import torch

import augment_cases as A
import augment_configs as CFG
import augment_reference as R
from augment_cases import DEV, NB, VARIANTS, same_bits, t

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def aug(built_library):
    from se3conv3d_amd import augment
    return augment


@pytest.fixture(scope="module")
def base():
    """The batch and its restated statistics, computed once."""
    pts, ids = A.cloud(1)
    tab = A.random_table(2)
    return {"pts": pts, "ids": ids, "table": tab, "plain": R.stats(pts, ids, NB), "under": R.stats(pts, ids, NB, tab)}


# -------------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("variant", VARIANTS)
def test_stats_bit_for_bit(aug, base, variant):
    p, b, w, _ = A.on_device(base["pts"], base["ids"], variant)
    for table, key in ((None, "plain"), (t(base["table"]), "under")):
        counts, st = aug.aug_stats(p, b, NB, table, w)
        again = aug.aug_stats(p, b, NB, table, w)[1]
        want_counts, want = base[key]
        assert counts.cpu().tolist() == want_counts.tolist() == list(A.SIZES)
        assert same_bits(st, want), (variant, key, np.abs(st.cpu().numpy() - want).max())
        assert same_bits(again, st.cpu().numpy())
    assert np.isnan(want[0, 9:12]).all() and not want[3].any()          # one row: torch.std's NaN; the empty element: zeros


# --------------------------------------------------------------------------------------------------------- the affine table
STEPS = [
    ("rot_z", {"name": "RotationAug", "p_axis": 2}), ("rot_x", {"name": "RotationAug", "p_axis": 0, "p_min_angle": -0.13, "p_max_angle": 0.13}),
    ("rot_y_fixed", {"name": "RotationAug", "p_axis": 1, "p_angle_values": [0.0, 2.5]}), ("rot3d", {"name": "RotationAug3D"}),
    ("rot3d_axis", {"name": "RotationAug3D", "p_axis": 0}), ("center", {"name": "CenterAug", "p_axes": [True, False, True]}),
    ("linear", {"name": "LinearAug"}), ("linear_single", {"name": "LinearAug", "p_channel_independent": True}),
    ("linear_fixed", {"name": "LinearAug", "p_a_values": [[0.5, 2.0, 1.5]], "p_b_values": [[0.1, -0.2, 0.3]]}),
    ("mirror", {"name": "MirrorAug", "p_axes": [True, True, True]}), ("translation", {"name": "TranslationAug", "p_max_aabb_ratio": [0.5, 0.25, 0.0]}),
    ("stdnorm", {"name": "STDDevNormAug", "p_new_std": 0.7}),
]


@pytest.mark.parametrize("name,cfg", STEPS, ids=[s[0] for s in STEPS])
def test_affine_step_against_the_restatement(aug, base, name, cfg):
    kind, consts, _, _, _ = R.spec_of(cfg, 1 if name == "rot_y_fixed" else 0)      # (the second angle of its table)
    prob = 1.0 if kind in ("center", "stdnorm") else 0.6
    draws = A.draws(31)
    draws[:, 0] = [0.1, 0.9, 0.6, 0.2, 0.61, 0.0, 0.3]                  # elements 1 and 4 keep their tables; 0.6 <= 0.6 applies
    rotation = kind in ("rot_axis", "rot_3d")
    start = R.identity(NB) if rotation else base["table"]               # from the identity the table IS the rotation's entries
    counts, st = base["plain"] if rotation else base["under"]
    want = R.affine_step(kind, consts, prob, draws, start, counts, st)
    got = t(start.copy())
    needs = kind in R.NEEDS_STATS
    aug.aug_affine_step(kind, consts, prob, t(draws), got, t(counts) if needs else None, t(st) if needs else None)
    got = got.cpu().numpy()
    closed = draws[:, 0] > F(prob)
    assert same_bits(got[closed], start[closed]) and (closed.sum() == (0 if prob == 1.0 else 2))
    if rotation:
        assert np.abs(got.astype(np.float64) - want).max() <= np.spacing(F(1.0)) / 2 + 1e-12, name   # one rounding of |entry| <= 1
        assert not np.array_equal(got[0], start[0])
    else:
        assert same_bits(got, want), (name, np.abs(got - want).max())
        if kind == "stdnorm":
            assert np.isnan(got[0]).any() and same_bits(got[3], start[3])     # one row: NaN as torch; empty: kept


# ------------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("variant", VARIANTS)
def test_apply_bit_for_bit_from_the_devices_table(aug, base, variant):
    p, b, w, rows = A.on_device(base["pts"], base["ids"], variant)
    table = t(R.identity(NB))
    for cfg, seed in (({"name": "RotationAug3D"}, 41), ({"name": "RotationAug", "p_axis": 0}, 42), ({"name": "LinearAug"}, 43)):
        kind, consts, prob, _, _ = R.spec_of(cfg)
        aug.aug_affine_step(kind, consts, prob, t(A.draws(seed)), table)
    tab = table.cpu().numpy()                                            # the DEVICE's table: from here on everything is exact
    n = len(base["pts"])
    for linear_only in (False, True):
        y = aug.aug_apply(p, b, NB, table, linear_only, n_valid=w)
        assert same_bits(y, A.host_padded(R.apply(base["pts"], base["ids"], NB, tab, linear_only), rows)), (variant, linear_only)
    rng = np.random.default_rng(5)
    ones = (rng.random(rows) > 0.3).astype(np.uint8)
    y = aug.aug_apply(p, b, NB, None, ones_mask=t(ones), n_valid=w)
    want = A.host_padded(R.apply(base["pts"], base["ids"], NB, None, ones_mask=ones[:n]), rows)
    assert same_bits(y, want) and (want[:n][ones[:n] == 0] == 1).all()
    assert same_bits(aug.aug_apply(p, b, NB, None, n_valid=w), A.host_padded(base["pts"], rows))      # the identity copies


# ------------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("variant", VARIANTS)
def test_noise_values_gate_and_clip(aug, variant):
    ids = A.ids_of()
    zeros = np.zeros((A.N, 3), dtype=F)
    p, b, w, rows = A.on_device(zeros, ids, variant)
    draws = A.draws(51)
    draws[:, 0] = [0.1, 0.2, 0.9, 0.3, 0.4, 0.95, 0.5]                   # elements 2 and 5: no noise
    seed, word, step = 123456789, 4000000000, 6
    seed_t = torch.tensor([word - (1 << 32)], dtype=torch.int32, device=DEV)
    seed_eff = (seed + word) & 0xFFFFFFFF
    open_rows = np.isin(ids, np.flatnonzero(draws[:, 0] <= F(0.8)))
    # sigma 1, no clip, x = 0: y IS the Gaussian number of the row's words
    y = aug.aug_apply(p, b, NB, None, noise=(t(draws), 0.8, 1.0, None), seed=seed, seed_tensor=seed_t, step=step, n_valid=w).cpu().numpy()
    z64, z32 = R.gaussian(seed_eff, step, np.arange(A.N), np.float64), R.gaussian(seed_eff, step, np.arange(A.N), F)
    assert not y[A.N:].any() and not y[:A.N][~open_rows].any() and open_rows.sum() == A.N - 64 - 257
    u1 = R.uniform(R.word(seed_eff, step, np.arange(A.N, dtype=np.uint32)[:, None], 2 * np.arange(3, dtype=np.uint32)[None])).astype(np.float64)
    scale = np.sqrt(-2.0 * np.log(1.0 - u1)) + 1e-30                     # the radius: cos only turns it
    emulated = float((np.abs(z32 - z64) / scale).max())
    ratio = float((np.abs(y[:A.N] - z64) / scale)[open_rows].max())
    print(f"gaussian {variant}: library {ratio:.2e}, fp32 restatement {emulated:.2e}, bound {8 * emulated:.2e}")
    assert ratio <= 8 * emulated, (ratio, emulated)
    assert abs(float(y[:A.N][open_rows].mean())) < 0.1 and 0.9 < float(y[:A.N][open_rows].std()) < 1.1
    # another seed word, another step: other numbers (a wrong key would show here or above)
    other = aug.aug_apply(p, b, NB, None, noise=(t(draws), 0.8, 1.0, None), seed=seed, seed_tensor=seed_t, step=step + 1, n_valid=w).cpu().numpy()
    assert float(np.abs(other[:A.N] - R.gaussian(seed_eff, step + 1, np.arange(A.N), np.float64))[open_rows].max()) < 1e-5
    # NoiseAug's own numbers: sigma 0.005 clipped at 0.008, the clip reached and never passed
    e = aug.aug_apply(p, b, NB, None, noise=(t(draws), 0.8, 0.005, 0.008), seed=seed, seed_tensor=seed_t, step=step, n_valid=w).cpu().numpy()
    assert float(np.abs(e).max()) == float(F(0.008)) and (np.abs(e[:A.N][open_rows]) < F(0.008)).mean() > 0.8
    want = R.add_noise(zeros, z64.astype(F), 0.005, 0.008)[0]
    assert float(np.abs(e[:A.N] - want)[open_rows].max()) <= 8 * emulated * 0.005 * float(scale.max())


def test_every_noise_word_bit_for_bit(aug):
    """The six uniform numbers NoiseAug reads per row, pinned exactly: `U > p` is false at p = U and true at the fp32 number
    below it, so the two masks of the drop kind with word index j fix the device's U(w(step, row, j)) to the restatement's
    bits.  Rows on both sides of a wavefront, a seed whose sum with the device word wraps, two steps."""
    n, seed, word = 70, 0xF0000001, 0x20000005
    p, b = t(np.zeros((n, 3), dtype=F)), t(np.zeros(n, dtype=np.int32))
    seed_t = torch.tensor([word], dtype=torch.int32, device=DEV)
    seed_eff = (seed + word) & 0xFFFFFFFF
    draws = t(np.zeros((1, R.DRAWS), dtype=F))
    wrong = torch.zeros((), dtype=torch.int64, device=DEV)
    for step in (0, 9):
        for j in range(6):
            u = R.uniform(R.word(seed_eff, step, np.arange(n, dtype=np.uint32), j))
            assert len(np.unique(u)) == n and u.min() > 0
            for r in range(n):                                           # every row's own value as a threshold, and the number below it
                for thr, keep in ((u[r], u > u[r]), (np.nextafter(u[r], F(0)), u >= u[r])):
                    mask = aug.aug_keep_mask("drop", [float(thr), j], 1.0, p, b, 1, draws, None, seed, seed_t, step)
                    wrong += (mask != t(keep.astype(np.uint8))).sum()
    assert int(wrong) == 0


# ------------------------------------------------------------------------------------------------------ masks and compaction
def check_mask_and_compaction(aug, pts, ids, nb, variant, kind, consts, prob, draws, seed_eff=0, step=0, idx_in=None):
    p, b, w, rows = A.on_device(pts, ids, variant)
    n = len(pts)
    st = R.stats(pts, ids, nb)[1] if kind == "crop_box" else None
    want = A.host_padded(R.keep_mask(kind, consts, prob, pts, ids, nb, draws, st, seed_eff, step), rows)
    got = aug.aug_keep_mask(kind, consts, prob, p, b, nb, t(draws), None if st is None else t(st), seed_eff, None, step, w)
    assert np.array_equal(got.cpu().numpy(), want), (kind, variant, int((got.cpu().numpy() != want).sum()))
    hostile = got.clone()
    hostile[n:] = 1                                                      # the compaction itself must not read an absent row's byte
    idx, n_out, counts, orig = aug.aug_compact(hostile if w is not None else got, b, nb, w, None if idx_in is None else t(A.host_padded(idx_in, rows)))
    w_idx, w_n, w_counts, w_orig = R.compact(want[:n], ids, nb, None, idx_in)
    assert np.array_equal(idx.cpu().numpy(), np.concatenate((w_idx, np.full(rows - n, -1, dtype=np.int32))))
    assert n_out.cpu().tolist() == [w_n] and counts.cpu().tolist() == w_counts.tolist()
    if idx_in is not None:
        assert np.array_equal(orig.cpu().numpy(), np.concatenate((w_orig, np.full(rows - n, -1, dtype=np.int32))))
    return want[:n]


@pytest.mark.parametrize("variant", VARIANTS)
def test_drop_masks(aug, base, variant):
    draws = A.draws(61)
    draws[:, 0] = [0.1, 0.2, 0.3, 0.4, 0.9, 0.5, 0.6]                    # element 4 is left alone
    kept = {}
    for drop in (0.3, 0.0, 1.0):
        kind, consts, _, _, _ = R.spec_of({"name": "DropAug", "p_drop_prob": drop})
        kept[drop] = check_mask_and_compaction(aug, base["pts"], base["ids"], NB, variant, kind, consts, 0.8, draws, 0xDEADBEEF, 3,
                                               np.arange(A.N, dtype=np.int32)[::-1].copy() if drop == 0.3 else None)
    el4 = base["ids"] == 4
    assert kept[0.3][el4].all() and 0.6 < kept[0.3][~el4].mean() < 0.8
    assert kept[0.0].sum() >= A.N - 1 and kept[1.0].sum() == el4.sum()   # u > 0 keeps all but a zero word; u > 1 keeps nothing


@pytest.mark.parametrize("variant", VARIANTS)
def test_crop_box_masks(aug, base, variant):
    kind, consts, prob, _, _ = R.spec_of({"name": "CropBoxAug", "p_min_crop_size": 0.5, "p_max_crop_size": 1.0})
    kept = check_mask_and_compaction(aug, base["pts"], base["ids"], NB, variant, kind, consts, prob, A.draws(62))
    assert 0 < kept.sum() < A.N
    # boxes whose faces pass through points: lattice points (every sum below is exact), first the bounding box itself -- both
    # faces belong to the box -- then a box of two cells from the lower corner, which cuts THROUGH planes of points
    pts, ids, nb = A.lattice_batch()
    for size, cells in ((9.0, None), (2.0, 3)):
        kind, consts, prob, _, _ = R.spec_of({"name": "CropBoxAug", "p_min_crop_size": size, "p_max_crop_size": size})
        draws = A.draws(63, nb=nb)
        draws[:, 4:7] = 0.0
        kept = check_mask_and_compaction(aug, pts, ids, nb, variant, kind, consts, prob, draws)
        assert kept.all() if cells is None else [int(kept[ids == b].sum()) for b in range(nb)] == [cells ** 3] * nb


@pytest.mark.parametrize("variant", VARIANTS)
def test_crop_pts_masks(aug, base, variant):
    for cfg in ({"name": "CropPtsAug", "p_max_pts": 100, "p_crop_ratio": 0.8}, {"name": "CropPtsAug", "p_crop_ratio": 0.37}):
        kind, consts, prob, _, _ = R.spec_of(cfg)
        kept = check_mask_and_compaction(aug, base["pts"], base["ids"], NB, variant, kind, consts, prob, A.draws(64))
        want = [R.crop_pts_count(n, consts) for n in A.SIZES]
        assert [int(kept[base["ids"] == b].sum()) for b in range(NB)] == [min(n, m) for n, m in zip(A.SIZES, want)]
    kind, consts, prob, _, _ = R.spec_of({"name": "CropPtsAug", "p_max_pts": 0, "p_crop_ratio": 1.0})      # keeps everything
    assert check_mask_and_compaction(aug, base["pts"], base["ids"], NB, variant, kind, consts, prob, A.draws(65)).all()


@pytest.mark.parametrize("variant", VARIANTS)
def test_crop_pts_with_planted_distance_ties(aug, variant):
    pts, ids, nb = A.lattice_batch()
    kind, consts, prob, _, _ = R.spec_of({"name": "CropPtsAug", "p_max_pts": 50, "p_crop_ratio": 0.9})
    draws = A.draws(66, nb=nb)
    kept = check_mask_and_compaction(aug, pts, ids, nb, variant, kind, consts, prob, draws)
    assert [int(kept[ids == b].sum()) for b in range(nb)] == [50, 50, 50]
    other = R.keep_mask(kind, consts, prob, pts, ids, nb, draws, ties_to_highest=True)
    assert not np.array_equal(kept, other)                                # the thresholds ARE tied: the other order differs


# ---------------------------------------------------------------------------------------------------------------- pipeline
def extras_for(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3)).astype(F)
    return [nrm, rng.random((n, 3)).astype(F), rng.integers(0, 20, n).astype(np.int64), np.arange(n, dtype=np.int32)]


def both_runs(cfgs, pts, ids, nb, draws, seed, extras):
    """The scene-by-scene statement in fp32 and, keeping the same rows, in fp64."""
    s32 = R.scene_by_scene(cfgs, pts, ids, nb, draws, seed, extras)
    return s32, R.scene_by_scene(cfgs, pts, ids, nb, draws, seed, extras, dtype=np.float64, masks=s32["masks"])


def cat(parts):
    return np.concatenate(parts)


def row_ratio(a, b, peak):
    """max over rows of |a - b|_inf / the row's scale; rows of scale 0 must agree exactly."""
    d = np.abs(np.asarray(a, dtype=np.float64) - b).max(1)
    live = peak > 0
    assert not d[~live].any()
    return float((d[live] / peak[live]).max()) if live.any() else 0.0


def check_against_the_scenes(res, s32, s64, cfgs, n_in, rows, what):
    """The library's batch against the scenes run one by one.  Surviving rows, their order, ids and original rows: exact.
    Values: per row, |library - fp64 scenes|_inf / the largest norm the row reached (`peak`) within 8 x what the fp32 scenes
    reach, plus one fp32 rounding (2^-24 of the row's scale) per rotation step: the device's fp64 cos / sin may differ from
    numpy's in the last fp64 bit, which can move the fp32 rounding of an entry of magnitude <= 1."""
    rotations = sum(c["name"] in ("RotationAug", "RotationAug3D") for c in cfgs)
    want64, peak = cat(s64["pts"]), cat(s64["peak"])
    n = len(want64)
    removed = bool(s32["masks"])
    if removed:
        assert res.n_valid_.cpu().tolist() == [n]
        assert np.array_equal(res.idx_.cpu().numpy(), np.concatenate((cat(s32["orig"]), np.full(rows - n, -1, dtype=np.int32))))
        assert np.array_equal(res.batch_ids_[:n].cpu().numpy(), np.repeat(np.arange(len(s32["pts"]), dtype=np.int32), [len(p) for p in s32["pts"]]))
    else:
        assert res.idx_ is None and n == n_in
    got = res.pts_.cpu().numpy()
    assert got.shape == (rows, 3) and not got[n:].any()
    emulated, ratio = row_ratio(cat(s32["pts"]), want64, peak), row_ratio(got[:n], want64, peak)
    for i, g in enumerate(res.extra_tensors_):
        g, e64, e32 = g.cpu().numpy(), cat(s64["extras"][i]), cat(s32["extras"][i])
        m = len(e64)
        assert not g[m:].any()                                           # behind ITS rows: zeros
        word = res.extra_n_valid_[i]
        assert m == (n_in if word is None else int(word))                # the word of ITS rows
        if s64["extra_peak"][i][0] is not None and any(c["name"] not in ("DropAug", "CropBoxAug", "CropPtsAug") and
                                                       (list(c.get("p_apply_extra_tensors", [])) + [False] * 8)[i] for c in cfgs):
            pk = cat(s64["extra_peak"][i])
            emulated, ratio = max(emulated, row_ratio(e32, e64, pk)), max(ratio, row_ratio(g[:m], e64, pk))
        else:
            assert np.array_equal(g[:m], e32)                            # only moved, never computed on
    bound = 8 * emulated + rotations * 2.0 ** -24
    print(f"{what}: library {ratio:.2e}, fp32 scenes {emulated:.2e}, bound {bound:.2e} ({rotations} rotation steps)")
    assert ratio <= bound, (what, ratio, bound)
    return n


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["DFAUST", "MN40", "SCANNET"])
def test_pipeline_against_the_scenes_one_by_one(aug, base, name, variant):
    cfgs = getattr(CFG, name)
    extras = extras_for(A.N, 71)[:len(cfgs[0]["p_apply_extra_tensors"])]
    draws, seed = A.draws(72, len(cfgs)), 987654321
    s32, s64 = both_runs(cfgs, base["pts"], base["ids"], NB, draws, seed, extras)
    p, b, w, rows = A.on_device(base["pts"], base["ids"], variant)
    pipe = aug.AugPipeline()
    pipe.create_pipeline(cfgs)
    res = pipe.augment_batch(p, b, NB, [t(A.host_padded(e, rows)) for e in extras], n_valid=w, seed=seed, draws=t(draws))
    n = check_against_the_scenes(res, s32, s64, cfgs, A.N, rows, f"{name} {variant}")
    assert (0 < n < A.N) if name == "SCANNET" else (res.n_valid_ is w)
    if name == "DFAUST":                                                 # the table of the last write: CenterAug's, -mean per element
        tab = res.affine_.cpu().numpy()
        assert np.array_equal(tab[:, 9:12], -base["plain"][1][:, 6:9]) and np.array_equal(tab[:, :9], R.identity(NB)[:, :9])


OWN_ROWS = [
    {"name": "RotationAug", "p_axis": 2, "p_apply_extra_tensors": [True, True, False]},
    {"name": "DropAug", "p_drop_prob": 0.3, "p_keep_zeros": False, "p_apply_extra_tensors": [True, False, True]},
    {"name": "MirrorAug", "p_axes": [True, True, True], "p_apply_extra_tensors": [True, True, False]},
    {"name": "CropPtsAug", "p_crop_ratio": 0.7, "p_apply_extra_tensors": [True, False, False]},
    {"name": "NoiseAug", "p_stddev": 0.05, "p_clip": 0.08, "p_apply_extra_tensors": [True, False, False]},   # NoiseAug.py:58-61
    {"name": "RotationAug", "p_axis": 0, "p_apply_extra_tensors": [True, True, False]},
    {"name": "LinearAug", "p_apply_extra_tensors": [False, True, False]},
    {"name": "CenterAug", "p_apply_extra_tensors": [False, False, False]},
]


@pytest.mark.parametrize("variant", VARIANTS)
def test_extras_keep_their_own_rows(aug, base, variant):
    """Three extra tensors: one follows the points through both removing steps, one through NEITHER (and still takes every
    later rotation, mirror and linear step, on all its rows, with its own scene's parameters), one through the first only."""
    extras = extras_for(A.N, 73)[:2] + [np.arange(A.N, dtype=np.int64)]
    draws, seed = A.draws(74, len(OWN_ROWS)), 1357
    s32, s64 = both_runs(OWN_ROWS, base["pts"], base["ids"], NB, draws, seed, extras)
    p, b, w, rows = A.on_device(base["pts"], base["ids"], variant)
    pipe = aug.AugPipeline()
    pipe.create_pipeline(OWN_ROWS)
    res = pipe.augment_batch(p, b, NB, [t(A.host_padded(e, rows)) for e in extras], n_valid=w, seed=seed, draws=t(draws))
    n = check_against_the_scenes(res, s32, s64, OWN_ROWS, A.N, rows, f"own rows {variant}")
    lens = [len(cat(s32["extras"][i])) for i in range(3)]
    assert lens[0] == n < lens[2] < lens[1] == A.N and res.cropped_ == [True, False, True]
    assert res.extra_n_valid_[0] is res.n_valid_ and res.extra_n_valid_[1] is w and int(res.extra_n_valid_[2]) == lens[2]
    with pytest.raises(ValueError, match="no longer the points' rows"):   # a mask on a tensor that was left out before
        pipe.create_pipeline(OWN_ROWS + [{"name": "CropPtsAug", "p_crop_ratio": 0.5, "p_apply_extra_tensors": [False, True, False]}])
        pipe.augment_batch(p, b, NB, [t(A.host_padded(e, rows)) for e in extras], n_valid=w, seed=seed)


def test_single_cloud_signature(aug, base):
    pipe = aug.AugPipeline()
    pipe.create_pipeline([{"name": "CenterAug"}, {"name": "CropPtsAug", "p_crop_ratio": 0.5, "p_apply_extra_tensors": [True, False, False]},
                          {"name": "MirrorAug", "p_mirror_prob": -1.0, "p_axes": [True, False, False], "p_apply_extra_tensors": [False, False, True]}])
    x = t(base["pts"][:300])
    labels, other, normals = torch.arange(300, device=DEV), torch.arange(300, device=DEV), t(base["pts"][300:600])
    out, params, extras = pipe.augment(x, [labels, other, normals])
    assert out.shape == (150, 3) and params == [] and extras[0].shape == (150,) and extras[1] is other
    centre = base["pts"][:300].astype(np.float64).mean(0)
    want = (base["pts"][:300][extras[0].cpu().numpy()] - centre) * np.array([-1.0, 1.0, 1.0])
    assert float(np.abs(out.cpu().numpy() - want).max()) < 1e-5
    # the tensor the crop left alone keeps its 300 rows and is mirrored on every one of them
    assert same_bits(extras[2], base["pts"][300:600] * np.array([-1, 1, 1], dtype=F))


# --------------------------------------------------------------------------------------------------------------- hierarchy
def test_result_feeds_a_padded_hierarchy_and_a_convolution(aug, built_library):
    import se3conv3d_amd as amd
    from bounded_levels_cases import cloud

    PC = amd.pc
    pts, bid = cloud((700, 500, 600), 5)
    nb, rows = 3, 2000
    p, b = torch.full((rows, 3), float("nan"), device=DEV), torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    p[:1800], b[:1800] = pts.to(DEV), bid.to(DEV).int()
    w = torch.tensor([1800], dtype=torch.int32, device=DEV)
    pipe = aug.AugPipeline()
    pipe.create_pipeline([{"name": "RotationAug", "p_axis": 2}, {"name": "NoiseAug", "p_stddev": 0.001, "p_clip": 0.003},
                          {"name": "CropPtsAug", "p_crop_ratio": 0.8}])
    res = pipe.augment_batch(p, b, nb, n_valid=w, seed=5)
    cfg = {"pca": True, "n_frames": 2, "fixed_axis": False, "neigh_method": "knn", "neigh_kwargs": {"neigh_k": 16}}
    pc0 = PC.PointcloudRotEquiv(res.pts_, res.batch_ids_, cfg, p_n_valid=res.n_valid_, num_batches=nb)
    hier = PC.PointHierarchyRotEquiv(pc0, 1, "grid_avg", p_capacities="input", p_padded=True, grid_radii=[0.12])
    sizes = hier.level_sizes()
    assert sizes[0] == 560 + 400 + 480 and 0 < sizes[1] < sizes[0] and not hier.overflowed()
    torch.manual_seed(1)
    conv = amd.PNEConvLayerRotEquivFactory(9, 32, "mlp_gelu").create_conv_layer(32, 32).to(DEV)
    conv.norm_neigh_dist_.fill_(1.0 / 0.15), conv.norm_num_neighs_.fill_(1.0 / 14.0)
    nbh = PC.BQNeighborhood(pc0, pc0, 0.15, p_capacity=120000)
    x = torch.randn(rows * 2, 32, device=DEV)
    out = conv(p_pc_in=pc0, p_pc_out=pc0, p_in_features=x, p_neighborhood=nbh)
    assert out.shape == (rows * 2, 32) and bool(torch.isfinite(out[:sizes[0] * 2]).all()) and float(out[:sizes[0] * 2].abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------- capture
def test_whole_pipeline_replays_as_one_graph(aug):
    """`augment_batch` of the ScanNet list -- statistics, table steps, noise, point crop, compaction, row gathers -- captured
    ONCE and replayed on batches of another valid count with another seed word and new draws: each replay is the eager run
    bit for bit."""
    from test_gpu_graph_nodes import HIP_GRAPH_NODE_TYPE_MEMSET, node_types

    cfgs = CFG.SCANNET
    rows, seed = A.ROWS, 24680
    s_pts = torch.full((rows, 3), float("nan"), device=DEV)
    s_ids = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    s_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_seed = torch.zeros(1, dtype=torch.int32, device=DEV)
    s_draws = torch.zeros((len(cfgs), NB, R.DRAWS), device=DEV)
    s_extras = [torch.zeros((rows, 3), device=DEV), torch.zeros((rows, 3), device=DEV), torch.zeros(rows, dtype=torch.int64, device=DEV),
                torch.zeros(rows, dtype=torch.int32, device=DEV)]
    pipe = aug.AugPipeline()
    pipe.create_pipeline(cfgs)
    held = {}

    def load(sizes, seed_word, case_seed):
        pts, ids = A.cloud(case_seed, sizes)
        n = len(pts)
        s_pts.fill_(float("nan")), s_ids.fill_(-1)
        s_pts[:n], s_ids[:n] = t(pts), t(ids)
        s_word.fill_(n), s_seed.fill_(seed_word)
        s_draws.copy_(t(A.draws(case_seed + 1, len(cfgs))))
        for dst, src in zip(s_extras, extras_for(n, case_seed + 2)):
            dst.zero_()
            dst[:n] = t(src)

    def step():
        held["res"] = pipe.augment_batch(s_pts, s_ids, NB, s_extras, n_valid=s_word, seed=seed, seed_tensor=s_seed, draws=s_draws)

    def snapshot(res):
        return [x.clone() for x in (res.pts_, res.batch_ids_, res.n_valid_, res.idx_, res.affine_, *res.extra_tensors_)]

    load(A.SIZES, 1, 81)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    held.clear()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):    # fails if anything on the path reads back
        step()
    types = node_types(graph)
    assert len(types) > 25 and types.count(HIP_GRAPH_NODE_TYPE_MEMSET) == 0, types
    captured = held["res"]
    counts = []
    for sizes, seed_word, case_seed in ((A.SIZES, 1, 81), ((300, 0, 41, 200, 1, 90, 7), 77, 91), ((64, 64, 64, 64, 64, 64, 64), -5, 95)):
        load(sizes, seed_word, case_seed)
        graph.replay()
        torch.cuda.synchronize()
        replayed = snapshot(captured)
        step()                                                          # the eager run on the same buffers
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(replayed, snapshot(held["res"]))):
            assert A.same_bits(a, b.cpu().numpy()), (sizes, i)
        counts.append(int(replayed[2]))
        assert counts[-1] == sum(min(n, int(n * 0.8)) for n in sizes)
    assert len(set(counts)) == 3
