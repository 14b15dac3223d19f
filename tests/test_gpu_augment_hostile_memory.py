"""GPU: the device entry points of include/se3conv_augment.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_global_pool_hostile_memory.py: points, ids, tables, draws, every output and the workspaces (sized to
exactly the queries' values) come from an arena, so the absent rows hold the arena's fill (NaN points, id -1); no band byte
changes, the results are those of the numpy restatement whatever the workspace held, every output byte is a result, and the
entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import augment_cases as A
import augment_configs as CFG
import augment_reference as R
import hostile_memory
from augment_cases import DEV, NB, same_bits, t
from hostile_memory import in_arena
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32

# entry point (include/se3conv_augment.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_aug_stats": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
    "se3_aug_affine_step": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
    "se3_aug_apply": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
    "se3_aug_keep_mask": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
    "se3_aug_compact": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
}


@pytest.fixture(scope="module")
def aug(built_library):
    from se3conv3d_amd import augment
    return augment


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_augment.h", _lib.AUGMENT_SIGNATURES)


def guarded(request, workspace_fill):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=True)


across_fills = hostile_memory.AcrossFills()


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_entry_points_one_by_one(aug, request, workspace_fill):
    pts, ids = A.cloud(3)
    tab, draws = A.random_table(4), A.draws(5)
    draws[:, 0] = [0.1, 0.9, 0.2, 0.3, 0.4, 0.5, 0.6]
    n, rows, prob = A.N, A.ROWS, 0.8
    with guarded(request, workspace_fill) as arena:
        p, b = in_arena(arena, t(pts), rows), in_arena(arena, t(ids), rows)
        assert torch.isnan(p[n:]).all() and bool((b[n:] == -1).all())
        w, table, d = arena.place(torch.tensor([n], dtype=torch.int32)), arena.place(t(tab)), arena.place(t(draws))
        # statistics
        counts, st = aug.aug_stats(p, b, NB, table, w)
        w_counts, w_st = R.stats(pts, ids, NB, tab)
        assert counts.cpu().tolist() == w_counts.tolist() and same_bits(st, w_st)
        # one table step that needs them, one that does not
        for cfg in ({"name": "TranslationAug", "p_max_aabb_ratio": 0.5}, {"name": "MirrorAug"}):
            kind, consts, _, _, _ = R.spec_of(cfg)
            needs = kind in R.NEEDS_STATS
            want = R.affine_step(kind, consts, prob, draws, tab, w_counts, w_st)
            aug.aug_affine_step(kind, consts, prob, d, table, counts if needs else None, st if needs else None)
            assert same_bits(table, want)
            tab = want
        # apply, with noise and the rows set to one
        ones = arena.alloc((rows,), torch.uint8)
        ones[:n] = t((np.arange(n) % 5 != 0).astype(np.uint8))
        y = aug.aug_apply(p, b, NB, table, noise=(d, prob, 0.005, 0.02), seed=11, step=2, ones_mask=ones, n_valid=w)
        want = R.apply(pts, ids, NB, tab, noise=(draws, prob, 0.005, 0.02), seed_eff=11, step=2, ones_mask=(np.arange(n) % 5 != 0))
        assert not bool(y[n:].view(torch.int32).any()) and float(np.abs(y[:n].cpu().numpy() - want).max()) < 2e-6
        plain = aug.aug_apply(p, b, NB, table, n_valid=w)
        assert same_bits(plain, A.host_padded(R.apply(pts, ids, NB, tab), rows))
        # masks: the three kinds, on the points as they are
        _, box = aug.aug_stats(p, b, NB, None, w)
        w_box = R.stats(pts, ids, NB)[1]
        assert same_bits(box, w_box)
        masks = []
        for cfg in ({"name": "DropAug", "p_drop_prob": 0.25}, {"name": "CropBoxAug"}, {"name": "CropPtsAug", "p_crop_ratio": 0.6}):
            kind, consts, _, _, _ = R.spec_of(cfg)
            mask = aug.aug_keep_mask(kind, consts, prob, p, b, NB, d, box if kind == "crop_box" else None, 11, None, 3, w)
            want = R.keep_mask(kind, consts, prob, pts, ids, NB, draws, w_box, 11, 3)
            assert np.array_equal(mask.cpu().numpy(), A.host_padded(want, rows)), kind       # absent rows: 0, every byte written
            masks.append((mask, want))
        # compaction of the last one, composed with an earlier index list; the mask's absent bytes made hostile again
        mask, want = masks[-1]
        mask[n:] = 0xFF
        idx_in = arena.alloc((rows,), torch.int32)
        idx_in[:n] = t(np.arange(n, dtype=np.int32)[::-1].copy())
        idx, n_out, kept, orig = aug.aug_compact(mask, b, NB, w, idx_in)
        w_idx, w_n, w_kept, w_orig = R.compact(want, ids, NB, None, np.arange(n, dtype=np.int32)[::-1])
        tail = np.full(rows - n, -1, dtype=np.int32)
        assert np.array_equal(idx.cpu().numpy(), np.concatenate((w_idx, tail))) and np.array_equal(orig.cpu().numpy(), np.concatenate((w_orig, tail)))
        assert n_out.cpu().tolist() == [w_n] and kept.cpu().tolist() == w_kept.tolist() and 0 < w_n < n
        # no present row at all: zeros, -1 and 0
        zero = arena.place(torch.tensor([0], dtype=torch.int32))
        c0, s0 = aug.aug_stats(p, b, NB, table, zero)
        assert not bool(c0.any()) and not bool(s0.view(torch.int32).any())
        assert not bool(aug.aug_apply(p, b, NB, table, n_valid=zero).view(torch.int32).any())
        i0, n0, k0, _ = aug.aug_compact(mask, b, NB, zero)
        assert bool((i0 == -1).all()) and n0.cpu().tolist() == [0] and not bool(k0.any())
        across_fills("entry points", workspace_fill, (counts, st, table, y, plain, box, idx, n_out, kept, orig) + tuple(m for m, _ in masks[:2]))


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_pipeline_in_the_arena(aug, request, workspace_fill):
    """The ScanNet list end to end with every allocation of the module in the arena: the result of the ordinary run, bit for bit."""
    cfgs = CFG.SCANNET
    pts, ids = A.cloud(6)
    draws = t(A.draws(7, len(cfgs)))
    n, rows = A.N, A.ROWS
    rng = np.random.default_rng(8)
    extras = [rng.standard_normal((n, 3)).astype(F), rng.random((n, 3)).astype(F), rng.integers(0, 20, n).astype(np.int64), np.arange(n, dtype=np.int32)]
    pipe = aug.AugPipeline()
    pipe.create_pipeline(cfgs)
    p0, b0, w0, _ = A.on_device(pts, ids, "copies")
    ordinary = pipe.augment_batch(p0, b0, NB, [t(A.host_padded(e, rows)) for e in extras], n_valid=w0, seed=99, draws=draws)
    with guarded(request, workspace_fill) as arena:
        p, b = in_arena(arena, t(pts), rows), in_arena(arena, t(ids), rows)
        w = arena.place(torch.tensor([n], dtype=torch.int32))
        ex = [in_arena(arena, t(e), rows) for e in extras]
        res = pipe.augment_batch(p, b, NB, ex, n_valid=w, seed=99, draws=arena.place(draws))
        kept = int(res.n_valid_)
        assert 0 < kept < n and kept == int(ordinary.n_valid_)
        assert same_bits(res.pts_, ordinary.pts_.cpu().numpy()) and not bool(res.pts_[kept:].view(torch.int32).any())
        assert torch.equal(res.idx_, ordinary.idx_) and bool((res.idx_[kept:] == -1).all())
        assert torch.equal(res.batch_ids_[:kept], ordinary.batch_ids_[:kept]) and same_bits(res.affine_, ordinary.affine_.cpu().numpy())
        for g, o in zip(res.extra_tensors_, ordinary.extra_tensors_):
            assert torch.equal(g[:kept], o[:kept]) and not bool(g[kept:].any())
        across_fills("pipeline", workspace_fill, (res.pts_, res.idx_, res.n_valid_, res.affine_))
