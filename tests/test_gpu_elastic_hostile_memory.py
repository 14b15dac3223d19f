"""GPU: the device entry points of include/se3conv_elastic.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_augment_hostile_memory.py: points, ids, draws, the raw numbers, every output, the grid and the
workspace (sized to exactly the query's value, filled 0x00 and 0xFF) come from an arena, so the absent rows hold the arena's
fill (NaN points, id -1); no band byte changes, the grid's tail behind the placed total keeps its fill, the results are those
of the numpy restatement whatever the workspace held, and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import augment_cases as A
import augment_configs as CFG
import augment_reference as R
import elastic_cases as EC
import elastic_reference as E
import hostile_memory
from augment_cases import DEV, same_bits, t
from hostile_memory import in_arena
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
GRAN, MAG = CFG.SCANNET_ELASTIC["p_granularity"], CFG.SCANNET_ELASTIC["p_magnitude"]

# entry point (include/se3conv_elastic.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_elastic_plan": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
    "se3_elastic_grids": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
    "se3_elastic_displace": ["test_entry_points_one_by_one", "test_pipeline_in_the_arena"],
}
SIZES = (70, 0, 1, 65, 90)   # an empty and a one-row element; the last one finds no room


@pytest.fixture(scope="module")
def aug(built_library):
    from se3conv3d_amd import augment
    return augment


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_elastic.h", _lib.ELASTIC_SIGNATURES)


def guarded(request, workspace_fill):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=True)


across_fills = hostile_memory.AcrossFills()


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_entry_points_one_by_one(aug, request, workspace_fill):
    nb = len(SIZES)
    pts, ids = A.cloud(13, SIZES)
    pts = (pts * F(0.7)).astype(F)
    n, rows = len(pts), len(pts) + 203
    draws = A.draws(14, nb=nb)
    draws[:, 0] = [0.1, 0.2, 0.3, 0.4, 0.5]
    w_counts, w_st = R.stats(pts, ids, nb)
    full = E.plan(w_counts, w_st, draws, 0.8, GRAN, 1 << 40)[0]
    cap = int(full[4, 0, 3]) + 50                                         # room for elements 0, 2 and 3; 50 cells behind them
    want_table, want_flag, want_prefix = E.plan(w_counts, w_st, draws, 0.8, GRAN, cap)
    total = cap - 50
    assert want_flag == 1 and [e for e in range(nb) if want_table[e, 0, 3] >= 0] == [0, 2, 3]
    noise = EC.noise_rows(EC.recorded_stream(), cap)
    with guarded(request, workspace_fill) as arena:
        p, b = in_arena(arena, t(pts), rows), in_arena(arena, t(ids), rows)
        assert torch.isnan(p[n:]).all() and bool((b[n:] == -1).all())
        w, d = arena.place(torch.tensor([n], dtype=torch.int32)), arena.place(t(draws))
        counts, st = aug.aug_stats(p, b, nb, None, w)
        assert counts.cpu().tolist() == w_counts.tolist() and same_bits(st, w_st)
        # plan: table, word and every word of the workspace
        table, word, ws = aug.aug_elastic_plan(counts, st, d, 0.8, GRAN, cap)
        assert np.array_equal(table.cpu().numpy(), want_table) and int(word) == want_flag
        assert ws.numel() == _lib.load().se3_elastic_workspace_bytes(nb, 3)
        assert np.array_equal(ws[:8 * (nb * 3 + 1)].view(torch.int64).cpu().numpy(), want_prefix)
        # grids of given numbers: bit for bit, the tail untouched, no NaN from lane 3 or from behind the placed total
        grid = aug.aug_elastic_grids(table, ws, cap, noise_in=arena.place(t(noise)))
        want_grid = E.grids(want_table, cap, noise_in=noise)
        assert grid.shape == (cap, 4) and same_bits(grid[:total], want_grid[:total]) and not np.isnan(want_grid[:total]).any()
        assert arena.holds_fill(grid[total:])
        # grids from the hash: the values of the restatement (device logf / cosf: to 1e-5), the same tail
        hashed = aug.aug_elastic_grids(table, ws, cap, 11, None, 3)
        want_hashed = E.grids(want_table, cap, 11, 3, dtype=np.float64)
        assert float(np.abs(hashed[:total].cpu().numpy() - want_hashed[:total]).max()) < 1e-5 and arena.holds_fill(hashed[total:])
        # displace: no absent row is read (NaN points, id -1), absent rows zero, element 4 (no room) copied
        y = aug.aug_elastic_displace(p, b, nb, st, table, MAG, grid, w)
        want = E.displace(pts, ids, nb, w_st, want_table, MAG, want_grid)
        assert same_bits(y, A.host_padded(want, rows)) and not bool(y[n:].view(torch.int32).any())
        assert np.array_equal(A.bits(want[ids == 4]), A.bits(pts[ids == 4])) and (np.abs(want - pts).max(1)[ids != 4] > 0).all()
        # no present row at all
        zero = arena.place(torch.tensor([0], dtype=torch.int32))
        c0, s0 = aug.aug_stats(p, b, nb, None, zero)
        t0, w0, ws0 = aug.aug_elastic_plan(c0, s0, d, 0.8, GRAN, cap)
        assert int(w0) == 0 and bool((t0[:, :, 3] == -1).all()) and not bool(t0[:, :, 0:3].any()) and not bool(ws0[:8 * (nb * 3 + 1)].any())
        g0 = aug.aug_elastic_grids(t0, ws0, cap, 11, None, 3)
        assert arena.holds_fill(g0)
        assert not bool(aug.aug_elastic_displace(p, b, nb, s0, t0, MAG, g0, zero).view(torch.int32).any())
        across_fills("entry points", workspace_fill, (table, word, grid[:total], hashed[:total], y))


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_pipeline_in_the_arena(aug, request, workspace_fill):
    """The ScanNet list with its elastic step, every allocation of the module in the arena: the ordinary run bit for bit."""
    cfgs = CFG.SCANNET[:6] + [CFG.SCANNET_ELASTIC] + CFG.SCANNET[6:]
    nb = len(SIZES)
    pts, ids = A.cloud(16, SIZES)
    n, rows = len(pts), len(pts) + 203
    draws = A.draws(17, len(cfgs), nb)
    draws[6, :, 0] = 0.5
    rng = np.random.default_rng(18)
    extras = [rng.standard_normal((n, 3)).astype(F), rng.random((n, 3)).astype(F), rng.integers(0, 20, n).astype(np.int64), np.arange(n, dtype=np.int32)]
    pipe = aug.AugPipeline(p_elastic=True)
    pipe.create_pipeline(cfgs)
    cap = pipe.elastic_capacity((2.0, 2.0, 2.0), nb)
    p0, b0, w0 = t(A.host_padded(pts, rows)), t(A.host_padded(ids, rows)), torch.tensor([n], dtype=torch.int32, device=DEV)
    ordinary = pipe.augment_batch(p0, b0, nb, [t(A.host_padded(e, rows)) for e in extras], n_valid=w0, seed=99, draws=t(draws), grid_capacity=cap)
    with guarded(request, workspace_fill) as arena:
        p, b = in_arena(arena, t(pts), rows), in_arena(arena, t(ids), rows)
        w = arena.place(torch.tensor([n], dtype=torch.int32))
        ex = [in_arena(arena, t(e), rows) for e in extras]
        res = pipe.augment_batch(p, b, nb, ex, n_valid=w, seed=99, draws=arena.place(t(draws)), grid_capacity=cap)
        kept = int(res.n_valid_)
        assert 0 < kept < n and kept == int(ordinary.n_valid_) and res.overflow_.cpu().tolist() == [0]
        assert same_bits(res.pts_, ordinary.pts_.cpu().numpy()) and not bool(res.pts_[kept:].view(torch.int32).any())
        assert torch.equal(res.idx_, ordinary.idx_) and bool((res.idx_[kept:] == -1).all())
        for g, o in zip(res.extra_tensors_, ordinary.extra_tensors_):
            assert torch.equal(g[:kept], o[:kept]) and not bool(g[kept:].any())
        across_fills("pipeline", workspace_fill, (res.pts_, res.idx_, res.n_valid_, res.overflow_))
