"""GPU: the entry points of include/se3conv_padded_rows.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the
policy of tests/test_gpu_padded_hostile_memory.py: feature rows, gradients, batch ids, every output and the workspace (sized
to exactly the query's value) come from an arena, so the absent rows hold the arena's fill (NaN features, batch id -1); no
band byte changes, the results are those of the calls on the present rows alone whatever the workspace held, every output
byte is a result or a stated zero / -1, and the entry points are proven to have been called."""
import pytest
import torch

import hostile_memory
import padded_rows_cases as R
from hostile_memory import in_arena
from padded_cases import DEV, same_bits, seeded_cloud
from padded_rows_cases import F32, I32, I64, FromArena, Plain, assert_rows, zero_bits

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_padded_rows.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_bn_fwd_padded": ["test_batch_norm_and_skip_connection"],
    "se3_bn_bwd_padded": ["test_batch_norm_and_skip_connection"],
    "se3_skip_fwd_padded": ["test_batch_norm_and_skip_connection"],
    "se3_skip_bwd_padded": ["test_batch_norm_and_skip_connection"],
    "se3_channel_sums_padded": ["test_batch_norm_and_skip_connection"],
    "se3_frame_pool_padded": ["test_frame_and_level_pooling"],
    "se3_frame_unpool_padded": ["test_frame_and_level_pooling"],
    "se3_segment_unpool_padded": ["test_frame_and_level_pooling"],
    "se3_rows_gather_padded": ["test_frame_and_level_pooling"],
    "se3_rows_unpick_padded": ["test_frame_and_level_pooling"],
}
# (n_rows, valid, frames, c): the vector path with a live grid below the launched one, and the scalar path
GLUE = [(3000, 1777, 2, 64), (1000, 593, 3, 3)]


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


def feats(rows, c, seed):
    return (torch.randn(rows, c, generator=torch.Generator().manual_seed(seed)) * 1.5 + 0.25).to(DEV)


def guarded(request, workspace_fill, needs_workspace):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=needs_workspace, with_recorder=True)


across_fills = hostile_memory.AcrossFills()


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_batch_norm_and_skip_connection(ops, request, workspace_fill):
    from se3conv3d_amd import _lib

    plain, real = Plain(), _lib.load()
    want = []
    for i, (n_rows, valid, f, c) in enumerate(GLUE):       # the trimmed calls, from the ordinary allocator
        p = valid * f
        x, dy, y2 = feats(p, c, 50 + i), feats(p, c, 60 + i), feats(p, c, 70 + i)
        w, b = feats(1, c, 80 + i).reshape(-1), feats(1, c, 90 + i).reshape(-1)
        rm, rv, nbt = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros(1, dtype=I64, device=DEV)
        y, mean, invstd = R.bn_fwd(real, plain, x, w, b, rm, rv, nbt)
        dx, dg, db = R.bn_bwd(real, plain, dy, x, mean, invstd, w)
        rb = R.row_batch_ids(valid, f).to(DEV)
        gate = torch.tensor([0.9, 0.5, 0.1], device=DEV)
        so = R.skip_fwd(real, plain, x, y2, w, gate, 0.8, rb)
        sdx, sdg = R.skip_bwd(real, plain, dy, x, w, gate, 0.8, rb)
        sums = R.channel_sums(real, plain, dy, (p, 1, None))
        want.append((x, dy, y2, w, b, rb, gate, (y, mean, invstd, rm, rv, nbt, dx, dg, db, so, sdx, sdg, sums)))
    with guarded(request, workspace_fill, True) as (arena, lib):
        A = FromArena(arena)
        for i, ((n_rows, valid, f, c), (x, dy, y2, w, b, rb, gate, ref)) in enumerate(zip(GLUE, want)):
            p, rows = valid * f, n_rows * f
            xp, dyp, y2p, rbp = (in_arena(arena, t, rows) for t in (x, dy, y2, rb))
            assert torch.isnan(xp[p:]).all() and bool((rbp[p:] == -1).all())
            wp, bp, gp = arena.place(w), arena.place(b), arena.place(gate)
            rm, rv = arena.place(torch.zeros(c, device=DEV)), arena.place(torch.ones(c, device=DEV))
            nbt = arena.place(torch.zeros(1, dtype=I64, device=DEV))
            pad = (n_rows, f, arena.place(torch.tensor([valid], dtype=I32)))
            y, mean, invstd = R.bn_fwd(lib, A, xp, wp, bp, rm, rv, nbt, pad)
            dx, dg, db = R.bn_bwd(lib, A, dyp, xp, mean, invstd, wp, pad)
            so = R.skip_fwd(lib, A, xp, y2p, wp, gp, 0.8, rbp, pad)
            sdx, sdg = R.skip_bwd(lib, A, dyp, xp, wp, gp, 0.8, rbp, pad)
            got = (y, mean, invstd, rm, rv, nbt, dx, dg, db, so, sdx, sdg, R.channel_sums(lib, A, dyp, pad))
            for k, (a_, b_) in enumerate(zip(got, ref)):
                if a_.dim() == 2:
                    assert_rows(a_, b_, p, (i, k))
                else:
                    assert same_bits(a_, b_), (i, k)
            across_fills(("glue", i), workspace_fill, got)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_frame_and_level_pooling(ops, request, workspace_fill):
    from padded_cases import padded, word
    from se3conv3d_amd import _lib

    plain, real = Plain(), _lib.load()
    n_rows, valid, f, c = 700, 450, 3, 12
    x, g = feats(valid * f, c, 1), feats(valid, c, 2)
    x[::3] = x[::3].round()
    frame_ref = []
    for mode in range(4):
        out, arg = R.frame_pool(real, plain, x, f, mode)
        frame_ref.append((out, arg, R.frame_unpool(real, plain, g, arg, f, mode)))
    # a level with dropped cells (capacity = half the cell count), averaged and random, built outside the arena
    pts, bid = seeded_cloud(valid, 2, 77)
    trimmed = ops.grid_subsample(pts.to(DEV), bid.to(DEV), 0.15, 2)
    cap = trimmed.n_cells // 2
    pp, bb = (t.to(DEV) for t in padded(pts, bid, n_rows, "nan", 7))
    u = torch.rand(trimmed.n_cells, generator=torch.Generator().manual_seed(5)).to(DEV)
    lv = ops.grid_levels_bounded(pp, bb, [0.15], [cap], 2, n_valid=word(valid), rnd=[True], rnd_values=[u[:cap].contiguous()]).levels[0]
    _, picked_t = ops.grid_pick(trimmed, u)
    kept_rows = torch.zeros(n_rows, dtype=torch.bool, device=DEV)
    kept_rows[:valid] = lv["cell_ids"][:valid] >= 0
    vals = feats(cap, c, 3)
    vfull = torch.zeros(trimmed.n_cells, c, device=DEV)
    vfull[:cap] = vals
    xs = feats(valid, c, 4)
    level_ref = []
    for mode in range(4):
        _, arg_t = R.segment_pool(real, plain, xs, trimmed.sorted_ids, trimmed.cell_ends, trimmed.n_cells, mode)
        level_ref.append((arg_t, R.segment_unpool(real, plain, vfull, trimmed.cell_ids, trimmed.cell_ends, arg_t, mode)))
    sub_t = ops.rows_gather(xs, picked_t[:cap].contiguous())
    up_t = ops.rows_scatter(vals, picked_t[:cap].contiguous(), valid)
    with guarded(request, workspace_fill, False) as (arena, lib):
        A = FromArena(arena)
        xp, gp = in_arena(arena, x, n_rows * f), in_arena(arena, g, n_rows)
        w = arena.place(torch.tensor([valid], dtype=I32))
        got = []
        for mode, (out_t, arg_t, gx_t) in enumerate(frame_ref):
            out, arg = R.frame_pool(lib, A, xp, f, mode, w, padded=True)
            gx = R.frame_unpool(lib, A, gp, arg, f, mode, w, padded=True)
            assert_rows(out, out_t, valid, mode), assert_rows(gx, gx_t, valid * f, mode)
            if arg is not None:
                assert torch.equal(arg[:valid], arg_t) and bool((arg[valid:] == -1).all())
            got += [out, gx]
        ids, ends, picked = arena.place(lv["cell_ids"]), arena.place(lv["cell_ends"]), arena.place(lv["picked"])
        vp, xsp = arena.place(vals), in_arena(arena, xs, n_rows)
        for mode, (arg_t, back_t) in enumerate(level_ref):
            arg = arena.place(arg_t[:cap].contiguous()) if arg_t is not None else None
            back = R.segment_unpool(lib, A, vp, ids, ends, arg, mode, padded=True)
            assert same_bits(back[kept_rows], back_t[kept_rows[:valid]]) and zero_bits(back[~kept_rows]), mode
            got.append(back)
        sub = R.rows_gather_padded(lib, A, xsp, picked)
        assert_rows(sub, sub_t, cap, "gather")
        up = R.rows_unpick_padded(lib, A, vp, ids, picked)
        assert_rows(up, up_t, valid, "unpick")
        across_fills("pooling", workspace_fill, got + [sub, up])
