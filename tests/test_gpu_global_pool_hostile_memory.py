"""GPU: the device entry points of include/se3conv_global_pool.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py)
-- the policy of tests/test_gpu_knn_edges_hostile_memory.py: the features, the ids, every output and the workspace (sized to
exactly the query's value) come from an arena, so the absent rows hold the arena's fill (NaN features, id -1); no band byte
changes, the results are those of the numpy contract bit for bit whatever the workspace held, every output byte is a result,
and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import global_pool_reference as R
import hostile_memory
from hostile_memory import in_arena
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_global_pool.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_global_pool": ["test_pool_and_unpool", "test_cloud_methods"],
    "se3_global_unpool": ["test_pool_and_unpool", "test_cloud_methods"],
}
ROWS, VALID, FRAMES, C, NB = 2 * R.CHUNK + 100, R.CHUNK + 37, 2, 65, 4      # 65 channels: wavefronts that straddle two chunks


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_global_pool.h", _lib.GLOBAL_POOL_SIGNATURES)


def guarded(request, workspace_fill, workspace=True):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=workspace)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def case():
    rng = np.random.default_rng(21)
    ids = R.sized_ids(R.split(VALID, NB, empty=2))
    ids[::41] = NB + 3                                                   # points of no element
    x = (rng.standard_normal((VALID * FRAMES, C)) * 1.5).astype(np.float32)
    x[::5] = np.round(x[::5])                                            # ties
    g = rng.standard_normal((NB, C)).astype(np.float32)
    return ids, x, g


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_pool_and_unpool(ops, request, workspace_fill):
    ids, x, g = case()
    with guarded(request, workspace_fill) as arena:
        xp, idp = in_arena(arena, t(x), ROWS * FRAMES), in_arena(arena, t(ids), ROWS)
        assert torch.isnan(xp[VALID * FRAMES:]).all() and bool((idp[VALID:] == -1).all())
        gp = arena.place(t(g))
        for valid in (VALID, 0):
            w = arena.place(torch.tensor([valid], dtype=torch.int32))
            for mode in range(4):
                out, arg, counts = ops.global_pool(xp, idp, NB, mode, FRAMES, n_valid=w)
                w_out, w_arg, w_counts = R.global_pool(x, ids, NB, mode, FRAMES, valid)
                assert np.array_equal(bits(out.cpu().numpy()), bits(w_out)), (valid, mode)
                assert counts.cpu().tolist() == w_counts.tolist() and (arg is None) == (mode in (R.AVG, R.SUM))
                if arg is not None:
                    assert np.array_equal(arg.cpu().numpy(), w_arg)
                back = ops.global_unpool(gp, idp, mode, FRAMES, n_valid=w, arg=arg, counts=counts)
                assert np.array_equal(bits(back[:VALID * FRAMES].cpu().numpy()), bits(R.global_unpool(g, ids, w_arg, w_counts, mode, FRAMES, valid)))
                assert not bool(back[VALID * FRAMES:].view(torch.int32).any())    # every byte written: absent rows +0.0
                across_fills(("pool", valid, mode), workspace_fill, (out, counts, back) + (() if arg is None else (arg,)))
        # without a word every row of a (whole) buffer is present
        whole_x, whole_ids = arena.place(t(x)), arena.place(t(ids))
        out, _, counts = ops.global_pool(whole_x, whole_ids, NB, "avg", FRAMES)
        assert np.array_equal(bits(out.cpu().numpy()), bits(R.global_pool(x, ids, NB, R.AVG, FRAMES)[0]))
        # no rows at all: zeros, -1 and 0, and the un-pooling has nothing to write
        out, arg, counts = ops.global_pool(arena.alloc((0, C), torch.float32), arena.alloc((0,), torch.int32), NB, "max", FRAMES)
        assert not bool(out.view(torch.int32).any()) and bool((arg == -1).all()) and not bool(counts.any())
        assert ops.global_unpool(gp, arena.alloc((0,), torch.int32), "sum", FRAMES).shape == (0, C)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_cloud_methods(ops, request, workspace_fill):
    """The three methods of a padded cloud with `p_native=True`, forward and backward, on arena buffers."""
    import se3conv3d_amd as amd

    ids, x, g = case()
    with guarded(request, workspace_fill) as arena:
        pts = arena.alloc((ROWS, 3), torch.float32)
        idp = in_arena(arena, t(ids), ROWS)
        frames = arena.alloc((ROWS, FRAMES, 9), torch.float32)
        w = arena.place(torch.tensor([VALID], dtype=torch.int32))
        pc = amd.pc.PointcloudRotEquiv.from_frames(pts, idp, frames, p_n_valid=w, num_batches=NB, p_padded_rows=True)
        xp = in_arena(arena, t(x), ROWS * FRAMES).requires_grad_(True)
        gp = arena.place(t(g))
        y = pc.global_pooling(xp, "avg", p_native=True)
        y.backward(gp)
        w_out, w_arg, w_counts = R.global_pool(x, ids, NB, R.AVG, FRAMES, VALID)
        assert np.array_equal(bits(y.detach().cpu().numpy()), bits(w_out))
        want = R.global_unpool(g, ids, w_arg, w_counts, R.AVG, FRAMES, VALID)
        assert np.array_equal(bits(xp.grad[:VALID * FRAMES].cpu().numpy()), bits(want)) and not bool(xp.grad[VALID * FRAMES:].view(torch.int32).any())
        xp.grad = None
        y2 = pc.global_pooling_specific_feature_pooling(xp, "max", "min", p_native=True)
        y2.backward(gp)
        pooled = x.reshape(VALID, FRAMES, C).min(1)
        assert np.array_equal(bits(y2.detach().cpu().numpy()), bits(R.global_pool(pooled, ids, NB, R.MAX, 1)[0]))
        assert not bool(xp.grad[VALID * FRAMES:].view(torch.int32).any()) and bool(torch.isfinite(xp.grad).all())
        z = gp.clone().requires_grad_(True)
        up = pc.global_upsample(z, p_native=True)
        up_g = in_arena(arena, t(x), ROWS * FRAMES)
        up.backward(up_g)
        assert np.array_equal(bits(up[:VALID * FRAMES].detach().cpu().numpy()), bits(R.global_unpool(g, ids, None, None, R.SUM, FRAMES, VALID)))
        assert not bool(up[VALID * FRAMES:].detach().view(torch.int32).any())
        assert np.array_equal(bits(z.grad.cpu().numpy()), bits(R.global_pool(x, ids, NB, R.SUM, FRAMES, VALID)[0]))
        across_fills("cloud", workspace_fill, (y.detach(), y2.detach(), up.detach(), z.grad))
