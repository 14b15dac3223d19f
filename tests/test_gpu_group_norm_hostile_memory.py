"""GPU: the device entry points of include/se3conv_group_norm.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py)
-- the policy of tests/test_gpu_global_pool_hostile_memory.py: the features, the gradient, the ids, every output and the
workspace (sized to exactly the query's value) come from an arena, so the absent rows hold the arena's fill (NaN features, id
-1); no band byte changes, the results are those of the numpy contract bit for bit whatever the workspace held, every output
byte is a result, and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import group_norm_reference as R
import hostile_memory
from hostile_memory import in_arena
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_group_norm.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_group_norm_fwd": ["test_forward_and_backward", "test_module_on_a_padded_cloud"],
    "se3_group_norm_bwd": ["test_forward_and_backward", "test_module_on_a_padded_cloud"],
}
ROWS, VALID, FRAMES, C, GROUPS, NB = 2 * R.CHUNK + 100, R.CHUNK + 37, 2, 72, 8, 4     # 72 channels: wavefronts that straddle two chunks


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_group_norm.h", _lib.GROUP_NORM_SIGNATURES)


def guarded(request, workspace_fill, workspace=True):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=workspace)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


def case():
    rng = np.random.default_rng(22)
    ids = R.sized_ids(R.split(VALID, NB, empty=2), seed=5)
    ids[::41] = NB + 3                                                   # points of no element
    x = (rng.standard_normal((VALID * FRAMES, C)) * 1.5 + 0.5).astype(np.float32)
    g = rng.standard_normal((VALID * FRAMES, C)).astype(np.float32)
    return ids, x, g, rng.uniform(0.5, 1.5, (1, C)).astype(np.float32), rng.uniform(-0.5, 0.5, (1, C)).astype(np.float32)


def contract(ids, x, g, gamma, beta, valid):
    y, mean, invstd = R.forward(x, gamma, beta, ids, NB, GROUPS, R.EPS, FRAMES, valid)
    return (y,) + R.backward(g, x, gamma, mean, invstd, ids, NB, GROUPS, FRAMES, valid)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_forward_and_backward(ops, request, workspace_fill):
    ids, x, g, gamma, beta = case()
    with guarded(request, workspace_fill) as arena:
        idp = in_arena(arena, t(ids), ROWS)
        gp = in_arena(arena, t(g), ROWS * FRAMES)
        assert torch.isnan(gp[VALID * FRAMES:]).all() and bool((idp[VALID:] == -1).all())
        for valid in (VALID, 0):
            w = arena.place(torch.tensor([valid], dtype=torch.int32))
            xp = in_arena(arena, t(x), ROWS * FRAMES).requires_grad_(True)
            ga, be = arena.place(t(gamma)).requires_grad_(True), arena.place(t(beta)).requires_grad_(True)
            y = ops.GroupNorm.apply(xp, ga, be, idp, NB, GROUPS, R.EPS, w, FRAMES)
            y.backward(gp)
            w_y, w_dx, w_dgamma, w_dbeta = contract(ids, x, g, gamma, beta, valid)
            n = VALID * FRAMES
            assert np.array_equal(bits(y[:n]), bits(w_y)) and np.array_equal(bits(xp.grad[:n]), bits(w_dx)), valid
            assert not bits(y[n:]).any() and not bits(xp.grad[n:]).any()                      # every byte written: absent rows +0.0
            assert np.array_equal(bits(ga.grad.reshape(-1)), bits(w_dgamma)) and np.array_equal(bits(be.grad.reshape(-1)), bits(w_dbeta))
            across_fills(("padded", valid), workspace_fill, (y.detach(), xp.grad, ga.grad, be.grad))
        # without a word every row of a (whole) buffer is present
        xw = arena.place(t(x)).requires_grad_(True)
        y = ops.GroupNorm.apply(xw, arena.place(t(gamma)), arena.place(t(beta)), arena.place(t(ids)), NB, GROUPS, R.EPS, None, FRAMES)
        y.backward(arena.place(t(g)))
        w_y, w_dx, _, _ = contract(ids, x, g, gamma, beta, None)
        assert np.array_equal(bits(y), bits(w_y)) and np.array_equal(bits(xw.grad), bits(w_dx))
        across_fills("whole", workspace_fill, (y.detach(), xw.grad))
        # no rows at all: nothing to write but the statistics, which are zeros
        x0 = arena.alloc((0, C), torch.float32).requires_grad_(True)
        y0 = ops.GroupNorm.apply(x0, arena.place(t(gamma)), arena.place(t(beta)), arena.alloc((0,), torch.int32), NB, GROUPS, R.EPS)
        y0.sum().backward()
        assert y0.shape == (0, C) and x0.grad.shape == (0, C)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_module_on_a_padded_cloud(request, workspace_fill, built_library):
    """`blocks.GroupNormPC` on a `p_padded_rows` cloud, forward and backward, on arena buffers."""
    import se3conv3d_amd as amd

    ids, x, g, gamma, beta = case()
    with guarded(request, workspace_fill) as arena:
        pts = arena.alloc((ROWS, 3), torch.float32)
        idp = in_arena(arena, t(ids), ROWS)
        frames = arena.alloc((ROWS, FRAMES, 9), torch.float32)
        w = arena.place(torch.tensor([VALID], dtype=torch.int32))
        pc = amd.pc.PointcloudRotEquiv.from_frames(pts, idp, frames, p_n_valid=w, num_batches=NB, p_padded_rows=True)
        norm = amd.GroupNormPC(C, GROUPS).to(DEV)
        with torch.no_grad():
            norm.gamma_.copy_(t(gamma)), norm.betas_.copy_(t(beta))
        xp = in_arena(arena, t(x), ROWS * FRAMES).requires_grad_(True)
        y = norm(xp, pc)
        y.backward(in_arena(arena, t(g), ROWS * FRAMES))
        w_y, w_dx, w_dgamma, w_dbeta = contract(ids, x, g, gamma, beta, VALID)
        n = VALID * FRAMES
        assert np.array_equal(bits(y[:n]), bits(w_y)) and np.array_equal(bits(xp.grad[:n]), bits(w_dx))
        assert not bits(y[n:]).any() and not bits(xp.grad[n:]).any()
        assert np.array_equal(bits(norm.gamma_.grad.reshape(-1)), bits(w_dgamma)) and np.array_equal(bits(norm.betas_.grad.reshape(-1)), bits(w_dbeta))
        across_fills("module", workspace_fill, (y.detach(), xp.grad, norm.gamma_.grad, norm.betas_.grad))
