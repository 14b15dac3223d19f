"""GPU: the device entry points of include/se3conv_seg_head.h on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) --
the policy of tests/test_gpu_group_norm_hostile_memory.py: logits, labels, the class mask, the word, every output and the
workspace (sized to exactly the query's value) come from an arena, so the absent rows hold the arena's fill (NaN logits, label
-1); no band byte changes, the results are those of the trimmed call whatever the workspace held, every output byte is a result
-- except `tallies`, the one buffer the library adds to, which must hold its pre-fill plus the counts -- and the entry points
are proven to have been called."""
import numpy as np
import pytest
import torch

import hostile_memory
import seg_head_reference as R
from hostile_memory import in_arena
from padded_cases import DEV
from se3conv3d_amd import _lib

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_seg_head.h) -> the tests of this module that run it inside the arena and assert that they did
COVERED = {
    "se3_seg_loss_fwd": ["test_forward_and_backward", "test_metrics_on_a_padded_cloud"],
    "se3_seg_loss_bwd": ["test_forward_and_backward", "test_metrics_on_a_padded_cloud"],
}
ROWS, VALID, EPS = 2 * R.CHUNK + 100, R.CHUNK + 37, 0.1
WIDTHS = [21, R.TILE_CLASSES + 1]                                     # the LDS-tile form and the form that reads rows in memory


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


@pytest.fixture(autouse=True)
def recorded(monkeypatch):
    """hostile_memory's Recorder notes the names of `_lib.TABLES`: the header of the third registry stands there for the
    duration of a test."""
    monkeypatch.setitem(_lib.TABLES, "se3conv_seg_head.h", _lib.SEG_HEAD_SIGNATURES)


def guarded(request, workspace_fill, workspace=True):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill, workspace=workspace)


across_fills = hostile_memory.AcrossFills()
t = lambda a: torch.from_numpy(np.array(a, copy=True)).to(DEV)
bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


def case(classes):
    x, y = R.case(VALID, classes, 300 + classes, masked=(classes - 1,))
    return x, y, R.counted_of(classes, (classes - 1,))


def contract(x, y, counted, valid, pre):
    """The numpy contract on the present rows: `(loss, count, tallies = pre + counts, grad)` (grad for a gradient of 1)."""
    tallies = pre.copy()
    loss, count, lse, _ = R.forward(x[:valid], y[:valid], EPS, counted, None, tallies)
    return loss, count, tallies, R.backward(x[:valid], y[:valid], lse, count, 1.0, EPS, counted)


def assert_close_to_contract(loss, grad, want_loss, want_grad, count, what):
    """The bounds of tests/test_gpu_seg_head.py: the loss to one fp32 unit, the gradient to one fp32 unit plus 1e-13 / count."""
    assert abs(float(loss) - float(want_loss)) <= R.ulp32(want_loss), what
    bound = R.ulp32(want_grad) + 1e-13 / max(count, 1)
    assert (np.abs(grad.astype(np.float64) - want_grad.astype(np.float64)) <= bound).all(), what


@pytest.mark.parametrize("classes", WIDTHS)
@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_forward_and_backward(ops, request, workspace_fill, classes):
    x, y, counted = case(classes)
    pre = np.arange(3 * classes, dtype=np.int64).reshape(3, classes) * 1000
    with guarded(request, workspace_fill) as arena:
        cd = arena.place(t(counted))
        for labels in (y, y.astype(np.int32)):
            xp_ = in_arena(arena, t(x), ROWS)
            yp = in_arena(arena, t(labels), ROWS)
            assert torch.isnan(xp_[VALID:]).all() and bool((yp[VALID:] == -1).all())
            for valid in (VALID, 0):
                w = arena.place(torch.tensor([valid], dtype=torch.int32))
                xp = xp_.detach().requires_grad_(True)
                tallies = arena.place(t(pre))
                loss = ops.seg_loss(xp, yp, EPS, counted=cd, n_valid=w, tallies=tallies)
                loss.backward(arena.place(torch.ones((), device=DEV)))
                w_loss, w_count, w_tallies, w_grad = contract(x, labels, counted, valid, pre)
                assert np.array_equal(tallies.cpu().numpy(), w_tallies), valid        # the pre-fill plus the counts, nothing else
                assert_close_to_contract(loss, xp.grad[:valid].cpu().numpy(), w_loss, w_grad, w_count, valid)
                assert not bits(xp.grad[valid:]).any()                                # every byte written: other rows +0.0
                if valid == 0:
                    assert bits(loss.detach().reshape(1))[0] == 0
                across_fills(("padded", classes, labels.dtype.name, valid), workspace_fill, (loss.detach().reshape(1), xp.grad, tallies))
        # without a word every row of a (whole) buffer is present; without tallies and without a backward (lse NULL)
        xw, yw = arena.place(t(x)).requires_grad_(True), arena.place(t(y))
        loss = ops.seg_loss(xw, yw, EPS, counted=cd)
        loss.backward(arena.place(torch.ones((), device=DEV)))
        w_loss, w_count, _, w_grad = contract(x, y, counted, VALID, pre)
        assert_close_to_contract(loss, xw.grad.cpu().numpy(), w_loss, w_grad, w_count, "whole")
        with torch.no_grad():
            alone = ops.seg_loss(arena.place(t(x)), yw, EPS, counted=cd)
        assert bits(alone.reshape(1))[0] == bits(loss.detach().reshape(1))[0]
        across_fills(("whole", classes), workspace_fill, (loss.detach().reshape(1), xw.grad))
        # no rows at all: loss and count are written, nothing else is
        x0 = arena.alloc((0, classes), torch.float32).requires_grad_(True)
        tallies = arena.place(t(pre))
        l0 = ops.seg_loss(x0, arena.alloc((0,), torch.int64), EPS, counted=cd, tallies=tallies)
        l0.backward()
        assert bits(l0.detach().reshape(1))[0] == 0 and x0.grad.shape == (0, classes) and np.array_equal(tallies.cpu().numpy(), pre)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_metrics_on_a_padded_cloud(request, workspace_fill, built_library):
    """`metrics.SemSegMetrics.loss` and its device `update_metrics` on arena buffers: the counters live in the arena too."""
    import se3conv3d_amd as amd

    classes = 21
    x, y, counted = case(classes)
    with guarded(request, workspace_fill) as arena:
        m = amd.SemSegMetrics(classes, [classes - 1], device=DEV)
        m.tallies_, m.counted_ = arena.place(m.tallies_), arena.place(m.counted_)
        xp, yp = in_arena(arena, t(x), ROWS).requires_grad_(True), in_arena(arena, t(y), ROWS)
        w = arena.place(torch.tensor([VALID], dtype=torch.int32))
        loss = m.loss(xp, yp, EPS, n_valid=w)
        loss.backward(arena.place(torch.ones((), device=DEV)))
        m.update_metrics(xp.detach(), yp, n_valid=w)                          # the counters alone: a second time the same counts
        w_loss, w_count, w_tallies, w_grad = contract(x, y, counted, VALID, np.zeros((3, classes), np.int64))
        assert np.array_equal(m.tallies_.cpu().numpy(), 2 * w_tallies)
        assert np.array_equal(m.accum_gt_, 2.0 * w_tallies[0]) and np.array_equal(m.accum_intersection_, 2.0 * w_tallies[2])
        assert_close_to_contract(loss, xp.grad[:VALID].cpu().numpy(), w_loss, w_grad, w_count, "metrics")
        assert not bits(xp.grad[VALID:]).any()
        across_fills("metrics", workspace_fill, (loss.detach().reshape(1), xp.grad, m.tallies_))
