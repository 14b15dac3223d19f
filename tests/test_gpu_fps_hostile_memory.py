"""GPU: se3_fps on 0xFF-filled, guard-banded buffers (tests/hostile_memory.py) -- the policy of
tests/test_gpu_hostile_memory.py for the entry points of include/se3conv_fps.h: every output and the workspace (sized to
exactly the query's value) come from an arena, no band byte changes, the results are those of the numpy contract whatever the
workspace held, every output byte is a result or a stated pad value, and the entry points are proven to have been called."""
import numpy as np
import pytest
import torch

import fps_reference as R
import hostile_memory
from test_gpu_fps import DEV, assert_exact, bits, cloud, draws

pytestmark = pytest.mark.gpu

# entry point (include/se3conv_fps.h) -> the tests of this module that run it inside the arena and assert that they did
ALL = ["test_resident_form", "test_streaming_form", "test_absent_rows"]
COVERED = {"se3_fps": ALL, "se3_fps_workspace_bytes": ALL}


@pytest.fixture(scope="module")
def ops(built_library):
    import se3conv3d_amd as amd
    return amd.ops


def guarded(request, workspace_fill):
    return hostile_memory.guarded(request, COVERED, DEV, workspace_fill)


def assert_written(res, arena, n_rows, nb):
    """No output byte still holds the fill unless the contract puts a -1 there (assert_exact has checked where), no float
    is NaN, and the workspace is exactly the query's value: its high band starts on the first byte past it."""
    from se3conv3d_amd import _lib

    assert not torch.isnan(res.d2).any() and bool((res.info >= 0).all()) and bool((res.starts >= 0).all())
    need = _lib.load().se3_fps_workspace_bytes(n_rows, nb)
    ws = [a for a in arena.allocations if a.label.startswith("workspace of")]
    assert ws and all(a.nbytes == need >= 256 for a in ws)


def snapshot(res):
    return [bits(t).copy() for t in (res.ids, res.d2, res.starts, res.info)]


def same_snapshot(a, b, key):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), key


across_fills = hostile_memory.AcrossFills(snapshot, same_snapshot)


def run_in(arena, ops, pts, bid, ratio, nb, u, **kw):
    place = lambda a: arena.place(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return ops.fps(place(pts), place(bid), ratio, nb, start_u=place(u), **kw)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_resident_form(ops, request, workspace_fill):
    pts, bid = cloud([300, 0, 1025], 41)
    u = draws(3, 42)
    ref = R.fps_reference(pts, bid, 0.05, 3, u)
    with guarded(request, workspace_fill) as arena:
        for cap in (None, len(ref[0]), len(ref[0]) - 4):
            res = run_in(arena, ops, pts, bid, 0.05, 3, u, capacity=cap)
            assert_exact(res, ref, flags=(int(cap is not None and cap < len(ref[0])), 0))
            assert_written(res, arena, len(bid), 3)
            across_fills(("resident", cap), workspace_fill, res)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_streaming_form(ops, request, workspace_fill):
    from se3conv3d_amd import _lib

    pts, bid = cloud([70, _lib.FPS_RESIDENT_MAX + 1], 43)
    u = draws(2, 44)
    ratio = 40.0 / _lib.FPS_RESIDENT_MAX
    ref = R.fps_reference(pts, bid, ratio, 2, u)
    assert np.diff(ref[2]).tolist() == [1, 41]
    with guarded(request, workspace_fill) as arena:
        res = run_in(arena, ops, pts, bid, ratio, 2, u)
        assert_exact(res, ref)
        assert_written(res, arena, len(bid), 2)
        across_fills(("streaming",), workspace_fill, res)


@pytest.mark.parametrize("workspace_fill", [0x00, 0xFF])
def test_absent_rows(ops, request, workspace_fill):
    """The cloud inside 3000-row arrays whose tail is the arena's fill (NaN points, batch id -1), behind a device word."""
    pts, bid = cloud([600, 1177], 45)
    u = draws(2, 46)
    ref = R.fps_reference(pts, bid, 0.25, 2, u)
    with guarded(request, workspace_fill) as arena:
        p, b = arena.alloc((3000, 3), torch.float32), arena.alloc((3000,), torch.int32)
        p[:1777], b[:1777] = torch.from_numpy(pts).to(DEV), torch.from_numpy(bid).to(DEV)
        assert torch.isnan(p[1777:]).all() and bool((b[1777:] == -1).all())
        word = arena.place(torch.tensor([1777], dtype=torch.int32))
        res = ops.fps(p, b, 0.25, 2, start_u=arena.place(torch.from_numpy(u).to(DEV)), n_valid=word)
        assert_exact(res, ref)
        assert_written(res, arena, 3000, 2)
        across_fills(("absent",), workspace_fill, res)
