"""CPU: the guard-band harness itself (tests/hostile_memory.py) on CPU tensors.  (The coverage tables of the hostile-memory
modules are held against the C surface by tests/test_abi_tables.py.)"""
import pytest
import torch

from hostile_memory import ALIGN, BAND, FILL, Arena, BandDamage, Recorder


def one(arena, shape=(10, 3), dtype=torch.float32, label="victim"):
    t = arena.alloc(shape, dtype, label)
    return t, arena.allocations[-1]


def test_layout_of_an_allocation():
    arena = Arena("cpu")
    for shape, dtype in (((10, 3), torch.float32), ((7,), torch.int32), ((5, 2), torch.int64), ((0, 2), torch.int32),
                         ((), torch.float32), ((1001,), torch.uint8)):
        t, a = one(arena, shape, dtype)
        assert t.shape == torch.Size(shape) and t.dtype == dtype and t.is_contiguous()
        assert a.nbytes == t.numel() * t.element_size()
        assert BAND >= 64 * 1024 and BAND % 256 == 0 and ALIGN == 256
        assert a.low().numel() == BAND and a.high().numel() == BAND
        assert a.low().data_ptr() % 256 == 0                                  # hence the payload start: BAND % 256 == 0
        assert a.low().data_ptr() + BAND == a.raw.data_ptr() + a.start      # the payload follows the low band ...
        if t.numel():
            assert t.data_ptr() == a.raw.data_ptr() + a.start and t.data_ptr() % 256 == 0
        assert a.high().data_ptr() == a.raw.data_ptr() + a.start + a.nbytes  # ... the high band its last byte, unrounded
        assert bool((a.raw == FILL).all())                                   # EVERY byte, payload included
    f = arena.alloc((4,), torch.float32)
    assert bool(torch.isnan(f).all())
    assert arena.alloc((4,), torch.int32).tolist() == [-1] * 4 and arena.alloc((2,), torch.int64).tolist() == [-1] * 2
    assert bool(torch.isnan(arena.alloc((4,), torch.bfloat16).float()).all())
    arena.check()


def test_workspace_ends_on_the_byte_asked_for_and_takes_either_fill():
    for fill in (0xFF, 0x00):
        arena = Arena("cpu", workspace_fill=fill)
        ws = arena.workspace(1000, "cpu")            # not a multiple of 256, let alone 512
        a = arena.allocations[-1]
        assert ws.dtype == torch.uint8 and ws.numel() == 1000 and a.nbytes == 1000 and bool((ws == fill).all())
        assert bool((a.low() == FILL).all()) and bool((a.high() == FILL).all())
        ws[999] = 1
        arena.check()
        assert arena.workspace(0, "cpu").numel() == 256   # as ops._workspace: never an empty buffer
        out = arena.empty((3, 4), dtype=torch.float32, device="cpu")
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(arena.empty_like(out)).all())   # results: always 0xFF
        assert arena.empty(5, dtype=torch.int32, device="cpu").shape == (5,) and arena.empty(2, 3, dtype=torch.int32, device="cpu").shape == (2, 3)


def test_untouched_arena_and_payload_writes_pass():
    arena = Arena("cpu")
    t, a = one(arena)
    t.fill_(1.0)
    p = arena.place(torch.arange(12, dtype=torch.int32).reshape(6, 2), "input")
    assert p.tolist() == torch.arange(12).reshape(6, 2).tolist()
    arena.check()
    assert arena.damage() == []


@pytest.mark.parametrize("where", ["one_past", "one_before", "far_end_high", "far_end_low"])
def test_a_single_damaged_byte_is_reported_with_label_side_and_offsets(where):
    arena = Arena("cpu")
    one(arena, (4,), torch.int32, "bystander")
    t, a = one(arena, (10, 3), torch.float32, "victim")
    one(arena, (4,), torch.int32, "another bystander")
    at, side, off = {"one_past": (a.start + a.nbytes, "high", 120), "one_before": (a.start - 1, "low", -1),
                     "far_end_high": (a.start + a.nbytes + BAND - 1, "high", 120 + BAND - 1),
                     "far_end_low": (a.start - BAND, "low", -BAND)}[where]
    a.raw[at] = 0x7F
    with pytest.raises(BandDamage) as err:
        arena.check()
    assert len(err.value.reports) == 1
    r = err.value.reports[0]
    assert (r["label"], r["side"], r["first"], r["last"], r["count"]) == ("victim", side, off, off, 1)
    assert "victim" in str(err.value) and side in str(err.value) and str(off) in str(err.value)


def test_a_damaged_range_reports_its_first_and_last_offset():
    arena = Arena("cpu")
    t, a = one(arena, (16,), torch.float32, "row")
    a.raw[a.start + a.nbytes + 8:a.start + a.nbytes + 24] = 0        # 16 bytes, starting 8 past the end
    a.raw[a.start + a.nbytes + 100] = 1
    with pytest.raises(BandDamage) as err:
        arena.check()
    (r,) = err.value.reports
    assert (r["side"], r["first"], r["last"], r["count"]) == ("high", 64 + 8, 64 + 100, 17)


def test_recorder_notes_calls_not_lookups():
    class Lib:
        def se3_a(self, x):
            return x + 1

        def se3_b(self):
            return 0

        other = 5

    rec = Recorder(Lib(), {"se3_a", "se3_b"})
    rec.se3_b                       # looked up, never called
    assert rec.se3_a(2) == 3 and rec.other == 5
    assert rec.called == {"se3_a"}



def test_the_guard_fails_on_an_unclaimed_test_an_uncalled_entry_point_a_workspace_and_a_damaged_band(built_library):
    """`guarded` is shared by the module of every header: each of its refusals, on CPU tensors and host-only entry points
    (one name of the first table, one of the last: the recorder sees every table)."""
    from types import SimpleNamespace

    from hostile_memory import guarded
    from se3conv3d_amd import _lib, ops

    real = _lib.load()
    request = SimpleNamespace(node=SimpleNamespace(originalname="test_x"))
    covered = {"se3_abi_version": ["test_x"], "se3_fps_workspace_bytes": ["test_x", "test_y"]}

    def body(workspace=False, fps=True):
        lib = _lib.load()
        assert isinstance(lib, Recorder) and lib.se3_abi_version() == _lib.ABI_VERSION
        if fps:
            assert lib.se3_fps_workspace_bytes(100, 2) > 0
        if workspace:
            assert ops._workspace(10, "cpu").numel() == 256

    with guarded(request, covered, "cpu", workspace=False):
        body()
    with guarded(request, covered, "cpu", 0x00, workspace=True, with_recorder=True) as (arena, rec):
        body(workspace=True)
        assert rec is _lib._lib and arena.workspace_fill == 0x00 and len(arena.allocations) == 1
    assert _lib._lib is real and ops._workspace(10, "cpu").numel() == 256      # everything put back
    with pytest.raises(AssertionError, match=r"claimed but not called: \['se3_fps_workspace_bytes'\]"):
        with guarded(request, covered, "cpu"):
            body(fps=False)
    with pytest.raises(AssertionError, match="test_x is not in COVERED"):
        with guarded(request, {"se3_abi_version": ["test_y"]}, "cpu"):
            body()
    with pytest.raises(AssertionError):
        with guarded(request, covered, "cpu", workspace=True):
            body()
    with pytest.raises(AssertionError):
        with guarded(request, covered, "cpu", workspace=False):
            body(workspace=True)
    with pytest.raises(BandDamage):
        with guarded(request, covered, "cpu") as arena:
            body()
            _, a = one(arena, (4,), torch.int32)
            a.raw[a.start + a.nbytes] = 0
    assert _lib._lib is real
