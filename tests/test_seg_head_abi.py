"""CPU: include/se3conv_seg_head.h against its ctypes table, the built library and its hostile-memory module -- the five checks
of tests/abi_tables.py (a to e), in the manner of tests/test_group_norm_abi.py.  The header stands in the third registry,
`_lib.EXTENSION_TABLES`; every test places it into `_lib.TABLES` and `abi_tables.HEADERS` for its own duration, runs the
checks that every other header gets, and the registries are as they were afterwards.  Nothing here says what the third
registry EQUALS: the next header is one more entry of it."""
import ctypes as C
import os

import pytest

import abi_tables as T
from se3conv3d_amd import _lib, build

HEADER = "se3conv_seg_head.h"
NAMES = ("se3_seg_head_workspace_bytes", "se3_seg_loss_bwd", "se3_seg_loss_fwd")
PIN = T.Header("test_gpu_seg_head_hostile_memory", {"se3_seg_head_workspace_bytes"}, NAMES)


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.SEG_HEAD_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_third_registry_holds_the_header_and_the_pinned_ones_do_not():
    assert _lib.EXTENSION_TABLES[HEADER] is _lib.SEG_HEAD_SIGNATURES
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert HEADER in [os.path.basename(p) for p in build.EXTENSION_HEADERS] and all(os.path.exists(p) for p in build.EXTENSION_HEADERS)
    assert "seg_head.hip" in build.SOURCES and build.SOURCES.index("seg_head.hip") < build.SOURCES.index("api.hip")
    assert os.path.exists(os.path.join(build.CSRC, "seg_head.hip"))
    assert sorted(_lib.SEG_HEAD_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_seg_head_workspace_bytes": 2, "se3_seg_loss_fwd": 15, "se3_seg_loss_bwd": 13}


def test_the_constants_are_those_of_the_header():
    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    assert f"#define SE3_SEG_HEAD_CHUNK {_lib.SEG_HEAD_CHUNK} " in text
    assert f"#define SE3_SEG_HEAD_TILE_CLASSES {_lib.SEG_HEAD_TILE_CLASSES}\n" in text
    import seg_head_reference as R

    assert (R.CHUNK, R.TILE_CLASSES) == (_lib.SEG_HEAD_CHUNK, _lib.SEG_HEAD_TILE_CLASSES)


def test_b_no_name_stands_in_any_two_tables(placed, monkeypatch):
    T.check_tables_are_disjoint()
    # ... nor in a table of the second registry, nor in another of the third
    for header, table in list(_lib.ADDED_TABLES.items()) + [(h, t) for h, t in _lib.EXTENSION_TABLES.items() if h != placed]:
        monkeypatch.setitem(_lib.TABLES, header, table)
    T.check_tables_are_disjoint()


def test_c_library_exports_and_types_the_entry_points_inside_abi_version_6(built_library, placed):
    T.check_library_exports_and_types(placed, built_library)


def test_d_argument_counts_are_those_of_the_header(placed):
    T.check_argument_counts(placed)


def test_e_every_entry_point_with_a_device_pointer_is_covered_on_hostile_memory(placed):
    T.check_hostile_memory_coverage(placed)
    G = T.guard_module(placed)
    assert set(G.COVERED) == {"se3_seg_loss_fwd", "se3_seg_loss_bwd"}


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.SEG_HEAD_SIGNATURES["se3_seg_loss_bwd"]
    monkeypatch.setitem(_lib.SEG_HEAD_SIGNATURES, "se3_seg_loss_bwd", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_seg_loss_bwd \(12 in the table, 13 in the header\)"):
        T.check_argument_counts(placed)
    monkeypatch.setitem(_lib.SEG_HEAD_SIGNATURES, "se3_seg_loss_twice", (C.c_int, []))
    with pytest.raises(AssertionError, match=r"only in the table \['se3_seg_loss_twice'\]"):
        T.check_header_and_table_agree(placed)
    monkeypatch.delitem(_lib.SEG_HEAD_SIGNATURES, "se3_seg_loss_twice")
    monkeypatch.setitem(_lib.SEG_HEAD_SIGNATURES, "se3_seg_loss_bwd", (res, args))
    monkeypatch.setitem(T.HEADERS, HEADER, T.Header(PIN.guard, set(), NAMES))            # the query no longer host-only
    with pytest.raises(AssertionError, match="not covered on hostile memory: \\['se3_seg_head_workspace_bytes'\\]"):
        T.check_hostile_memory_coverage(placed)


def test_an_older_build_without_the_entry_points_is_named(built_library, monkeypatch):
    """`_lib.load()` binds the third registry with the same message as the first two."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SEG_HEAD_SIGNATURES, "se3_seg_loss_not_built", (C.c_int, []))
    with pytest.raises(_lib.Se3LibraryError, match="does not export se3_seg_loss_not_built: it was built from older sources"):
        _lib.load()


def test_the_workspace_query_refuses_what_the_calls_refuse(built_library):
    q = _lib.load().se3_seg_head_workspace_bytes
    assert q(300, 21) >= 2 * (8 + 4 + 3 * 21 * 4) and q(0, 21) > 0 and q(1, 1) > 0 and q(1 << 20, 1024) > 0
    assert q(99000, 21) >= 387 * (8 + 4 + 3 * 21 * 4)
    assert [q(-1, 21), q(300, 0), q(300, -3), q(300, 1025), q(1 << 31, 1), q((1 << 31) // 21 + 1, 21), q(1 << 21, 1024)] == [0] * 7
    assert q((1 << 31) // 21, 21) > 0                                    # n_rows * classes just below 2^31: the last shape taken


def test_registries_are_as_they_were_afterwards(built_library):
    assert HEADER not in _lib.TABLES and HEADER not in T.HEADERS and HEADER in _lib.EXTENSION_TABLES
    assert not set(_lib.ADDED_TABLES) & set(_lib.TABLES)
    assert sorted(_lib.SEG_HEAD_SIGNATURES) == list(NAMES)
    lib = _lib.load()
    assert lib.se3_seg_head_workspace_bytes.restype == C.c_size_t and lib.se3_seg_loss_fwd.argtypes[4] == C.c_int64
