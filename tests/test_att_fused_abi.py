"""CPU: include/se3conv_att_fused.h against its ctypes table, the built library and its hostile-memory module -- the five checks
of tests/abi_tables.py (a to e), in the manner of tests/test_basis_att_abi.py.  The header stands in the third registry,
`_lib.EXTENSION_TABLES` (asserted: that it is IN it, never where); every test places it into `_lib.TABLES` and
`abi_tables.HEADERS` for its own duration, runs the checks that every other header gets, and the registries are as they were
afterwards."""
import ctypes as C
import os
import re

import pytest

import abi_tables as T
from se3conv3d_amd import _lib, build

HEADER = "se3conv_att_fused.h"
NAMES = ("se3_att_fused_bwd", "se3_att_fused_fwd", "se3_att_fused_workspace_bytes")
PIN = T.Header("test_gpu_att_fused_hostile_memory", {"se3_att_fused_workspace_bytes"}, NAMES)


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.ATT_FUSED_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_third_registry_holds_the_header():
    assert _lib.EXTENSION_TABLES[HEADER] is _lib.ATT_FUSED_SIGNATURES
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert os.path.join(T.INCLUDE, HEADER) in [os.path.abspath(p) for p in build.EXTENSION_HEADERS]
    assert all(os.path.exists(p) for p in build.EXTENSION_HEADERS)
    assert "att_fused.hip" in build.SOURCES and build.SOURCES.index("att_fused.hip") < build.SOURCES.index("api.hip")
    assert os.path.exists(os.path.join(build.CSRC, "att_fused.hip"))
    assert sorted(_lib.ATT_FUSED_SIGNATURES) == list(NAMES)
    assert sorted(_lib.BASIS_ATT_SIGNATURES) == ["se3_basis_att_bwd", "se3_basis_att_fwd", "se3_basis_att_workspace_bytes"]  # untouched


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_att_fused_workspace_bytes": 5, "se3_att_fused_fwd": 13, "se3_att_fused_bwd": 21}


def test_b_no_name_stands_in_any_two_tables(placed, monkeypatch):
    T.check_tables_are_disjoint()
    for header, table in list(_lib.ADDED_TABLES.items()) + [(h, t) for h, t in _lib.EXTENSION_TABLES.items() if h != placed]:
        monkeypatch.setitem(_lib.TABLES, header, table)
    T.check_tables_are_disjoint()


def test_c_library_exports_and_types_the_entry_points_inside_abi_version_6(built_library, placed):
    T.check_library_exports_and_types(placed, built_library)


def test_d_argument_counts_are_those_of_the_header(placed):
    T.check_argument_counts(placed)


def test_e_every_entry_point_with_a_device_pointer_is_covered_on_hostile_memory(placed):
    T.check_hostile_memory_coverage(placed)
    assert set(T.guard_module(placed).COVERED) == set(NAMES) - {"se3_att_fused_workspace_bytes"}


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.ATT_FUSED_SIGNATURES["se3_att_fused_bwd"]
    monkeypatch.setitem(_lib.ATT_FUSED_SIGNATURES, "se3_att_fused_bwd", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_att_fused_bwd \(20 in the table, 21 in the header\)"):
        T.check_argument_counts(placed)
    monkeypatch.setitem(_lib.ATT_FUSED_SIGNATURES, "se3_att_fused_bwd", (res, args))
    monkeypatch.setitem(T.HEADERS, HEADER, T.Header(PIN.guard, set(), NAMES))            # the query no longer host-only
    with pytest.raises(AssertionError, match="not covered on hostile memory: \\['se3_att_fused_workspace_bytes'\\]"):
        T.check_hostile_memory_coverage(placed)


def test_the_constants_of_the_header_are_those_of_the_binding_and_the_restatement():
    import att_fused_reference as R

    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert define("SE3_ATT_FUSED_CHUNK") == _lib.ATT_FUSED_CHUNK == R.CHUNK and R.CHUNK % 64 == 0
    assert define("SE3_ATT_FUSED_SLAB") == _lib.ATT_FUSED_SLAB == R.SLAB == 64
    assert R.MAX_BASIS == _lib.BASIS_ATT_MAX_BASIS == 64 and "SE3_BASIS_ATT_MAX_BASIS" in text   # the cap is se3conv_basis_att.h's


def workspace(n, e, v, h, k):
    """The header's formula: a and dc [E,H] and ds [N,K,H] as fp32, each rounded up to 16 bytes, then 8 bytes per (chunk, k, i)."""
    up = lambda b: (b + 15) // 16 * 16
    chunks = max((n + _lib.ATT_FUSED_CHUNK - 1) // _lib.ATT_FUSED_CHUNK, 1)
    return 2 * up(4 * e * h) + up(4 * n * k * h) + 8 * chunks * k * v


def test_the_workspace_query_follows_the_header_and_refuses_what_the_calls_refuse(built_library):
    q = _lib.load().se3_att_fused_workspace_bytes
    for n, e, v, h, k in ((65536, 65536 * 32, 64, 4, 32), (1, 1, 6, 3, 5), (_lib.ATT_FUSED_CHUNK, 7, 8, 2, 8), (_lib.ATT_FUSED_CHUNK + 1, 7, 8, 2, 8),
                          (37, 0, 12, 2, 8), (0, 0, 8, 2, 8), (3, 5, 9, 9, 3)):
        assert q(n, e, v, h, k) == workspace(n, e, v, h, k), (n, e, v, h, k)
    assert q(0, 0, 8, 2, 8) == 8 * 8 * 8 and q(3, 5, 9, 9, 3) == 2 * 192 + 336 + 8 * 27
    refused = [q(-1, 0, 8, 2, 8), q(10, -1, 8, 2, 8), q(0, 1, 8, 2, 8), q(10, 5, 0, 1, 8), q(10, 5, 8, 0, 8), q(10, 5, 8, 3, 8), q(10, 5, 8, 2, 0),
               q(10, 5, 8, 2, _lib.BASIS_ATT_MAX_BASIS + 1), q(1 << 24, 5, 64, 64, 2), q(1 << 25, 5, 64, 1, 1), q(10, 1 << 26, 8, 2, 32),
               q(10, 1 << 26, 64, 32, 8), q(1 << 30, 1 << 30, 1, 1, 1), q(1, 1, 1 << 26, 1, 32)]
    assert refused == [0] * len(refused)


def test_the_calls_refuse_on_the_host(built_library):
    """Every refusal is made before a launch, so null pointers show it without a GPU."""
    lib = _lib.load()
    fwd = lambda n, e, v, h, k: lib.se3_att_fused_fwd(None, None, None, None, None, n, e, v, h, k, None, None, None)
    bwd = lambda n, e, v, h, k, ws=0: lib.se3_att_fused_bwd(*([None] * 10), n, e, v, h, k, None, None, None, None, ws, None)
    for call in (fwd, bwd):
        assert [call(-1, 0, 8, 2, 8), call(10, -1, 8, 2, 8), call(0, 1, 8, 2, 8), call(10, 5, 0, 1, 8), call(10, 5, 8, 0, 8), call(10, 5, 8, 3, 8),
                call(10, 5, 8, 2, 0)] == [-1] * 7, "invalid arguments"
        assert [call(10, 5, 8, 2, 65), call(1 << 24, 5, 64, 64, 2), call(1 << 25, 5, 64, 1, 1), call(10, 1 << 26, 8, 2, 32),
                call(10, 1 << 26, 64, 32, 8), call(1 << 30, 1 << 30, 1, 1, 1), call(1, 1, 1 << 26, 1, 32)] == [-2] * 7, "unsupported sizes"
        assert call(10, 5, 8, 2, 8) == -1 and call(10, 0, 8, 2, 8) == -1 and call(0, 0, 8, 2, 8) == -1, "NULL pe even without a row"
    # the pointers one class at a time: real host memory stands in for them, the calls refuse before they would touch any of it
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.se3_att_fused_fwd(None, None, p, None, None, 0, 0, 8, 2, 8, None, None, None) == 0, "no row: pe alone is required"
    assert lib.se3_att_fused_fwd(None, p, p, None, p, 10, 5, 8, 2, 8, p, p, None) == -1, "edges without phi and neighbors"
    assert lib.se3_att_fused_fwd(p, None, p, p, p, 10, 5, 8, 2, 8, p, p, None) == -1, "rows without x"
    need = lib.se3_att_fused_workspace_bytes(10, 3, 2, 1, 4)
    assert need == workspace(10, 3, 2, 1, 4) == 2 * 16 + 160 + 4 * 2 * 8
    full = [p] * 10 + [10, 3, 2, 1, 4, p, p, p, p]
    assert lib.se3_att_fused_bwd(*full, need - 1, None) == -3
    assert lib.se3_att_fused_bwd(*([p] * 7 + [None, p, p]), 10, 3, 2, 1, 4, p, p, p, p, need, None) == -1, "edges without t_samples"
    assert lib.se3_att_fused_bwd(*([p] * 10), 10, 3, 2, 1, 4, p, p, None, p, need, None) == -1, "no dpe"
    assert lib.se3_att_fused_bwd(*([p] * 10), 10, 3, 2, 1, 4, p, p, p, None, need, None) == -1, "no workspace"


def test_registries_are_as_they_were_afterwards(built_library):
    assert HEADER not in _lib.TABLES and HEADER not in T.HEADERS and HEADER in _lib.EXTENSION_TABLES
    assert list(_lib.EXTENSION_TABLES)[-1] == "se3conv_pne.h"
    assert sorted(_lib.ATT_FUSED_SIGNATURES) == list(NAMES)
    lib = _lib.load()
    assert lib.se3_att_fused_workspace_bytes.restype == C.c_size_t and lib.se3_att_fused_fwd.argtypes[5] == C.c_int64
