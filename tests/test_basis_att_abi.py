"""CPU: include/se3conv_basis_att.h against its ctypes table, the built library and its hostile-memory module -- the five checks
of tests/abi_tables.py (a to e), in the manner of tests/test_group_norm_abi.py.  The header stands in the third registry,
`_lib.EXTENSION_TABLES` (asserted: that it is IN it, never where); every test places it into `_lib.TABLES` and
`abi_tables.HEADERS` for its own duration, runs the checks that every other header gets, and the registries are as they were
afterwards."""
import ctypes as C
import os
import re

import pytest

import abi_tables as T
from se3conv3d_amd import _lib, build

HEADER = "se3conv_basis_att.h"
NAMES = ("se3_basis_att_bwd", "se3_basis_att_fwd", "se3_basis_att_workspace_bytes")
PIN = T.Header("test_gpu_basis_att_hostile_memory", {"se3_basis_att_workspace_bytes"}, NAMES)


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.BASIS_ATT_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_third_registry_holds_the_header():
    assert _lib.EXTENSION_TABLES[HEADER] is _lib.BASIS_ATT_SIGNATURES
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert os.path.join(T.INCLUDE, HEADER) in [os.path.abspath(p) for p in build.EXTENSION_HEADERS]
    assert all(os.path.exists(p) for p in build.EXTENSION_HEADERS)
    assert "basis_att.hip" in build.SOURCES and build.SOURCES.index("basis_att.hip") < build.SOURCES.index("api.hip")
    assert os.path.exists(os.path.join(build.CSRC, "basis_att.hip"))
    assert sorted(_lib.BASIS_ATT_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_basis_att_workspace_bytes": 4, "se3_basis_att_fwd": 11, "se3_basis_att_bwd": 16}


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
    assert set(T.guard_module(placed).COVERED) == set(NAMES) - {"se3_basis_att_workspace_bytes"}


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.BASIS_ATT_SIGNATURES["se3_basis_att_bwd"]
    monkeypatch.setitem(_lib.BASIS_ATT_SIGNATURES, "se3_basis_att_bwd", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_basis_att_bwd \(15 in the table, 16 in the header\)"):
        T.check_argument_counts(placed)
    monkeypatch.setitem(_lib.BASIS_ATT_SIGNATURES, "se3_basis_att_bwd", (res, args))
    monkeypatch.setitem(T.HEADERS, HEADER, T.Header(PIN.guard, set(), NAMES))            # the query no longer host-only
    with pytest.raises(AssertionError, match="not covered on hostile memory: \\['se3_basis_att_workspace_bytes'\\]"):
        T.check_hostile_memory_coverage(placed)


def test_the_constants_of_the_header_are_those_of_the_binding_and_the_restatement():
    import basis_att_reference as R

    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert define("SE3_BASIS_ATT_CHUNK") == _lib.BASIS_ATT_CHUNK == R.CHUNK and R.CHUNK % 64 == 0
    assert define("SE3_BASIS_ATT_MAX_BASIS") == _lib.BASIS_ATT_MAX_BASIS == R.MAX_BASIS == 64


def test_the_workspace_query_is_eight_bytes_per_chunk_k_i_and_refuses_what_the_calls_refuse(built_library):
    q = _lib.load().se3_basis_att_workspace_bytes
    chunks = lambda n: max((n + _lib.BASIS_ATT_CHUNK - 1) // _lib.BASIS_ATT_CHUNK, 1)
    for n, v, h, k in ((5000, 64, 4, 32), (1, 6, 3, 5), (_lib.BASIS_ATT_CHUNK, 8, 2, 8), (_lib.BASIS_ATT_CHUNK + 1, 8, 2, 8), (0, 8, 2, 8)):
        assert q(n, v, h, k) == chunks(n) * k * v * 8
    refused = [q(-1, 8, 2, 8), q(10, 0, 1, 8), q(10, 8, 0, 8), q(10, 8, 3, 8), q(10, 8, 2, 0), q(10, 8, 2, _lib.BASIS_ATT_MAX_BASIS + 1),
               q(1 << 22, 8, 2, 64), q(1 << 24, 64, 64, 2), q(1, 1 << 26, 1, 32)]
    assert refused == [0] * len(refused)


def test_the_calls_refuse_on_the_host(built_library):
    """Every refusal is made before a launch, so null pointers show it without a GPU."""
    lib = _lib.load()
    fwd = lambda n, v, h, k, stride: lib.se3_basis_att_fwd(None, None, stride, None, n, v, h, k, None, None, None)
    bwd = lambda n, v, h, k, stride, ws=0: lib.se3_basis_att_bwd(None, None, None, stride, None, None, n, v, h, k, None, None, None,
                                                                 None, ws, None)
    for call in (fwd, bwd):
        assert [call(-1, 8, 2, 8, 8), call(10, 0, 1, 8, 8), call(10, 8, 0, 8, 8), call(10, 8, 3, 8, 8), call(10, 8, 2, 0, 8),
                call(10, 8, 2, 8, 7), call(10, 8, 2, 8, -1)] == [-1] * 7, "invalid arguments"
        assert [call(10, 8, 2, 65, 8), call(1 << 22, 8, 2, 64, 8), call(1 << 24, 64, 64, 2, 64), call(1 << 20, 8, 2, 8, 1 << 11),
                call(1, 1 << 26, 1, 32, 1 << 26)] == [-2] * 5, "unsupported sizes"
        assert call(10, 8, 2, 8, 8) == -1 and call(0, 8, 2, 8, 8) == -1, "NULL pe (and dpe, the workspace) even without a row"
    # the workspace: real host memory stands in for the pointers, the call refuses before it would touch any of it
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    need = lib.se3_basis_att_workspace_bytes(10, 2, 1, 4)
    assert need == 4 * 2 * 8
    assert lib.se3_basis_att_bwd(p, p, p, 2, p, p, 10, 2, 1, 4, p, p, p, p, need - 1, None) == -3


def test_registries_are_as_they_were_afterwards(built_library):
    assert HEADER not in _lib.TABLES and HEADER not in T.HEADERS and HEADER in _lib.EXTENSION_TABLES
    assert sorted(_lib.BASIS_ATT_SIGNATURES) == list(NAMES)
    lib = _lib.load()
    assert lib.se3_basis_att_workspace_bytes.restype == C.c_size_t and lib.se3_basis_att_fwd.argtypes[2] == C.c_int64
