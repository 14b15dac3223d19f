"""CPU: include/se3conv_pne.h against its ctypes table, the built library and its hostile-memory module -- the five checks of
tests/abi_tables.py (a to e), in the manner of tests/test_group_norm_abi.py.  The header stands in the third registry,
`_lib.EXTENSION_TABLES`; every test places it into `_lib.TABLES` and `abi_tables.HEADERS` for its own duration, runs the
checks that every other header gets, and the registries are as they were afterwards."""
import ctypes as C
import os
import re

import pytest

import abi_tables as T
from se3conv3d_amd import _lib, build

HEADER = "se3conv_pne.h"
NAMES = ("se3_neigh_max_bwd", "se3_neigh_max_fwd", "se3_pne_embed_bwd", "se3_pne_embed_fwd", "se3_pne_embed_workspace_bytes")
PIN = T.Header("test_gpu_pne_hostile_memory", {"se3_pne_embed_workspace_bytes"}, NAMES)


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.PNE_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_third_registry_holds_the_header_at_its_end():
    assert _lib.EXTENSION_TABLES[HEADER] is _lib.PNE_SIGNATURES and list(_lib.EXTENSION_TABLES)[-1] == HEADER
    assert HEADER not in _lib.TABLES and HEADER not in _lib.ADDED_TABLES
    assert [os.path.basename(p) for p in build.EXTENSION_HEADERS] == list(_lib.EXTENSION_TABLES)
    assert all(os.path.exists(p) for p in build.EXTENSION_HEADERS)
    assert "pne.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pne.hip"))
    assert sorted(_lib.PNE_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_pne_embed_workspace_bytes": 4, "se3_pne_embed_fwd": 14, "se3_pne_embed_bwd": 18,
                                  "se3_neigh_max_fwd": 12, "se3_neigh_max_bwd": 17}


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
    assert set(T.guard_module(placed).COVERED) == set(NAMES) - {"se3_pne_embed_workspace_bytes"}


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.PNE_SIGNATURES["se3_neigh_max_bwd"]
    monkeypatch.setitem(_lib.PNE_SIGNATURES, "se3_neigh_max_bwd", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_neigh_max_bwd \(16 in the table, 17 in the header\)"):
        T.check_argument_counts(placed)
    monkeypatch.setitem(_lib.PNE_SIGNATURES, "se3_neigh_max_bwd", (res, args))
    monkeypatch.setitem(T.HEADERS, HEADER, T.Header(PIN.guard, set(), NAMES))            # the query no longer host-only
    with pytest.raises(AssertionError, match="not covered on hostile memory: \\['se3_pne_embed_workspace_bytes'\\]"):
        T.check_hostile_memory_coverage(placed)


def test_the_constants_of_the_header_are_those_of_the_binding_and_the_restatement():
    import pne_reference as R

    text = open(os.path.join(T.INCLUDE, HEADER)).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert define("SE3_PNE_CHUNK") == _lib.PNE_CHUNK == R.CHUNK and define("SE3_PNE_MAX_KPTS") == _lib.PNE_MAX_KPTS == R.MAX_KPTS
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"SE3_PNE_(\w+) = (\d+)", text)}
    assert enum == _lib.PNE_KINDS == R.KINDS


def test_the_workspace_query_refuses_what_the_calls_refuse(built_library):
    q = _lib.load().se3_pne_embed_workspace_bytes
    gauss, relu = _lib.PNE_KINDS["kp_gauss"], _lib.PNE_KINDS["mlp_relu"]
    chunks = (5000 + _lib.PNE_CHUNK - 1) // _lib.PNE_CHUNK
    assert q(5000, gauss, 13, 32) >= chunks * 14 * 32 * 8 and q(5000, relu, 0, 16) >= chunks * 4 * 16 * 8
    assert q(5000, gauss, 55, 32) > q(5000, gauss, 13, 32) and q(0, relu, 0, 8) > 0
    refused = [q(-1, relu, 0, 8), q(10, relu, 0, 0), q(10, -1, 0, 8), q(10, 8, 13, 8), q(10, gauss, 0, 8),
               q(10, gauss, _lib.PNE_MAX_KPTS + 1, 8), q(1 << 30, relu, 0, 8), q(1 << 27, relu, 0, 16)]
    assert refused == [0] * len(refused)


def test_the_calls_refuse_on_the_host(built_library):
    """Every refusal is made before a launch, so null pointers show it without a GPU."""
    lib = _lib.load()
    relu, gauss = _lib.PNE_KINDS["mlp_relu"], _lib.PNE_KINDS["kp_gauss"]
    fwd = lambda e, kind, j, k: lib.se3_pne_embed_fwd(None, None, None, e, None, kind, None, j, 0.3, None, None, k, None, None)
    assert [fwd(-1, relu, 0, 8), fwd(10, 9, 0, 8), fwd(10, gauss, 0, 8), fwd(10, relu, 0, 8)] == [-1, -1, -1, -1]
    assert [fwd(10, gauss, 65, 8), fwd(1 << 30, relu, 0, 8)] == [-2, -2]
    mx = lambda e, m, n, k, c: lib.se3_neigh_max_fwd(None, None, None, None, e, m, n, k, c, None, None, None)
    assert [mx(10, 4, 4, 0, 8), mx(10, 4, 4, 8, 0), mx(-1, 4, 4, 8, 8), mx(10, 4, 4, 8, 8)] == [-1, -1, -1, -1]
    assert [mx(10, 4, 1 << 20, 64, 64), mx(1 << 26, 4, 4, 64, 8), mx(10, 1 << 28, 4, 8, 8)] == [-2, -2, -2]
    bw = lambda e, m, n, k, c: lib.se3_neigh_max_bwd(*([None] * 9), e, m, n, k, c, None, None, None)
    assert [bw(10, 4, 4, 0, 8), bw(10, 4, 1 << 20, 64, 64), bw(10, 4, 4, 8, 8)] == [-1, -2, -1]


def test_registries_are_as_they_were_afterwards(built_library):
    assert HEADER not in _lib.TABLES and HEADER not in T.HEADERS and HEADER in _lib.EXTENSION_TABLES
    assert sorted(_lib.PNE_SIGNATURES) == list(NAMES)
    lib = _lib.load()
    assert lib.se3_pne_embed_workspace_bytes.restype == C.c_size_t and lib.se3_neigh_max_fwd.argtypes[4] == C.c_int64
