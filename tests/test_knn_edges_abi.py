"""CPU: include/se3conv_knn_edges.h against its ctypes table, the built library and its hostile-memory module -- the five
checks of tests/abi_tables.py (a to e).  The header stands in the second registry, `_lib.ADDED_TABLES` (tests/test_abi_tables.py
pins `_lib.TABLES` to the seven headers before it); every test places it into `_lib.TABLES` and `abi_tables.HEADERS` for its
own duration, runs the checks that every other header gets, and the registries are as they were afterwards."""
import ctypes as C
import os

import pytest

import abi_tables as T
from se3conv3d_amd import _lib, build

HEADER = "se3conv_knn_edges.h"
NAMES = ("se3_knn_edges_bounded", "se3_knn_edges_workspace_bytes", "se3_knn_query_pair_padded")
PIN = T.Header("test_gpu_knn_edges_hostile_memory", {"se3_knn_edges_workspace_bytes"}, NAMES)


@pytest.fixture
def placed(monkeypatch):
    monkeypatch.setitem(_lib.TABLES, HEADER, _lib.KNN_EDGES_SIGNATURES)
    monkeypatch.setitem(T.HEADERS, HEADER, PIN)
    return HEADER


def test_second_registry_holds_the_header_and_the_pinned_one_does_not():
    assert list(_lib.ADDED_TABLES) == [HEADER] and _lib.ADDED_TABLES[HEADER] is _lib.KNN_EDGES_SIGNATURES
    assert HEADER not in _lib.TABLES and len(_lib.TABLES) == 7 and len(build.HEADERS) == 9
    assert [os.path.basename(p) for p in build.ADDED_HEADERS] == [HEADER] and all(os.path.exists(p) for p in build.ADDED_HEADERS)
    assert "knn_edges.hip" in build.SOURCES
    assert sorted(_lib.KNN_EDGES_SIGNATURES) == list(NAMES)


def test_a_header_and_table_agree(placed):
    T.check_header_and_table_agree(placed)
    assert T.declared(placed) == {"se3_knn_query_pair_padded": 11, "se3_knn_edges_workspace_bytes": 1, "se3_knn_edges_bounded": 11}


def test_b_no_name_stands_in_two_tables(placed):
    T.check_tables_are_disjoint()
    assert len(_lib.TABLES) == 8
    assert not set(_lib.KNN_EDGES_SIGNATURES) & {n for h, t in _lib.TABLES.items() if h != placed for n in t}


def test_c_library_exports_and_types_the_entry_points_inside_abi_version_6(built_library, placed):
    T.check_library_exports_and_types(placed, built_library)


def test_d_argument_counts_are_those_of_the_header(placed):
    T.check_argument_counts(placed)


def test_e_every_entry_point_with_a_device_pointer_is_covered_on_hostile_memory(placed):
    T.check_hostile_memory_coverage(placed)
    G = T.guard_module(placed)
    assert set(G.COVERED) == {"se3_knn_query_pair_padded", "se3_knn_edges_bounded"}


def test_the_checks_can_fail_for_this_header(placed, monkeypatch):
    res, args = _lib.KNN_EDGES_SIGNATURES["se3_knn_edges_bounded"]
    monkeypatch.setitem(_lib.KNN_EDGES_SIGNATURES, "se3_knn_edges_bounded", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_knn_edges_bounded \(10 in the table, 11 in the header\)"):
        T.check_argument_counts(placed)
    monkeypatch.setitem(_lib.KNN_EDGES_SIGNATURES, "se3_knn_edges_twice", (C.c_int, []))
    with pytest.raises(AssertionError, match=r"only in the table \['se3_knn_edges_twice'\]"):
        T.check_header_and_table_agree(placed)


def test_an_older_build_without_the_added_entry_points_is_named(built_library, monkeypatch):
    """`_lib.load()` binds the second registry with the same message as the first."""
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.KNN_EDGES_SIGNATURES, "se3_knn_edges_not_built", (C.c_int, []))
    with pytest.raises(_lib.Se3LibraryError, match="does not export se3_knn_edges_not_built: it was built from older sources"):
        _lib.load()


def test_registries_are_as_they_were_afterwards():
    assert len(_lib.TABLES) == 7 and HEADER not in _lib.TABLES and HEADER not in T.HEADERS and len(T.HEADERS) == 7
    assert sorted(_lib.KNN_EDGES_SIGNATURES) == list(NAMES)
    lib = _lib.load()
    assert lib.se3_knn_edges_workspace_bytes.restype == C.c_size_t and lib.se3_knn_edges_bounded.argtypes[1] == C.c_int64
