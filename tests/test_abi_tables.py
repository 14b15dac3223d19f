"""CPU: every header of `_lib.TABLES` against its ctypes table, the built library and its hostile-memory module -- the checks
of tests/abi_tables.py, one case per header each -- and the faults every check must catch, planted one at a time.  No
compute entry point is called here."""
import ctypes as C

import pytest

import abi_tables as T
from se3conv3d_amd import _lib

HEADERS = list(_lib.TABLES)


def test_registries_name_the_same_headers_in_the_order_they_were_added():
    assert HEADERS == list(T.HEADERS) == ["se3conv.h", "se3conv_capped.h", "se3conv_levels.h", "se3conv_forms.h",
                                          "se3conv_padded.h", "se3conv_padded_rows.h", "se3conv_fps.h"]
    assert [_lib.TABLES[h] is t for h, t in zip(HEADERS, (
        _lib.SIGNATURES, _lib.CAPPED_SIGNATURES, _lib.LEVEL_SIGNATURES, _lib.FORMS_SIGNATURES, _lib.PADDED_SIGNATURES,
        _lib.PADDED_ROWS_SIGNATURES, _lib.FPS_SIGNATURES))] == [True] * 7
    from se3conv3d_amd import build
    assert [p.split("/include/")[-1] for p in build.HEADERS[2:]] == HEADERS and len(build.HEADERS) == 9


@pytest.mark.parametrize("header", HEADERS)
def test_header_and_table_agree(header):
    T.check_header_and_table_agree(header)


@pytest.mark.parametrize("header", HEADERS)
def test_table_stays_apart_from_the_other_tables(header):
    T.check_tables_are_disjoint()       # over all tables, whichever header is asked about
    assert not set(_lib.TABLES[header]) & {n for h, t in _lib.TABLES.items() if h != header for n in t}


@pytest.mark.parametrize("header", HEADERS)
def test_library_exports_and_types_the_entry_points_inside_abi_version_6(built_library, header):
    T.check_library_exports_and_types(header, built_library)


@pytest.mark.parametrize("header", HEADERS)
def test_argument_counts_are_those_of_the_header(header):
    T.check_argument_counts(header)


@pytest.mark.parametrize("header", HEADERS)
def test_every_entry_point_with_a_device_pointer_is_covered_on_hostile_memory(header):
    T.check_hostile_memory_coverage(header)


def test_partition_of_the_main_header_is_the_pinned_one():
    """se3conv.h: its module's COVERED and HOST_ONLY do not overlap, and the exemption is for entry points without a device
    buffer and for nothing else."""
    import test_gpu_hostile_memory as G

    names = set(_lib.SIGNATURES)
    assert set(G.COVERED) | G.HOST_ONLY == names and not set(G.COVERED) & G.HOST_ONLY
    assert len(G.COVERED) == 39 and len(G.HOST_ONLY) == 19
    assert G.HOST_ONLY == ({"se3_abi_version", "se3_error_string", "se3conv_intermediate_bytes_per_element",
                            "se3conv_intermediate_row_bytes", "se3_ball_query_needs_grid", "se3conv_bwd_needs_t",
                            "se3_ball_query_grid_bytes"}
                           | {n for n in names if n.endswith("_workspace_bytes")} | {n for n in names if n.startswith("se3_profile_")})


def test_declared_counts_void_as_no_argument_and_skips_comments():
    d = T.declared("se3conv.h")
    assert d["se3_abi_version"] == 0 and d["se3_profile_reset"] == 0 and d["se3_error_string"] == 1
    assert d["se3conv_fwd"] == 18 and len(d) == 58 and sum(len(T.declared(h)) for h in HEADERS) == 82


# ------------------------------------------------------------------------------ planted faults: every check can fail, by name
def test_a_name_in_a_table_but_not_in_the_header_is_named(monkeypatch):
    monkeypatch.setitem(_lib.CAPPED_SIGNATURES, "se3_ball_query_capped_twice", (C.c_int, []))
    with pytest.raises(AssertionError, match=r"only in the table \['se3_ball_query_capped_twice'\]"):
        T.check_header_and_table_agree("se3conv_capped.h")
    T.check_header_and_table_agree("se3conv_levels.h")


def test_a_name_in_two_tables_is_named(monkeypatch):
    monkeypatch.setitem(_lib.FPS_SIGNATURES, "se3_grid_levels", _lib.LEVEL_SIGNATURES["se3_grid_levels"])
    with pytest.raises(AssertionError, match=r"se3_grid_levels \(se3conv_levels.h and se3conv_fps.h\)"):
        T.check_tables_are_disjoint()


def test_a_table_entry_with_one_argument_too_few_is_named(monkeypatch):
    res, args = _lib.PADDED_SIGNATURES["se3_pca_frames_padded"]
    monkeypatch.setitem(_lib.PADDED_SIGNATURES, "se3_pca_frames_padded", (res, args[:-1]))
    with pytest.raises(AssertionError, match=r"se3_pca_frames_padded \(7 in the table, 8 in the header\)"):
        T.check_argument_counts("se3conv_padded.h")
    monkeypatch.setitem(_lib.SIGNATURES, "se3_abi_version", (C.c_int, [C.c_int]))     # and one too many against (void)
    with pytest.raises(AssertionError, match=r"se3_abi_version \(1 in the table, 0 in the header\)"):
        T.check_argument_counts("se3conv.h")


def test_a_wrong_restype_is_named(built_library, monkeypatch):
    _lib.load()                                                                 # bound from the true table
    monkeypatch.setitem(_lib.SIGNATURES, "se3_error_string", (C.c_int, [C.c_int]))
    with pytest.raises(AssertionError, match=r"table of se3conv.h: \['se3_error_string'\]"):
        T.check_library_exports_and_types("se3conv.h", built_library)
    res, args = _lib.FPS_SIGNATURES["se3_fps"]
    monkeypatch.setitem(_lib.FPS_SIGNATURES, "se3_fps", (res, args[:-1] + [C.c_int]))   # ... and a wrong argument type
    with pytest.raises(AssertionError, match=r"table of se3conv_fps.h: \['se3_fps'\]"):
        T.check_library_exports_and_types("se3conv_fps.h", built_library)


@pytest.mark.parametrize("header,name", [("se3conv.h", "se3_knn_query_pair"), ("se3conv_levels.h", "se3_grid_levels"),
                                         ("se3conv_fps.h", "se3_fps")])
def test_a_pointer_taking_name_dropped_from_covered_is_named(monkeypatch, header, name):
    monkeypatch.delitem(T.guard_module(header).COVERED, name)
    with pytest.raises(AssertionError, match=rf"not covered on hostile memory: \['{name}'\]"):
        T.check_hostile_memory_coverage(header)


def test_a_claimed_test_that_does_not_exist_is_named(monkeypatch):
    G = T.guard_module("se3conv_padded_rows.h")
    monkeypatch.setitem(G.COVERED, "se3_bn_fwd_padded", ["test_batch_norm_and_skip_connection", "test_that_is_not_there"])
    with pytest.raises(AssertionError, match="se3_bn_fwd_padded: test_gpu_padded_rows_hostile_memory has no test_that_is_not_there"):
        T.check_hostile_memory_coverage("se3conv_padded_rows.h")
    monkeypatch.setitem(G.COVERED, "se3_bn_fwd_padded", [])
    with pytest.raises(AssertionError, match="se3_bn_fwd_padded: no test claimed"):
        T.check_hostile_memory_coverage("se3conv_padded_rows.h")


def test_a_host_only_name_with_a_device_pointer_is_named(monkeypatch):
    monkeypatch.setitem(T.HEADERS, "se3conv_fps.h", T.Header("test_gpu_fps_hostile_memory", {"se3_fps_workspace_bytes", "se3_fps"}))
    with pytest.raises(AssertionError, match="se3_fps is host-only but takes a device pointer"):
        T.check_hostile_memory_coverage("se3conv_fps.h")
