"""The C surface header by header (a helper module like hostile_memory.py, not a conftest): what every header of
`_lib.TABLES` must satisfy, as functions that raise AssertionError with the offending names, and the per-header facts the
checks need.  tests/test_abi_tables.py runs every check over every header and plants the faults each one must catch.

A new header gets one line in HEADERS below (and one in `_lib.TABLES`); it then has every check without a copy of any."""
import ctypes as C
import importlib
import inspect
import os
import re
from dataclasses import dataclass
from typing import Optional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
ABI_VERSION = 6


@dataclass(frozen=True)
class Header:
    guard: Optional[str]            # the hostile-memory module (its COVERED: entry point -> tests) that guards the header;
    #                                 None: no entry point of the header takes a device pointer
    host_only: object               # names that take no device buffer: a set, or the name of the guard module's own set
    names: Optional[tuple] = None   # the pinned surface, sorted (None: the header grows with the library, see `must`)
    must: tuple = ()                # names the header declares whatever else it does


HEADERS = {
    "se3conv.h": Header("test_gpu_hostile_memory", "HOST_ONLY", must=(
        "se3conv_fwd", "se3conv_bwd", "se3_ball_query_count", "se3_ball_query_store", "se3_feat_basis_proj",
        "se3_feat_basis_proj_grad", "se3_compute_keys", "se3_rot_tensors", "se3_csr_transpose")),
    "se3conv_capped.h": Header("test_gpu_capped_hostile_memory", {"se3_ball_query_capped_workspace_bytes"}, (
        "se3_ball_query_capped", "se3_ball_query_capped_workspace_bytes")),
    "se3conv_levels.h": Header("test_gpu_bounded_levels_hostile_memory", {"se3_grid_levels_workspace_bytes"}, (
        "se3_grid_levels", "se3_grid_levels_workspace_bytes")),
    "se3conv_forms.h": Header(None, {"se3conv_forms"}, ("se3conv_forms",)),      # its only function takes host pointers
    "se3conv_padded.h": Header("test_gpu_padded_hostile_memory", {"se3_ball_query_padded_workspace_bytes",
                                                                  "se3_knn_query_padded_workspace_bytes"}, (
        "se3_ball_query_padded", "se3_ball_query_padded_workspace_bytes", "se3_batch_aabb_padded", "se3_knn_grid_params_padded",
        "se3_knn_query_padded", "se3_knn_query_padded_workspace_bytes", "se3_pca_frames_padded")),
    "se3conv_padded_rows.h": Header("test_gpu_padded_rows_hostile_memory", set(), (
        "se3_bn_bwd_padded", "se3_bn_fwd_padded", "se3_channel_sums_padded", "se3_frame_pool_padded", "se3_frame_unpool_padded",
        "se3_rows_gather_padded", "se3_rows_unpick_padded", "se3_segment_unpool_padded", "se3_skip_bwd_padded",
        "se3_skip_fwd_padded")),
    "se3conv_fps.h": Header("test_gpu_fps_hostile_memory", {"se3_fps_workspace_bytes"}, ("se3_fps", "se3_fps_workspace_bytes")),
}
SKIPS = ("pytest.skip", "mark.skip", "xfail")   # what a hostile-memory module may not contain: the tables allow no exemption


def tables():
    from se3conv3d_amd import _lib

    return _lib.TABLES


def header_text(header):
    """The header without its block and line comments."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def declared(header):
    """{symbol: argument count} of the functions `header` declares; `(void)` counts as no argument."""
    text = header_text(header)
    out = {}
    for name in re.findall(r"^(?:int|int64_t|size_t|const char\*)\s+(se3\w+)\s*\(", text, flags=re.M):
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1).strip()
        out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


def guard_module(header):
    guard = HEADERS[header].guard
    return importlib.import_module(guard) if guard else None


def host_only(header):
    names = HEADERS[header].host_only
    return set(getattr(guard_module(header), names) if isinstance(names, str) else names)


# ------------------------------------------------------------------------------------------------------------- the checks
def check_header_and_table_agree(header):
    """a: the table lists exactly what the header declares (and what HEADERS pins for it)."""
    got, table = sorted(declared(header)), sorted(tables()[header])
    assert got == table, (f"{header} and its table disagree: only in the table {sorted(set(table) - set(got))}, "
                          f"only in the header {sorted(set(got) - set(table))}")
    pin = HEADERS[header]
    assert pin.names is None or got == list(pin.names), f"{header}: the pinned surface is {list(pin.names)}, declared {got}"
    assert set(pin.must) <= set(got), f"{header} no longer declares {sorted(set(pin.must) - set(got))}"


def check_tables_are_disjoint():
    """b: no name stands in two tables."""
    seen, twice = {}, []
    for header, table in tables().items():
        twice += [f"{name} ({seen[name]} and {header})" for name in table if name in seen]
        seen.update(dict.fromkeys(table, header))
    assert not twice, f"names in two tables: {twice}"


def check_library_exports_and_types(header, library_path):
    """c: the library exports every name, `_lib.load()` types each as its table says, inside ABI version 6."""
    from se3conv3d_amd import _lib

    raw = C.CDLL(library_path)
    missing = [name for name in tables()[header] if not hasattr(raw, name)]
    assert not missing, f"in the table of {header} but not exported: {missing}"
    lib = _lib.load()
    wrong = [name for name, (res, args) in tables()[header].items()
             if getattr(lib, name).restype != res or list(getattr(lib, name).argtypes or []) != list(args)]
    assert not wrong, f"restype / argtypes after load() are not those of the table of {header}: {wrong}"
    in_header = int(re.search(r"#define SE3_ABI_VERSION (\d+)", open(os.path.join(INCLUDE, "se3conv.h")).read()).group(1))
    assert lib.se3_abi_version() == _lib.ABI_VERSION == ABI_VERSION == in_header   # additions stay inside the version


def check_argument_counts(header):
    """d: as many argtypes as the header's declaration has arguments."""
    counts = declared(header)
    wrong = [f"{name} ({len(args)} in the table, {counts.get(name)} in the header)"
             for name, (_, args) in tables()[header].items() if counts.get(name) != len(args)]
    assert not wrong, f"argument counts of {header}: {wrong}"


def check_hostile_memory_coverage(header):
    """e: every entry point that takes a device pointer is claimed by a test of the header's hostile-memory module that
    exists and cannot be skipped; the host-only names are exactly those without a device pointer."""
    from se3conv3d_amd import _lib

    table, host, G = tables()[header], host_only(header), guard_module(header)
    covered = G.COVERED if G is not None else {}
    assert host <= set(table), f"{header}: host-only names outside the table: {sorted(host - set(table))}"
    missing, stray = set(table) - host - set(covered), set(covered) - set(table)
    assert not missing, f"{header}: not covered on hostile memory: {sorted(missing)}"
    assert not stray, f"{header}: covered but not in the table: {sorted(stray)}"
    for name, (_, args) in table.items():
        if name in host:
            assert _lib._P not in args or name.startswith("se3_profile_"), f"{name} is host-only but takes a device pointer"  # (profile: host pointers)
        else:
            assert _lib._P in args, f"{name} takes no device pointer: it belongs to the host-only names of {header}"
    if G is None:
        return
    tests = {n for n, f in inspect.getmembers(G, inspect.isfunction) if n.startswith("test_")}
    for name, where in covered.items():
        assert where, f"{name}: no test claimed"
        for t in where:
            assert t in tests, f"{name}: {G.__name__} has no {t}"
            assert not [s for s in SKIPS if s in inspect.getsource(getattr(G, t))], f"{t} can be skipped"
    assert not [s for s in SKIPS if s in inspect.getsource(G)], f"{G.__name__} contains a skip or an expected failure"
