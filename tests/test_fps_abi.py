"""CPU: the entry points of include/se3conv_fps.h (farthest-point sampling): the resident limit, the workspace query and
host-side argument checks that answer before any launch (tests/test_abi_tables.py holds the header against its table and the
library).  No kernel runs here."""
import ctypes as C
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "se3conv_fps.h")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_resident_limit_is_the_headers():
    from se3conv3d_amd import _lib

    (value,) = re.findall(r"^#define\s+SE3_FPS_RESIDENT_MAX\s+(\d+)\s*$", header_text(), flags=re.M)
    assert _lib.FPS_RESIDENT_MAX == int(value) and int(value) % 1024 == 0


def test_host_side_argument_checks(built_library):
    """Every refusal below is decided on the host, before the first launch: there is no GPU here, and the non-null
    pointers are not addresses of anything."""
    from se3conv3d_amd import _lib

    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    null, p = C.c_void_p(0), C.c_void_p(16)
    big = 1 << 62

    def call(pts=p, bid=p, n=100, n_valid=null, nb=2, ratio=0.25, u=null, cap=100, ids=p, d2=p, starts=p, info=p, ws=p,
             ws_bytes=big):
        return lib.se3_fps(pts, bid, n, n_valid, nb, ratio, u, cap, ids, d2, starts, info, ws, ws_bytes, null)

    assert call(pts=null) == INVALID and call(bid=null) == INVALID
    assert call(ids=null) == INVALID and call(starts=null) == INVALID and call(info=null) == INVALID
    assert call(ws=null) == INVALID
    for ratio in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        assert call(ratio=ratio) == INVALID, ratio
    assert call(cap=-1) == INVALID and call(n=-1) == INVALID and call(nb=0) == INVALID
    assert call(n=1 << 31) == UNSUPPORTED and call(cap=1 << 31) == UNSUPPORTED
    need = lib.se3_fps_workspace_bytes(100, 2)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert b"workspace" in lib.se3_error_string(WORKSPACE)


def test_workspace_query(built_library):
    from se3conv3d_amd import _lib

    lib = _lib.load()
    sizes = [lib.se3_fps_workspace_bytes(n, 3) for n in (0, 1, 300, 8192, 8193, 150000, (1 << 31) - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert sizes[5] >= 4 * 150000 + 4 * 4                      # one fp32 word per row and the element boundaries
    assert lib.se3_fps_workspace_bytes(100, 1) <= lib.se3_fps_workspace_bytes(100, 1000)
    assert lib.se3_fps_workspace_bytes(100, 0) == 0 and lib.se3_fps_workspace_bytes(-1, 1) == 0   # invalid: no size
    assert lib.se3_fps_workspace_bytes(1 << 31, 1) == 0
