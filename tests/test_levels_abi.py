"""CPU: the entry points of include/se3conv_levels.h (a chain of grid sub-sampling levels with device-side sizes): the struct
layout, the workspace query, and host-side argument checks that answer before any launch (tests/test_abi_tables.py holds the
header against its table and the library).  No kernel runs here."""
import ctypes as C


def _levels(n_levels=2, capacity=64, cell=0.5, rnd=False, ptr=16):
    from se3conv3d_amd import _lib

    arr = (_lib.Se3Level * n_levels)()
    for lv in arr:
        lv.cell_size, lv.capacity = cell, capacity
        lv.cell_ids = lv.sorted_ids = lv.cell_ends = lv.pts = lv.batch_ids = ptr
        if rnd:
            lv.u = lv.ids = lv.picked = ptr
    return arr


def test_struct_layout_is_that_of_the_header():
    from se3conv3d_amd import _lib

    # float, (padding), int64, eight pointers: 4 + 4 + 8 + 8 * 8 on the LP64 targets the library is built for
    assert C.sizeof(_lib.Se3Level) == 80 and _lib.Se3Level.capacity.offset == 8 and _lib.Se3Level.cell_ids.offset == 16
    assert [f[0] for f in _lib.Se3Level._fields_] == ["cell_size", "capacity", "cell_ids", "sorted_ids", "cell_ends", "pts",
                                                     "batch_ids", "u", "ids", "picked"]


def test_host_side_argument_checks(built_library):
    """Every refusal below is decided on the host, before the first launch: there is no GPU here, and the non-null
    pointers are not addresses of anything."""
    from se3conv3d_amd import _lib

    lib = _lib.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    null, p = C.c_void_p(0), C.c_void_p(16)
    big = 1 << 62

    def call(pts=p, bid=p, n=100, n_valid=null, nb=1, levels=None, n_levels=2, info=p, ws=p, ws_bytes=big):
        levels = _levels() if levels is None else levels
        return lib.se3_grid_levels(pts, bid, n, n_valid, nb, levels, n_levels, info, ws, ws_bytes, null)

    assert call(pts=null) == INVALID and call(bid=null) == INVALID
    assert call(info=null) == INVALID and call(ws=null) == INVALID
    assert call(levels=C.POINTER(_lib.Se3Level)()) == INVALID
    assert call(n=-1) == INVALID and call(nb=0) == INVALID and call(n_levels=0) == INVALID
    assert call(levels=_levels(cell=0.0)) == INVALID and call(levels=_levels(cell=-1.0)) == INVALID
    assert call(levels=_levels(capacity=0)) == INVALID
    for name in ("cell_ids", "sorted_ids", "cell_ends", "pts", "batch_ids"):
        bad = _levels()
        setattr(bad[1], name, None)
        assert call(levels=bad) == INVALID, name
    for name in ("u", "ids", "picked"):        # the random form takes all three or none
        bad = _levels(rnd=True)
        setattr(bad[0], name, None)
        assert call(levels=bad) == INVALID, name
    limit = (1 << 31) // 3
    assert call(n=limit) == UNSUPPORTED and call(levels=_levels(capacity=limit)) == UNSUPPORTED
    need = lib.se3_grid_levels_workspace_bytes(100, 1, _levels(), 2)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert b"workspace" in lib.se3_error_string(WORKSPACE)


def test_workspace_query_is_monotone_and_covers_the_widest_level(built_library):
    from se3conv3d_amd import _lib

    lib = _lib.load()
    sizes = [lib.se3_grid_levels_workspace_bytes(n, 3, _levels(capacity=1), 2) for n in (0, 1, 300, 4097, 70000, 1 << 21)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    # one region for the largest input of the chain: level 1 reads capacity[0] rows, the last capacity is never an input
    one = lambda n, caps: lib.se3_grid_levels_workspace_bytes(n, 1, _levels_with(caps), len(caps))
    assert one(100, [5000, 7]) == one(5000, [7, 7]) == lib.se3_grid_subsample_workspace_bytes(5000, 1)
    assert one(100, [7, 5000]) == lib.se3_grid_subsample_workspace_bytes(100, 1)
    assert lib.se3_grid_levels_workspace_bytes(100, 0, _levels(), 2) == 0      # invalid arguments: no size


def _levels_with(capacities):
    arr = _levels(len(capacities))
    for lv, cap in zip(arr, capacities):
        lv.capacity = cap
    return arr
