"""CPU: the entry points of include/se3conv_padded.h (boxes, ball query, self-k-NN and PCA frames of padded clouds, row counts
in device words): their host-side argument checks answer before any launch (tests/test_abi_tables.py holds the header
against its table, the library and its hostile-memory module).  No kernel runs here."""
import ctypes as C

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_host_side_argument_checks(built_library):
    """Every refusal below is decided on the host, before the first launch: there is no GPU here, and the non-null
    pointers are not addresses of anything."""
    from se3conv3d_amd import _lib

    lib = _lib.load()
    null, p = C.c_void_p(0), C.c_void_p(16)
    big = 1 << 62

    def aabb(pts=p, bid=p, n=100, nv=p, nb=1, mn=p, mx=p):
        return lib.se3_batch_aabb_padded(pts, bid, n, nv, nb, mn, mx, null)

    assert aabb(pts=null) == INVALID and aabb(bid=null) == INVALID and aabb(mn=null) == INVALID and aabb(mx=null) == INVALID
    assert aabb(n=-1) == INVALID and aabb(nb=0) == INVALID

    def bq(ps=p, pd=p, bs=p, bd=p, mn=p, nc=p, r=0.1, n_src=5000, n_dst=100, nb=1, grid=null, grid_bytes=0, ws=p, ws_bytes=big,
           cap=10, nbrs=p, ends=p, info=p):
        return lib.se3_ball_query_padded(ps, pd, bs, bd, mn, nc, r, n_src, n_dst, p, p, nb, grid, grid_bytes, 0, ws, ws_bytes, cap,
                                         nbrs, null, ends, info, null)

    assert bq(info=null) == INVALID and bq(ends=null) == INVALID and bq(ws=null) == INVALID
    assert bq(ps=null) == INVALID and bq(pd=null) == INVALID and bq(bs=null) == INVALID and bq(bd=null) == INVALID
    assert bq(mn=null) == INVALID and bq(nc=null) == INVALID          # 5000 sources: the grid path needs its parameters
    assert bq(n_src=-1) == INVALID and bq(n_dst=-1) == INVALID and bq(cap=-1) == INVALID and bq(nb=0) == INVALID
    assert bq(r=0.0) == INVALID and bq(r=-1.0) == INVALID and bq(nbrs=null) == INVALID
    assert bq(cap=1 << 31) == INVALID and bq(cap=(1 << 31) - 1, ws_bytes=0) == WORKSPACE      # (the last capacity that is taken)
    assert bq(n_src=1 << 31) == UNSUPPORTED and bq(n_dst=(1 << 31) // 9) == UNSUPPORTED
    need = lib.se3_ball_query_padded_workspace_bytes(5000, 100)
    assert need == lib.se3_ball_query_workspace_bytes(5000, 100) > 0
    assert bq(ws_bytes=need - 1) == WORKSPACE and bq(ws_bytes=0) == WORKSPACE
    assert bq(grid=p, grid_bytes=lib.se3_ball_query_grid_bytes(5000) - 1) == WORKSPACE

    def params(bid=p, n=100, bmn=p, bmx=p, nb=1, k=16, factor=1.6, mn=p, nc=p, cs=p):
        return lib.se3_knn_grid_params_padded(bid, n, p, bmn, bmx, nb, k, factor, mn, nc, cs, null)

    assert params(bid=null) == INVALID and params(bmn=null) == INVALID and params(bmx=null) == INVALID
    assert params(mn=null) == INVALID and params(nc=null) == INVALID and params(cs=null) == INVALID
    assert params(n=-1) == INVALID and params(nb=0) == INVALID and params(k=0) == INVALID and params(factor=0.0) == INVALID

    def knn(pts=p, bid=p, n=100, mn=p, nc=p, cs=p, k=16, out=p, ws=p, ws_bytes=big):
        return lib.se3_knn_query_padded(pts, bid, n, p, mn, nc, cs, k, out, ws, ws_bytes, null)

    assert knn(pts=null) == INVALID and knn(bid=null) == INVALID and knn(out=null) == INVALID and knn(ws=null) == INVALID
    assert knn(n=-1) == INVALID and knn(k=0) == INVALID
    assert knn(mn=null) == INVALID and knn(nc=null) == INVALID and knn(cs=null) == INVALID      # all three or none
    assert knn(k=65) == UNSUPPORTED and knn(k=65, mn=null, nc=null, cs=null) == UNSUPPORTED
    assert knn(k=33) == UNSUPPORTED and knn(n=1 << 31) == UNSUPPORTED
    need = lib.se3_knn_query_padded_workspace_bytes(100, 1)
    assert need == lib.se3_knn_query_grid_workspace_bytes(100) > 0 and lib.se3_knn_query_padded_workspace_bytes(100, 0) == 0
    assert knn(ws_bytes=need - 1) == WORKSPACE and knn(ws_bytes=0) == WORKSPACE

    def pca(pts=p, ids=p, n=100, k=16, axis=-1, frames=p):
        return lib.se3_pca_frames_padded(pts, ids, n, p, k, axis, frames, null)

    assert pca(pts=null) == INVALID and pca(ids=null) == INVALID and pca(frames=null) == INVALID
    assert pca(n=-1) == INVALID and pca(k=0) == INVALID and pca(axis=3) == INVALID
    assert pca(axis=0) == UNSUPPORTED and pca(n=1 << 31) == UNSUPPORTED
    assert b"workspace" in lib.se3_error_string(WORKSPACE)

