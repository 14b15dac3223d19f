"""CPU: the entry points of include/se3conv_padded_rows.h (batch norm, skip connection, frame pooling and the level pooling /
up-sampling on feature tensors of padded clouds): their host-side argument checks answer before any launch
(tests/test_abi_tables.py holds the header against its table, the library and its hostile-memory module).  No kernel runs here."""
import ctypes as C

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


def test_host_side_argument_checks(built_library):
    """Every refusal below is decided on the host, before the first launch: there is no GPU here, and the non-null
    pointers are not addresses of anything."""
    from se3conv3d_amd import _lib

    lib = _lib.load()
    null, p = C.c_void_p(0), C.c_void_p(16)
    big = 1 << 62
    two31 = 1 << 31

    def shapes(call):
        """The refusals every glue entry point shares: row count, frames, channels, 2^31 rows."""
        assert call(n=-1) == INVALID and call(f=0) == INVALID and call(c=0) == INVALID and call(c=1025) == INVALID
        assert call(c=258) == UNSUPPORTED and call(c=1023) == UNSUPPORTED
        assert call(n=two31) == UNSUPPORTED and call(n=two31 // 2, f=2) == UNSUPPORTED
        assert call(n=(two31 + 2) // 3, f=3) == UNSUPPORTED

    def bn_fwd(x=p, n=100, f=2, c=64, y=p, mean=p, invstd=p, ws=p, ws_bytes=big):
        return lib.se3_bn_fwd_padded(x, p, p, n, f, p, c, 1e-5, 0.2, p, p, p, y, mean, invstd, ws, ws_bytes, null)

    shapes(bn_fwd)
    assert bn_fwd(x=null) == INVALID and bn_fwd(y=null) == INVALID and bn_fwd(mean=null) == INVALID
    assert bn_fwd(invstd=null) == INVALID and bn_fwd(ws=null) == INVALID
    need = lib.se3_glue_workspace_bytes(64)
    assert need > 0 and bn_fwd(ws_bytes=need - 1) == WORKSPACE and bn_fwd(ws_bytes=0) == WORKSPACE

    def bn_bwd(dy=p, x=p, mean=p, invstd=p, n=100, f=2, c=64, dx=p, dgamma=p, dbeta=p, ws=p, ws_bytes=big):
        return lib.se3_bn_bwd_padded(dy, x, mean, invstd, p, n, f, p, c, dx, dgamma, dbeta, ws, ws_bytes, null)

    shapes(bn_bwd)
    for k in ("dy", "x", "mean", "invstd", "dx", "dgamma", "dbeta", "ws"):
        assert bn_bwd(**{k: null}) == INVALID, k
    assert bn_bwd(ws_bytes=need - 1) == WORKSPACE

    def skip_fwd(x=p, y=p, gamma=p, gate=p, rb=p, n=100, f=2, c=64, out=p):
        return lib.se3_skip_fwd_padded(x, y, gamma, gate, 0.8, rb, n, f, p, c, out, null)

    shapes(skip_fwd)
    for k in ("x", "y", "gamma", "out", "rb"):
        assert skip_fwd(**{k: null}) == INVALID, k

    def skip_bwd(g=p, x=p, gamma=p, gate=p, rb=p, n=100, f=2, c=64, dx=p, dgamma=p, ws=p, ws_bytes=big):
        return lib.se3_skip_bwd_padded(g, x, gamma, gate, 0.0, rb, n, f, p, c, dx, dgamma, ws, ws_bytes, null)

    shapes(skip_bwd)
    for k in ("g", "x", "gamma", "rb", "dgamma", "ws"):
        assert skip_bwd(**{k: null}) == INVALID, k
    assert skip_bwd(ws_bytes=need - 1) == WORKSPACE and skip_bwd(ws_bytes=0) == WORKSPACE

    def sums(x=p, n=100, f=2, c=64, out=p, ws=p, ws_bytes=big):
        return lib.se3_channel_sums_padded(x, n, f, p, c, out, ws, ws_bytes, null)

    shapes(sums)
    assert sums(x=null) == INVALID and sums(out=null) == INVALID and sums(ws=null) == INVALID
    assert sums(ws_bytes=need - 1) == WORKSPACE and sums(ws_bytes=0) == WORKSPACE

    def fpool(x=p, n=100, f=2, c=64, mode=0, out=p, arg=p):
        return lib.se3_frame_pool_padded(x, n, f, p, c, mode, out, arg, null)

    assert fpool(n=-1) == INVALID and fpool(f=0) == INVALID and fpool(c=0) == INVALID
    assert fpool(mode=-1) == INVALID and fpool(mode=4) == INVALID
    assert fpool(x=null) == INVALID and fpool(out=null) == INVALID and fpool(mode=1, arg=null) == INVALID
    assert fpool(mode=2, arg=null) == INVALID
    assert fpool(n=two31) == UNSUPPORTED and fpool(n=two31 // 2, f=2) == UNSUPPORTED

    def funpool(g=p, arg=p, n=100, f=2, c=64, mode=0, gx=p):
        return lib.se3_frame_unpool_padded(g, arg, n, f, p, c, mode, gx, null)

    assert funpool(n=-1) == INVALID and funpool(f=0) == INVALID and funpool(c=0) == INVALID
    assert funpool(mode=-1) == INVALID and funpool(mode=4) == INVALID
    assert funpool(g=null) == INVALID and funpool(gx=null) == INVALID and funpool(mode=1, arg=null) == INVALID
    assert funpool(n=two31) == UNSUPPORTED and funpool(n=two31 // 2, f=2) == UNSUPPORTED

    def unpool(vals=p, ids=p, ends=p, arg=p, n=100, c=64, mode=0, out=p):
        return lib.se3_segment_unpool_padded(vals, ids, ends, arg, n, c, mode, out, null)

    assert unpool(n=-1) == INVALID and unpool(c=0) == INVALID and unpool(mode=-1) == INVALID and unpool(mode=4) == INVALID
    assert unpool(vals=null) == INVALID and unpool(ids=null) == INVALID and unpool(out=null) == INVALID
    assert unpool(ends=null) == INVALID and unpool(mode=1, arg=null) == INVALID and unpool(mode=2, arg=null) == INVALID
    assert unpool(n=two31) == UNSUPPORTED

    def gather(src=p, idx=p, n=100, rb=256, out=p):
        return lib.se3_rows_gather_padded(src, idx, n, rb, out, null)

    assert gather(n=-1) == INVALID and gather(rb=0) == INVALID
    assert gather(src=null) == INVALID and gather(idx=null) == INVALID and gather(out=null) == INVALID
    assert gather(n=two31) == UNSUPPORTED

    def unpick(src=p, ids=p, picked=p, n=100, rb=256, out=p):
        return lib.se3_rows_unpick_padded(src, ids, picked, n, rb, out, null)

    assert unpick(n=-1) == INVALID and unpick(rb=0) == INVALID
    for k in ("src", "ids", "picked", "out"):
        assert unpick(**{k: null}) == INVALID, k
    assert unpick(n=two31) == UNSUPPORTED
    assert b"workspace" in lib.se3_error_string(WORKSPACE)

