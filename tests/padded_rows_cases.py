"""Helpers of tests/test_gpu_padded_rows*.py (a helper module like padded_cases.py, not a conftest): raw ctypes calls of the
entry points of include/se3conv_padded_rows.h and of their counterparts in include/se3conv.h through one signature each, so
that a padded call and the call on the trimmed arrays are written once; feature tensors whose absent rows are filled in the
two hostile ways of padded_cases.py; and the comparison of a padded result with the trimmed one."""
import ctypes as C

import torch

from padded_cases import DEV, FILLS, same_bits, split_sizes

F32, I32, I64 = torch.float32, torch.int32, torch.int64
# (n_rows, valid, frames, c) -- the grid counts are those of glue_blocks (csrc/glue.hip) for n_rows * frames and valid * frames:
# 47 launched / 28 live; the scalar path, 9 / 6; one vector column, 3 / 2; idle threads and an odd frame count; the launched
# grid at the cap of 1024 with 513 live; a small one
CASES = [(3000, 1777, 2, 64), (3000, 1777, 2, 3), (3000, 1777, 2, 4), (1000, 593, 3, 260), (9000, 4100, 1, 1024), (400, 300, 4, 32)]
INT_PAD = 0x7fffffff


def glue_blocks(rows, c):
    """csrc/glue.hip: the grid of a glue kernel over `rows` rows (what the word must reproduce on the device)."""
    vec = 4 if c % 4 == 0 and c // 4 <= 256 else 1
    rpb = 256 // (c // vec)
    return min(max(((rows + rpb - 1) // rpb + 7) // 8, 1), 1024)


def counts_of(n_rows, valid):
    """The (word value or None, present points) pairs every case runs: the case's own count, none, one, all, a word past
    the buffer (clamped) and no word at all."""
    return [(valid, valid), (0, 0), (1, 1), (n_rows, n_rows), (n_rows + 5, n_rows), (None, n_rows)]


def word_of(value):
    return None if value is None else torch.tensor([value], dtype=I32, device=DEV)


def rows_with_pad(present, total, fill, seed):
    """`present` [P, C] float rows (CPU) in front of a [total, C] buffer: NaN behind them, or copies of present rows (random
    rows when there is none to copy)."""
    p = present.shape[0]
    out = torch.full((total,) + tuple(present.shape[1:]), float("nan"))
    if fill == "copies" and total > p:
        g = torch.Generator().manual_seed(2000 + seed)
        out[p:] = present[torch.randint(0, p, (total - p,), generator=g)] if p else torch.randn((total - p,) + tuple(present.shape[1:]), generator=g)
    else:
        assert fill in FILLS
    out[:p] = present
    return out.contiguous()


def ids_with_pad(present, total, fill, seed):
    """int32 ids the same way: 0x7fffffff behind the present ones, or copies of present ids (zeros when there is none)."""
    p = present.shape[0]
    out = torch.full((total,), INT_PAD, dtype=I32)
    if fill == "copies" and total > p:
        g = torch.Generator().manual_seed(3000 + seed)
        out[p:] = present[torch.randint(0, p, (total - p,), generator=g)] if p else 0
    out[:p] = present
    return out.contiguous()


def row_batch_ids(points, frames, batches=3, empty=1):
    """Batch ids of `points` points over `batches` elements, one of them empty, repeated per frame."""
    sizes = split_sizes(points, batches, empty)
    bid = torch.repeat_interleave(torch.arange(batches, dtype=I32), torch.tensor(sizes))
    return bid.repeat_interleave(frames).to(I32).contiguous()


class Plain:
    """Outputs and workspaces from the ordinary allocator, pre-filled so that an unwritten byte shows: NaN floats, 0x7f7f7f7f
    integers (neither 0 nor -1), 0xFF workspace bytes."""

    def out(self, shape, dtype):
        if dtype == F32:
            return torch.full(shape, float("nan"), dtype=F32, device=DEV)
        t = torch.empty(shape, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(0x7f)
        return t

    def ws(self, nbytes):
        return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=DEV)


class FromArena:
    """The same from a hostile_memory.Arena: 0xFF everywhere, guard bands, the workspace sized exactly."""

    def __init__(self, arena):
        self.arena = arena

    def out(self, shape, dtype):
        return self.arena.alloc(shape, dtype)

    def ws(self, nbytes):
        return self.arena.workspace(nbytes, DEV)


def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    from se3conv3d_amd import ops
    return ops._stream(torch.device(DEV))


def _ok(rc, what):
    assert rc == 0, (what, rc)


# Each caller: `pad = None` runs the entry point of se3conv.h on the tensors as they are; `pad = (n_rows, frames, word)` runs
# the padded form (word: int32 device tensor or None).
def bn_fwd(lib, A, x, w, b, rm, rv, nbt, pad=None, eps=1e-5, momentum=0.2):
    rows, c = x.shape
    y, mean, invstd = A.out((rows, c), F32), A.out((c,), F32), A.out((c,), F32)
    need = lib.se3_glue_workspace_bytes(c)
    ws = A.ws(need)
    if pad is None:
        _ok(lib.se3_bn_fwd(_p(x), _p(w), _p(b), rows, c, eps, momentum, _p(rm), _p(rv), _p(nbt), _p(y), _p(mean), _p(invstd),
                           _p(ws), need, _stream()), "se3_bn_fwd")
    else:
        _ok(lib.se3_bn_fwd_padded(_p(x), _p(w), _p(b), pad[0], pad[1], _p(pad[2]), c, eps, momentum, _p(rm), _p(rv), _p(nbt),
                                  _p(y), _p(mean), _p(invstd), _p(ws), need, _stream()), "se3_bn_fwd_padded")
    return y, mean, invstd


def bn_bwd(lib, A, dy, x, mean, invstd, gamma, pad=None):
    rows, c = x.shape
    dx, dgamma, dbeta = A.out((rows, c), F32), A.out((c,), F32), A.out((c,), F32)
    need = lib.se3_glue_workspace_bytes(c)
    ws = A.ws(need)
    if pad is None:
        _ok(lib.se3_bn_bwd(_p(dy), _p(x), _p(mean), _p(invstd), _p(gamma), rows, c, _p(dx), _p(dgamma), _p(dbeta), _p(ws), need,
                           _stream()), "se3_bn_bwd")
    else:
        _ok(lib.se3_bn_bwd_padded(_p(dy), _p(x), _p(mean), _p(invstd), _p(gamma), pad[0], pad[1], _p(pad[2]), c, _p(dx),
                                  _p(dgamma), _p(dbeta), _p(ws), need, _stream()), "se3_bn_bwd_padded")
    return dx, dgamma, dbeta


def skip_fwd(lib, A, x, y, gamma, gate, keep, row_batch, pad=None):
    rows, c = x.shape
    out = A.out((rows, c), F32)
    if pad is None:
        _ok(lib.se3_skip_fwd(_p(x), _p(y), _p(gamma), _p(gate), keep, _p(row_batch), rows, c, _p(out), _stream()), "se3_skip_fwd")
    else:
        _ok(lib.se3_skip_fwd_padded(_p(x), _p(y), _p(gamma), _p(gate), keep, _p(row_batch), pad[0], pad[1], _p(pad[2]), c,
                                    _p(out), _stream()), "se3_skip_fwd_padded")
    return out


def skip_bwd(lib, A, g, x, gamma, gate, keep, row_batch, pad=None, want_dx=True):
    rows, c = x.shape
    dx = A.out((rows, c), F32) if want_dx else None
    dgamma = A.out((c,), F32)
    need = lib.se3_glue_workspace_bytes(c)
    ws = A.ws(need)
    if pad is None:
        _ok(lib.se3_skip_bwd(_p(g), _p(x), _p(gamma), _p(gate), keep, _p(row_batch), rows, c, _p(dx), _p(dgamma), _p(ws), need,
                             _stream()), "se3_skip_bwd")
    else:
        _ok(lib.se3_skip_bwd_padded(_p(g), _p(x), _p(gamma), _p(gate), keep, _p(row_batch), pad[0], pad[1], _p(pad[2]), c,
                                    _p(dx), _p(dgamma), _p(ws), need, _stream()), "se3_skip_bwd_padded")
    return dx, dgamma


def channel_sums(lib, A, x, pad):
    c = x.shape[1]
    out = A.out((c,), F32)
    need = lib.se3_glue_workspace_bytes(c)
    ws = A.ws(need)
    _ok(lib.se3_channel_sums_padded(_p(x), pad[0], pad[1], _p(pad[2]), c, _p(out), _p(ws), need, _stream()), "se3_channel_sums_padded")
    return out


def frame_pool(lib, A, x, frames, mode, word=None, padded=False):
    n, c = x.shape[0] // frames, x.shape[1]
    out = A.out((n, c), F32)
    arg = A.out((n, c), I32) if mode in (1, 2) else None
    if not padded:
        _ok(lib.se3_frame_pool(_p(x), n, frames, c, mode, _p(out), _p(arg), _stream()), "se3_frame_pool")
    else:
        _ok(lib.se3_frame_pool_padded(_p(x), n, frames, _p(word), c, mode, _p(out), _p(arg), _stream()), "se3_frame_pool_padded")
    return out, arg


def frame_unpool(lib, A, g, arg, frames, mode, word=None, padded=False):
    n, c = g.shape
    gx = A.out((n * frames, c), F32)
    if not padded:
        _ok(lib.se3_frame_unpool(_p(g), _p(arg), n, frames, c, mode, _p(gx), _stream()), "se3_frame_unpool")
    else:
        _ok(lib.se3_frame_unpool_padded(_p(g), _p(arg), n, frames, _p(word), c, mode, _p(gx), _stream()),
            "se3_frame_unpool_padded")
    return gx


def segment_pool(lib, A, src, sorted_ids, cell_ends, n_cells, mode):
    c = src.shape[1]
    out = A.out((n_cells, c), F32)
    arg = A.out((n_cells, c), I32) if mode in (1, 2) else None
    _ok(lib.se3_segment_pool(_p(src), _p(sorted_ids), _p(cell_ends), n_cells, c, mode, _p(out), _p(arg), _stream()),
        "se3_segment_pool")
    return out, arg


def segment_unpool(lib, A, vals, cell_ids, cell_ends, arg, mode, padded=False):
    n, c = cell_ids.shape[0], vals.shape[1]
    out = A.out((n, c), F32)
    fn = lib.se3_segment_unpool_padded if padded else lib.se3_segment_unpool
    _ok(fn(_p(vals), _p(cell_ids), _p(cell_ends), _p(arg), n, c, mode, _p(out), _stream()), "se3_segment_unpool")
    return out


def rows_gather_padded(lib, A, src, idx):
    out = A.out((idx.shape[0],) + tuple(src.shape[1:]), src.dtype)
    _ok(lib.se3_rows_gather_padded(_p(src), _p(idx), idx.shape[0], src[0].numel() * src.element_size(), _p(out), _stream()),
        "se3_rows_gather_padded")
    return out


def rows_unpick_padded(lib, A, src, cell_ids, picked):
    out = A.out((cell_ids.shape[0],) + tuple(src.shape[1:]), src.dtype)
    _ok(lib.se3_rows_unpick_padded(_p(src), _p(cell_ids), _p(picked), cell_ids.shape[0], src[0].numel() * src.element_size(),
                                   _p(out), _stream()), "se3_rows_unpick_padded")
    return out


def zero_bits(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def assert_rows(got, want, present, what):
    """A row-shaped output of a padded call: the present rows are those of the trimmed call bit for bit, the absent rows are
    +0.0f by their bits."""
    assert got.shape[0] >= present and want.shape[0] == present, what
    assert same_bits(got[:present], want), what
    assert zero_bits(got[present:]), what
