"""Tensor-level wrappers and autograd Functions over the C ABI (include/se3conv.h).

PyTorch is used for device memory, the current stream and autograd bookkeeping only; every
computation below runs in libse3conv_hip.so.  The class names / call signatures mirror the
reference's ``point_cloud_lib.custom_ops`` (FeatBasisProj.py, BallQuery.py, ComputeKeys.py).
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Callable, Optional, Tuple

import torch

from . import _lib
from ._lib import Se3Shape


# ------------------------------------------------------------------------------------- precision
# Arithmetic of the operator's contractions (include/se3conv.h, SE3_PRECISION_*): "bf16x3" = split-bf16
# MFMA with fp32 accumulate (~1e-5 rel. to the fp32 reference, the default), "fp32" = exact-fp32 MFMA.
import os as _os

_precision = _os.environ.get("SE3CONV_PRECISION", "bf16x3")
if _precision not in _lib.PRECISIONS:
    raise ValueError(f"SE3CONV_PRECISION={_precision!r}; expected one of {sorted(_lib.PRECISIONS)}")


def set_precision(name: str) -> None:
    global _precision
    if name not in _lib.PRECISIONS:
        raise ValueError(f"precision {name!r}; expected one of {sorted(_lib.PRECISIONS)}")
    _precision = name


def get_precision() -> str:
    return _precision


# --------------------------------------------------------------------------------------- helpers
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device) -> C.c_void_p:
    """The current HIP stream of ``device``, which must be the current device: the library launches on the stream it
    is handed and never switches devices itself, so tensors on another GPU than the current one would be launched
    on the wrong device's stream.  (The raw query: ``torch.cuda.current_stream()`` builds a Python object through
    several device-index lookups, ~20 us per call.)"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx != torch.cuda.current_device():
        raise ValueError(f"tensors live on cuda:{idx} but the current device is cuda:{torch.cuda.current_device()}: "
                         "call inside `with torch.cuda.device(tensor.device):` (one process per GPU is the intended use)")
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(idx))
    return C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)


def _ptr(t: Optional[torch.Tensor], dtype: torch.dtype, name: str, device=None) -> C.c_void_p:
    """Device pointer of a contiguous CUDA tensor of the given dtype (ValueError otherwise)."""
    if t is None:
        return C.c_void_p(0)
    # (the good case first: an eager neighbourhood build passes ~11 tensors per query and is bound by the host,
    # tools/host_split_neighbourhoods.py)
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and (device is None or t.device == device):
        return C.c_void_p(t.data_ptr())
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback), got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _as(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Contiguous copy-if-needed in ``dtype`` (what the reference wrappers do with ``.to``)."""
    if t.dtype == dtype and not t.requires_grad and t.is_contiguous():
        return t  # (nothing to convert or to detach: three tensor objects less per argument)
    return t.detach().to(dtype).contiguous()


def version_key(t: torch.Tensor):
    """What a per-cloud cache key holds for "the contents of ``t`` are still those": the tensor's version counter.  A
    tensor created under ``torch.inference_mode()`` has none (reading ``_version`` raises) and can be updated in place
    without a trace, so nothing is cached on it: its key entry is a fresh object, equal to no other, and every cache that
    carries it rebuilds -- as they do while a graph is being captured."""
    return object() if t.is_inference() else t._version


def _valid_word(n_valid, device, who: str) -> C.c_void_p:
    """The row-count word of a padded cloud (include/se3conv_padded.h): one int32 on the device, or None = every row."""
    p = _ptr(n_valid, torch.int32, "n_valid", device)
    if n_valid is not None and n_valid.numel() != 1:
        raise ValueError(f"{who}: n_valid is one int32 word on the device")
    return p


# Row-wise passes on padded clouds (include/se3conv_padded_rows.h).  A feature tensor padded like its cloud is
# [n_rows * frames, C], of which the first clamp(*n_valid) * frames rows exist.  A pass that is handed the cloud's row-count
# word never reads an absent row and leaves zeros there; it takes the tensor as it is (float32, contiguous rows, on the GPU),
# and nothing is a torch fallback.  Without a word every row exists, and the same pass converts what it is given.
def _padded_rows(t: torch.Tensor, frames: int, who: str) -> Tuple[torch.Tensor, int]:
    """``t`` as the [n_rows * frames, C] float32 matrix the library reads, and ``n_rows``."""
    t2 = _as(t, torch.float32)
    if t2.dim() != 2 or not t2.is_cuda:
        raise ValueError(f"{who}: expected [rows, C] features on the GPU (the HIP path has no CPU fallback)")
    if int(frames) < 1 or t2.shape[0] % int(frames):
        raise ValueError(f"{who}: {t2.shape[0]} rows are not a multiple of the frame count {frames}")
    return t2, t2.shape[0] // int(frames)


def _feature_rows(t: torch.Tensor, n_valid, frames: int, who: str) -> torch.Tensor:
    """``t`` as the [rows, C] float32 matrix of a glue pass; with a row-count word, the feature rows of a padded cloud under
    the checks of ``_padded_rows`` (on the GPU, whole points)."""
    if n_valid is not None:
        return _padded_rows(t, frames, who)[0]
    t2 = _as(t, torch.float32)
    if t2.dim() != 2:
        raise ValueError(f"{who}: expected [rows, C] features")
    return t2


def _row_pass(name: str, n_valid):
    """The entry point of a row-wise pass and its name: ``name`` (include/se3conv.h) without a row-count word, its ``_padded``
    form (include/se3conv_padded_rows.h) with one.  The library has one ``*_impl`` behind both, and a padded call with a null
    word launches what the ordinary call does -- but only its host side refuses ``n_rows * frames >= 2^31``, and the ordinary
    entry points are what callers without padded clouds are tested on, so such callers keep them."""
    if n_valid is not None:
        name += "_padded"
    return getattr(_lib.load(), name), name


def _glue_rows(x2: torch.Tensor, n_valid, frames: int, who: str) -> tuple:
    """The arguments of a glue pass that say which rows of ``x2`` exist: ``rows`` (every one), or ``n_rows, frames, n_valid``."""
    if n_valid is None:
        return (x2.shape[0],)
    return (x2.shape[0] // frames, frames, _valid_word(n_valid, x2.device, who))


def _padded_cloud(pts, batch_ids, who: str):
    """A padded cloud is taken as it is -- float32 [N,3] points, int32 [N] batch ids, contiguous: a conversion would read
    the absent rows (and be a launch of its own)."""
    if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{who}: only [N,3] point sets are supported")
    _ptr(pts, torch.float32, "pts")
    _ptr(batch_ids, torch.int32, "batch_ids", pts.device)
    if tuple(batch_ids.shape) != (pts.shape[0],):
        raise ValueError(f"{who}: batch_ids of shape {tuple(batch_ids.shape)} for {pts.shape[0]} points")


# every buffer the library writes -- results, saved tensors, cached operands -- is allocated through these two names and
# `_workspace` (tests/hostile_memory.py swaps all three for guard-banded, 0xFF-filled allocations)
_empty = torch.empty
_empty_like = torch.empty_like


def _workspace(nbytes: int, device) -> torch.Tensor:
    return _empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ----------------------------------------------------------------------------- grid keys (a10, f-2)
def compute_keys(pts, batch_ids, aabb_min, num_cells, cell_size) -> torch.Tensor:
    """``point_cloud_lib_ops.compute_keys`` (reference ComputeKeys.py / compute_keys.cu:75-124)."""
    lib = _lib.load()
    pts = _as(pts, torch.float32)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("compute_keys: only 3-D points are supported")
    dev = pts.device
    n = pts.shape[0]
    keys = _empty(n, dtype=torch.int64, device=dev)
    b = _as(batch_ids, torch.int32)
    mn = _as(aabb_min, torch.float32)
    nc = _as(num_cells, torch.int32).to(dev)
    cs = _as(cell_size, torch.float32).to(dev)
    _lib.check(lib.se3_compute_keys(_ptr(pts, torch.float32, "pts"), _ptr(b, torch.int32, "batch_ids", dev),
                                    _ptr(mn, torch.float32, "aabb_min", dev), _ptr(nc, torch.int32, "num_cells"),
                                    _ptr(cs, torch.float32, "cell_size"), n, _ptr(keys, torch.int64, "keys"),
                                    _stream(dev)), "se3_compute_keys")
    return keys


class ComputeKeys(torch.autograd.Function):
    """Drop-in for ``point_cloud_lib.custom_ops.ComputeKeys``."""

    @staticmethod
    def forward(ctx, p_pts, p_batch_ids, p_aabb_min, p_grid_size, p_cell_size):
        return compute_keys(p_pts, p_batch_ids, p_aabb_min, p_grid_size, p_cell_size)

    @staticmethod
    def backward(ctx, grad):
        return None, None, None, None, None


# ------------------------------------------------------------------------------- ball query (a10)
def batch_aabb(pts, batch_ids, n_batches: Optional[int] = None, n_valid: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-batch bounding boxes ``(min [B,3], max [B,3])`` (the reference's scatter_min / scatter_max calls).
    ``n_valid`` (int32 device word): a padded cloud -- only rows ``[0, n_valid)`` are present and read
    (``se3_batch_aabb_padded``); ``n_batches`` is then required."""
    lib = _lib.load()
    if n_valid is not None:
        _padded_cloud(pts, batch_ids, "batch_aabb")
        if n_batches is None:
            raise ValueError("batch_aabb: a padded cloud needs n_batches (reading it from the batch ids would be a read-back)")
        dev = pts.device
        mn = _empty((int(n_batches), 3), dtype=torch.float32, device=dev)
        mx = _empty((int(n_batches), 3), dtype=torch.float32, device=dev)
        _lib.check(lib.se3_batch_aabb_padded(_ptr(pts, torch.float32, "pts"), _ptr(batch_ids, torch.int32, "batch_ids", dev),
                                             pts.shape[0], _valid_word(n_valid, dev, "batch_aabb"), int(n_batches),
                                             _ptr(mn, torch.float32, "aabb_min"), _ptr(mx, torch.float32, "aabb_max"),
                                             _stream(dev)), "se3_batch_aabb_padded")
        return mn, mx
    pts = _as(pts, torch.float32)
    b = _as(batch_ids, torch.int32)
    if n_batches is None:
        # one tiny sync, the same one the reference pays with `torch::amax(...).item()` (ball_query.cu:46)
        n_batches = int(b.max().item()) + 1 if b.numel() else 1
    mn = _empty((n_batches, 3), dtype=torch.float32, device=pts.device)
    mx = _empty((n_batches, 3), dtype=torch.float32, device=pts.device)
    _lib.check(lib.se3_batch_aabb(_ptr(pts, torch.float32, "pts"), _ptr(b, torch.int32, "batch_ids", pts.device),
                                  pts.shape[0], n_batches, _ptr(mn, torch.float32, "aabb_min"),
                                  _ptr(mx, torch.float32, "aabb_max"), _stream(pts.device)), "se3_batch_aabb")
    return mn, mx


@functools.lru_cache(maxsize=4096)
def _ball_query_sizes(n_src: int, n_dst: int) -> Tuple[bool, int, int]:
    """(needs a cell grid, workspace bytes, grid bytes) of a query of this size: three library calls, asked once per size."""
    lib = _lib.load()
    return (bool(lib.se3_ball_query_needs_grid(n_src)), int(lib.se3_ball_query_workspace_bytes(n_src, n_dst)),
            int(lib.se3_ball_query_grid_bytes(n_src)))


def ball_query_needs_grid(n_src: int) -> bool:
    """Whether a query against ``n_src`` source points uses the cell grid (small source sets are scanned whole)."""
    return bool(_lib.load().se3_ball_query_needs_grid(int(n_src)))


def _batch_aabb_min_and_cells(pts_src, batch_src, radius: float, n_batches: Optional[int] = None, box=None):
    """Grid parameters exactly as BallQuery.forward builds them (BallQuery.py:34-38), on device, one library call.
    ``box`` = the source cloud's ``batch_aabb`` result when the caller has it (``Pointcloud.aabb()``: computed once per
    cloud, a cloud is the source of several queries per step): one tiny launch instead of a pass over the points."""
    lib = _lib.load()
    if n_batches is None:
        # one tiny sync, the same one the reference pays with `torch::amax(...).item()` (ball_query.cu:46)
        n_batches = int(batch_src.max().item()) + 1 if batch_src.numel() else 1
    dev = pts_src.device
    if box is not None and box[0].shape == (n_batches, 3) and box[0].device == dev:
        mn = _empty((n_batches, 3), dtype=torch.float32, device=dev)
        num_cells = _empty(3, dtype=torch.int32, device=dev)
        _lib.check(lib.se3_ball_query_grid_from_box(_ptr(box[0], torch.float32, "box_min", dev), _ptr(box[1], torch.float32, "box_max", dev),
                                                    n_batches, float(radius), _ptr(mn, torch.float32, "aabb_min"),
                                                    _ptr(num_cells, torch.int32, "num_cells"), _stream(dev)),
                   "se3_ball_query_grid_from_box")
        return mn, num_cells
    box = _empty((2, n_batches, 3), dtype=torch.float32, device=dev)  # [0] = shifted minimum, [1] = scratch
    num_cells = _empty(3, dtype=torch.int32, device=dev)
    _lib.check(lib.se3_ball_query_grid(
        _ptr(pts_src, torch.float32, "pts_src"), _ptr(batch_src, torch.int32, "batch_src", dev), pts_src.shape[0],
        n_batches, float(radius), C.c_void_p(box[0].data_ptr()), C.c_void_p(box[1].data_ptr()),
        _ptr(num_cells, torch.int32, "num_cells"), _stream(dev)), "se3_ball_query_grid")
    return box[0], num_cells


def ball_query(pts_src, pts_dst, batch_src, batch_dst, radius: float,
               n_batches: Optional[int] = None, src_box=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Radius neighbours: ``neighbors [E,2] int32`` (col0 sample, col1 source; grouped by sample)
    and ``ends [M] int32`` (inclusive end offsets).  Two-phase C ABI, one host sync for E."""
    lib = _lib.load()
    pts_src = _as(pts_src, torch.float32)
    pts_dst = _as(pts_dst, torch.float32)
    if pts_src.dim() != 2 or pts_src.shape[1] != 3 or pts_dst.dim() != 2 or pts_dst.shape[1] != 3:
        raise ValueError("ball_query: only [N,3] point sets are supported")
    if not (radius > 0):
        raise ValueError("ball_query: radius must be positive")
    dev = pts_src.device
    bs = _as(batch_src, torch.int32)
    bd = _as(batch_dst, torch.int32)
    n_src, n_dst = pts_src.shape[0], pts_dst.shape[0]
    if n_dst == 0 or n_src == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(n_dst, dtype=torch.int32, device=dev)
    ends = _empty(n_dst, dtype=torch.int32, device=dev)  # every entry is written by the count phase
    # small source sets are searched all-pairs by the library: no boxes / cell grid to prepare
    needs_grid, ws_bytes, _ = _ball_query_sizes(n_src, n_dst)
    mn, nc = _batch_aabb_min_and_cells(pts_src, bs, radius, n_batches, src_box) if needs_grid else (None, None)
    ws = _workspace(ws_bytes, dev)
    f32, i32 = torch.float32, torch.int32
    _lib.check(lib.se3_ball_query_count(
        _ptr(pts_src, f32, "pts_src"), _ptr(pts_dst, f32, "pts_dst", dev), _ptr(bs, i32, "batch_src", dev),
        _ptr(bd, i32, "batch_dst", dev), _ptr(mn, f32, "aabb_min"), _ptr(nc, i32, "num_cells"), float(radius),
        n_src, n_dst, C.c_void_p(ws.data_ptr()), ws.numel(), _ptr(ends, i32, "ends"), _stream(dev)),
        "se3_ball_query_count")
    n_edges = int(ends[-1].item())
    neighbors = _empty((n_edges, 2), dtype=torch.int32, device=dev)
    _lib.check(lib.se3_ball_query_store(
        _ptr(pts_dst, f32, "pts_dst"), _ptr(bd, i32, "batch_dst"), float(radius), n_src, n_dst,
        C.c_void_p(ws.data_ptr()), ws.numel(), _ptr(ends, i32, "ends"), n_edges,
        _ptr(neighbors, i32, "neighbors"), _stream(dev)), "se3_ball_query_store")
    return neighbors, ends


SHARED_GRIDS = _os.environ.get("SE3_SHARED_GRIDS", "1") != "0"  # (A/B switch, tools/time_faust_geometry.py)


class SourceGrids:
    """The cell grids of one source cloud, one per search radius (``se3_ball_query_bounded_shared``): the queries of a step
    that search the cloud with the same radius sort it once.  Kept on the cloud object (``source_grids``); a grid is
    rebuilt when the cloud's points, batch ids or batch count are no longer the ones it was built from."""

    __slots__ = ("grids", "params")

    def __init__(self):
        self.grids = {}
        self.params = {}  # per radius: (shifted box minima, cell counts) of the grid (se3_ball_query_grid_from_box)

    @staticmethod
    def key(pts, batch_ids, n_batches, n_valid=None):
        """What a grid is valid for: the cloud's OWN points and batch ids (storage and version), not converted copies -- a
        temporary's address says nothing about the cloud and may be recycled by the next temporary.  A padded cloud's grid
        is also keyed on its row-count word (storage and version: a new count is a new grid), which keeps it apart from
        the grids of the other queries."""
        key = (pts.data_ptr(), version_key(pts), batch_ids.data_ptr(), version_key(batch_ids), int(pts.shape[0]),
               int(n_batches or 0), str(pts.device))
        return key if n_valid is None else key + (n_valid.data_ptr(), version_key(n_valid))

    def slot(self, key, radius, nbytes, device):
        """``(buffer, valid)`` for this radius; ``valid`` says the buffer already holds the grid of ``key``.  A buffer
        handed out with ``False`` is the caller's to build the grid in: it is kept only once ``commit`` says the build has
        been enqueued (a call that fails in between leaves no entry that claims a grid)."""
        hit = self.grids.get(float(radius))
        if hit is not None and hit[0] == key and hit[1].numel() >= nbytes:
            return hit[1], True
        self.grids.pop(float(radius), None)
        self.params.pop(float(radius), None)
        return _empty(int(nbytes), dtype=torch.uint8, device=device), False

    def commit(self, key, radius, buf, params):
        """Keep ``buf`` as the grid of ``key`` for this radius, with its grid parameters: after the library call that
        builds it has returned."""
        if len(self.grids) >= 8 and float(radius) not in self.grids:
            # (a cloud is searched with two or three radii; a sweep over many drops the oldest)
            oldest = next(iter(self.grids))
            self.grids.pop(oldest)
            self.params.pop(oldest, None)
        self.grids[float(radius)] = (key, buf)
        self.params[float(radius)] = params


def source_grids(cloud) -> Optional["SourceGrids"]:
    """The holder of ``cloud``'s source grids, created on first use and kept on the object; None when the object takes
    no attribute."""
    holder = getattr(cloud, "_se3_grids_", None)
    if holder is None:
        holder = SourceGrids()
        try:
            cloud._se3_grids_ = holder
        except (AttributeError, TypeError):
            return None
    return holder


def forget_source_grids(cloud) -> None:
    """Drop ``cloud``'s source grids (what a new step's cloud starts without; timing loops that rebuild a step's
    neighbourhoods on the same cloud objects call it per repetition)."""
    holder = getattr(cloud, "_se3_grids_", None)
    if holder is not None:
        holder.grids.clear()
        holder.params.clear()


def _bounded_query(who, entries, pts_src, pts_dst, batch_src, batch_dst, radius, capacity, n_batches, neighbors_out, out_error,
                   src_box, grids, rows_per_sample=0, want_sources=False, want_degrees=False, workspace_bytes=None, tail=None,
                   n_valid=None):
    """What ``ball_query_bounded`` and ``ball_query_capped`` share: conversions and validation, the result buffers, the
    workspace, the source cloud's shared grid (slot, parameters, commit) and the library call itself.  ``entries``: the C
    entry point without and with the grid arguments (the first None: the second is called either way, with a NULL grid).
    ``capacity=None``: ``n_dst * rows_per_sample`` rows.  ``workspace_bytes(n_src, n_dst)``: where the call needs more
    than the bounded query.  ``tail(dev, degrees)``: checks and C arguments behind the stream.  ``n_valid = (source word,
    sample word)``: the padded call, which takes the two words behind the row counts and the clouds as they are.  Returns ``(neighbors, ends,
    info, sources, degrees)``."""
    lib = _lib.load()
    src_own, batch_own = pts_src, batch_src  # (what a source grid is keyed on: the caller's tensors, not their conversions)
    if n_valid is not None:
        _padded_cloud(pts_src, batch_src, who)
        _padded_cloud(pts_dst, batch_dst, who)
    pts_src = _as(pts_src, torch.float32)
    pts_dst = _as(pts_dst, torch.float32)
    if pts_src.dim() != 2 or pts_src.shape[1] != 3 or pts_dst.dim() != 2 or pts_dst.shape[1] != 3:
        raise ValueError("ball_query: only [N,3] point sets are supported")
    if not (radius > 0) or (capacity is not None and capacity < 0):
        raise ValueError(f"{who}: radius must be positive and capacity non-negative")
    dev = pts_src.device
    f32, i32 = torch.float32, torch.int32
    bs, bd = _as(batch_src, i32), _as(batch_dst, i32)
    n_src, n_dst = pts_src.shape[0], pts_dst.shape[0]
    rows = n_dst * rows_per_sample if capacity is None else int(capacity)
    if neighbors_out is not None:
        if capacity is None or neighbors_out.shape != (rows, 2) or neighbors_out.dtype != i32 or not neighbors_out.is_contiguous():
            raise ValueError(out_error)
        neighbors = neighbors_out
    else:
        neighbors = _empty((rows, 2), dtype=i32, device=dev)
    sources = _empty(rows, dtype=i32, device=dev) if want_sources else None
    ends = _empty(n_dst, dtype=i32, device=dev)
    degrees = _empty(n_dst, dtype=i32, device=dev) if want_degrees else None
    extra = tail(dev, degrees) if tail is not None else ()
    if n_dst == 0:
        return neighbors, ends, torch.zeros(2, dtype=i32, device=dev), sources, degrees
    info = _empty(2, dtype=i32, device=dev)  # both words are written by the store pass
    needs_grid, ws_bytes, grid_bytes = _ball_query_sizes(n_src, n_dst)
    ws = _workspace(workspace_bytes(n_src, n_dst) if workspace_bytes is not None else ws_bytes, dev)
    grid, valid, key = None, False, None
    capturing = torch.cuda.is_current_stream_capturing()
    # (a padded query also shares INSIDE a capture: the key then carries the capture's id, so only a grid built by an earlier
    # node of the same graph counts, which every replay rebuilds first)
    if grids is not None and needs_grid and src_box is not None and SHARED_GRIDS and (not capturing or n_valid is not None):
        # (src_box: the grid parameters are then a pure function of the cloud's cached boxes and the radius, so two calls
        # with the same key search the same cells -- and the parameters themselves are kept with the grid)
        key = SourceGrids.key(src_own, batch_own, n_batches, n_valid[0] if n_valid is not None else None)
        if capturing:
            key += (_capture_id(dev),)
        grid, valid = grids.slot(key, radius, grid_bytes, dev)
        params = grids.params.get(float(radius)) if valid else None
        if params is None:
            valid, params = False, _batch_aabb_min_and_cells(pts_src, bs, radius, n_batches, src_box)
        mn, nc = params
    else:
        mn, nc = _batch_aabb_min_and_cells(pts_src, bs, radius, n_batches, src_box) if needs_grid else (None, None)
    with_grid = grid is not None or entries[0] is None
    mid = (_valid_word(n_valid[0], dev, who), _valid_word(n_valid[1], dev, who)) if n_valid is not None else ()
    entry = entries[1] if with_grid else entries[0]
    grid_args = (C.c_void_p(grid.data_ptr() if grid is not None else 0), grid.numel() if grid is not None else 0,
                 int(valid)) if with_grid else ()
    _lib.check(getattr(lib, entry)(
        _ptr(pts_src, f32, "pts_src"), _ptr(pts_dst, f32, "pts_dst", dev), _ptr(bs, i32, "batch_src", dev),
        _ptr(bd, i32, "batch_dst", dev), _ptr(mn, f32, "aabb_min"), _ptr(nc, i32, "num_cells"), float(radius), n_src,
        n_dst, *mid, int(n_batches or 0), *grid_args, C.c_void_p(ws.data_ptr()), ws.numel(), rows, _ptr(neighbors, i32, "neighbors"),
        _ptr(sources, i32, "sources"), _ptr(ends, i32, "ends"), _ptr(info, i32, "info"), _stream(dev), *extra), entry)
    if grid is not None and not valid:
        grids.commit(key, radius, grid, params)
    return neighbors, ends, info, sources, degrees


def ball_query_bounded(pts_src, pts_dst, batch_src, batch_dst, radius: float, capacity: int,
                       n_batches: Optional[int] = None, want_sources: bool = False,
                       neighbors_out: Optional[torch.Tensor] = None, src_box=None, grids: Optional[SourceGrids] = None):
    """The same query without the host round trip for the edge count (``se3_ball_query_bounded``): the caller sizes the
    edge buffer (``capacity`` rows, e.g. 1.25 x the previous step's count).  Returns ``(neighbors [capacity,2] int32,
    ends [M] int32, info [2] int32 on the device)`` with ``info[0]`` = true edge count and ``info[1]`` = 1 when it did
    not fit (the list is then truncated and ``ends`` clamped: rerun with a larger buffer).  Capturable in a HIP graph
    when ``n_batches`` is given.  ``want_sources``: a fourth result, the source ids as a dense ``[capacity]`` array
    (the source-major edge list of a cloud against itself).  ``neighbors_out``: a caller-owned contiguous
    ``[capacity, 2]`` int32 buffer to write into (e.g. a slice of a larger arena) instead of a fresh allocation.
    ``grids``: the source cloud's ``SourceGrids`` -- its cell grid for this radius is then built once and shared by every
    query that passes the holder (not while a HIP graph is being captured: a replay must not depend on what ran before)."""
    neighbors, ends, info, sources, _ = _bounded_query(
        "ball_query_bounded", ("se3_ball_query_bounded", "se3_ball_query_bounded_shared"), pts_src, pts_dst, batch_src,
        batch_dst, radius, capacity, n_batches, neighbors_out, f"neighbors_out must be a contiguous int32 [{int(capacity)}, 2] tensor",
        src_box, grids, want_sources=want_sources)
    return (neighbors, ends, info, sources) if want_sources else (neighbors, ends, info)


def ball_query_padded(pts_src, pts_dst, batch_src, batch_dst, radius: float, capacity: int, n_batches: int,
                      n_valid_src: Optional[torch.Tensor] = None, n_valid_dst: Optional[torch.Tensor] = None,
                      want_sources: bool = False, neighbors_out: Optional[torch.Tensor] = None, src_box=None,
                      grids: Optional[SourceGrids] = None):
    """``ball_query_bounded`` between PADDED clouds (``se3_ball_query_padded``, include/se3conv_padded.h): only rows
    ``[0, n_valid_src)`` of the source arrays and ``[0, n_valid_dst)`` of the sample arrays are present (int32 device
    words; None = every row).  Absent rows are never read, absent sources never listed, absent samples have no edges
    (their ``ends`` are flat).  Same results as ``ball_query_bounded`` -- ``(neighbors [capacity,2], ends [rows_dst], info
    [2][, sources])`` -- and no host synchronisation: capturable, and a replay follows the words.  The clouds are taken as
    they are (float32 / int32, contiguous); ``n_batches`` is required.  ``src_box``: the source cloud's
    ``batch_aabb(..., n_valid=n_valid_src)`` when the caller has it.  ``grids``: as for ``ball_query_bounded``; a padded
    cloud's grid is kept per value of its count word, and the padded queries of ONE graph capture share it too (only a grid
    that an earlier node of the same graph builds is reused, never one from before the capture).  "Per value" is held
    through the word's storage and version counter: a word that a graph replay rewrites changes value without moving its
    version, so the clouds a captured build made must not be queried eagerly with a ``grids`` holder afterwards (build a
    fresh cloud over the buffers, or ``forget_source_grids`` first)."""
    lib = _lib.load()
    if n_batches is None or int(n_batches) < 1:
        raise ValueError("ball_query_padded: n_batches must be given (reading it from the batch ids would be a read-back)")
    if capacity is None:
        raise ValueError("ball_query_padded: needs a capacity")
    _padded_cloud(pts_src, batch_src, "ball_query_padded")
    if src_box is None and pts_src.shape[0] > 0 and pts_dst.shape[0] > 0 and ball_query_needs_grid(pts_src.shape[0]):
        src_box = batch_aabb(pts_src, batch_src, int(n_batches), n_valid_src) if n_valid_src is not None else \
            batch_aabb(pts_src, batch_src, int(n_batches))
    neighbors, ends, info, sources, _ = _bounded_query(
        "ball_query_padded", (None, "se3_ball_query_padded"), pts_src, pts_dst, batch_src, batch_dst, radius, capacity,
        int(n_batches), neighbors_out, f"neighbors_out must be a contiguous int32 [{int(capacity)}, 2] tensor", src_box, grids,
        want_sources=want_sources, workspace_bytes=lib.se3_ball_query_padded_workspace_bytes,
        n_valid=(n_valid_src, n_valid_dst))
    return (neighbors, ends, info, sources) if want_sources else (neighbors, ends, info)


MAX_CAPPED_NEIGHBORS = 64  # se3_ball_query_capped keeps one key per lane of a wavefront (include/se3conv_capped.h)


def draw_seed() -> int:
    """A 32-bit seed from torch's default CPU generator (reproducible under ``torch.manual_seed``; no device work)."""
    return int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())


def ball_query_capped(pts_src, pts_dst, batch_src, batch_dst, radius: float, max_neighbors: int, seed: int,
                      capacity: Optional[int] = None, n_batches: Optional[int] = None, want_degrees: bool = False,
                      neighbors_out: Optional[torch.Tensor] = None, src_box=None, grids: Optional[SourceGrids] = None,
                      seed_tensor: Optional[torch.Tensor] = None):
    """Radius neighbours with at most ``max_neighbors`` sources per sample (``se3_ball_query_capped``): a sample with more
    hits keeps the ``max_neighbors`` of them with the smallest keys ``hash(seed, sample, source)`` -- a uniform subset that
    depends on the seed, the sample and its hit SET only, in the order the uncapped query lists them (the contract is in
    include/se3conv_capped.h).  ``max_neighbors <= 0``: no limit.

    ``capacity=None``: builds into ``n_dst * max_neighbors`` rows (which cannot overflow), reads the edge count back once
    and returns ``(neighbors [E,2] int32, ends [M] int32)`` -- the one synchronisation ``ball_query`` has.  With a
    ``capacity`` there is none (capturable when ``n_batches`` is given) and the result is ``(neighbors [capacity,2], ends,
    info [2] on the device)`` as from ``ball_query_bounded``.  ``want_degrees``: one more result, the uncapped degree of
    every sample ``[M] int32``.  ``seed_tensor``: a 1-element int32 device tensor whose bits are added to ``seed`` on the
    device -- a replayed graph draws fresh subsets when it is updated.  ``neighbors_out`` / ``src_box`` / ``grids``: as for
    ``ball_query_bounded``."""
    lib = _lib.load()
    m = int(max_neighbors)
    if m > MAX_CAPPED_NEIGHBORS:
        raise NotImplementedError(f"ball_query_capped: max_neighbors = {m}; the HIP kernel keeps at most "
                                  f"{MAX_CAPPED_NEIGHBORS} neighbours per sample (one per lane of a wavefront)")
    exact = capacity is None
    if exact and m <= 0:  # no cap and no buffer to size from it: the two-phase query
        nb, ends = ball_query(pts_src, pts_dst, batch_src, batch_dst, radius, n_batches, src_box)
        return (nb, ends, torch.diff(ends, prepend=ends.new_zeros(1))) if want_degrees else (nb, ends)

    def tail(dev, degrees):
        if seed_tensor is not None and (seed_tensor.numel() != 1 or seed_tensor.dtype != torch.int32):
            raise ValueError("seed_tensor must be a 1-element int32 tensor")
        return (m, int(seed) & 0xFFFFFFFF, _ptr(seed_tensor, torch.int32, "seed_tensor", dev), _ptr(degrees, torch.int32, "degrees"))

    neighbors, ends, info, _, degrees = _bounded_query(
        "ball_query_capped", (None, "se3_ball_query_capped"), pts_src, pts_dst, batch_src, batch_dst, radius, capacity,
        n_batches, neighbors_out, "neighbors_out must be a contiguous int32 [capacity, 2] tensor (and needs a capacity)",
        src_box, grids, rows_per_sample=m, want_degrees=want_degrees,
        workspace_bytes=lib.se3_ball_query_capped_workspace_bytes, tail=tail)
    res = (neighbors[:int(info[0].item())], ends) if exact else (neighbors, ends, info)
    return res + (degrees,) if want_degrees else res


class BallQuery(torch.autograd.Function):
    """Drop-in for ``point_cloud_lib.custom_ops.BallQuery`` (BallQuery.py:11-53).  Like the
    reference it returns ``neighbors`` as int64 (ball_query.cu:99-101 promotes through ``cat``)
    and ``start_ids`` (inclusive ends) as int32.  ``max_neighbors > 0`` keeps a seeded uniform subset of that size per
    sample (``ball_query_capped``; the seed comes from torch's default CPU generator), zero or less means no limit."""

    @staticmethod
    def forward(ctx, p_pt_src, p_pt_sample, p_batch_id_src, p_batch_id_sample, radius, max_neighbors, n_batches=None):
        """``n_batches`` (extension; the reference reads it back from the device, ball_query.cu:46): batch count
        when the caller knows it -- saves a host sync."""
        if max_neighbors > 0:
            nb, ends = ball_query_capped(p_pt_src, p_pt_sample, p_batch_id_src, p_batch_id_sample, radius, int(max_neighbors),
                                         draw_seed(), n_batches=n_batches)
            return nb.to(torch.int64), ends
        nb, ends = ball_query(p_pt_src, p_pt_sample, p_batch_id_src, p_batch_id_sample, radius, n_batches)
        return nb.to(torch.int64), ends

    @staticmethod
    def backward(ctx, *grads):
        return None, None, None, None, None, None, None


def csr_transpose(neighbors_i32: torch.Tensor, n_src: int, n_valid: Optional[torch.Tensor] = None, want_edge_ids: bool = False):
    """Source-major copy of an edge list: ``t_samples [E]``, ``t_ends [n_src]`` (inclusive).  ``n_valid`` (device int32
    tensor, e.g. ``info`` of ``ball_query_bounded``): only the first ``n_valid[0]`` rows are edges -- the unset tail of a
    capacity-sized buffer is ignored, without a host round trip.  ``want_edge_ids``: a third result ``t_edge_ids [E]``,
    the row of ``neighbors_i32`` every entry came from."""
    lib = _lib.load()
    dev = neighbors_i32.device
    e = neighbors_i32.shape[0]
    t_samples = _empty(e, dtype=torch.int32, device=dev)
    t_ends = _empty(n_src, dtype=torch.int32, device=dev)  # every entry is written by the library
    t_ids = _empty(e, dtype=torch.int32, device=dev) if want_edge_ids else None
    ws = _workspace(lib.se3_csr_transpose_workspace_bytes(e), dev)
    _lib.check(lib.se3_csr_transpose_bounded(_ptr(neighbors_i32, torch.int32, "neighbors"), e,
                                             _ptr(n_valid, torch.int32, "n_valid", dev), n_src, C.c_void_p(ws.data_ptr()),
                                             ws.numel(), _ptr(t_samples, torch.int32, "t_samples"),
                                             _ptr(t_ends, torch.int32, "t_ends"), _ptr(t_ids, torch.int32, "t_edge_ids"),
                                             _stream(dev)), "se3_csr_transpose_bounded")
    return (t_samples, t_ends, t_ids) if want_edge_ids else (t_samples, t_ends)


# ------------------------------------------------------------------------- hierarchy build (row f-2)
POOL_MODES = {"avg": 0, "max": 1, "min": 2, "sum": 3}


class GridCells:
    """Result of one grid sub-sampling step (``se3_grid_subsample``): the cell of every point (what
    ``torch.unique(keys, return_inverse=True)`` returns in Grid.py:45), the points grouped by cell, the cell sizes
    as inclusive end offsets, and the next level's points / batch ids (PointHierarchy.py:46-49).  ``padded``: the level of
    a padded hierarchy (``of_level``), whose absent points carry the cell id -1."""

    def __init__(self, cell_ids, sorted_ids, cell_ends, n_cells, pts, batch_ids):
        self.cell_ids, self.sorted_ids, self.cell_ends, self.n_cells = cell_ids, sorted_ids, cell_ends, n_cells
        self.pts, self.batch_ids = pts, batch_ids
        self.padded = False

    @classmethod
    def of_level(cls, level) -> "GridCells":
        """One level dict of ``BoundedLevels.levels`` as it stands, nothing read back: the capacity-sized tensors and ALL
        ``capacity`` cells.  ``cell_ends`` behind the kept cells holds the present-row count, so those segments are empty --
        pooling writes 0 in ``out`` and -1 in ``arg`` there and reads only rows that kept cells list."""
        cells = cls(level["cell_ids"], level["sorted_ids"], level["cell_ends"], level["cell_ends"].shape[0], level["pts"],
                    level["batch_ids"])
        cells.padded = True
        return cells


def grid_subsample(pts, batch_ids, cell_size: float, n_batches: Optional[int] = None) -> GridCells:
    lib = _lib.load()
    pts = _as(pts, torch.float32)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("grid_subsample: only [N,3] point sets are supported")
    if not (cell_size > 0):
        raise ValueError("grid_subsample: cell size must be positive")
    b = _as(batch_ids, torch.int32)
    dev, n = pts.device, pts.shape[0]
    if n_batches is None:
        n_batches = int(b.max().item()) + 1 if n else 1
    i32 = torch.int32
    cell_ids = _empty(n, dtype=i32, device=dev)
    sorted_ids = _empty(n, dtype=i32, device=dev)
    cell_ends = _empty(n, dtype=i32, device=dev)
    n_cells = torch.zeros(1, dtype=i32, device=dev)
    cell_pts = _empty((n, 3), dtype=torch.float32, device=dev)
    cell_bid = _empty(n, dtype=i32, device=dev)
    ws = _workspace(lib.se3_grid_subsample_workspace_bytes(n, n_batches), dev)
    _lib.check(lib.se3_grid_subsample(
        _ptr(pts, torch.float32, "pts"), _ptr(b, i32, "batch_ids", dev), n, n_batches, float(cell_size),
        C.c_void_p(ws.data_ptr()), ws.numel(), _ptr(cell_ids, i32, "cell_ids"), _ptr(sorted_ids, i32, "sorted_ids"),
        _ptr(cell_ends, i32, "cell_ends"), _ptr(n_cells, i32, "n_cells"), _ptr(cell_pts, torch.float32, "cell_pts"),
        _ptr(cell_bid, i32, "cell_batch_ids"), _stream(dev)), "se3_grid_subsample")
    m = int(n_cells.item())  # the level size has to reach the host: every later allocation depends on it
    return GridCells(cell_ids, sorted_ids, cell_ends[:m], m, cell_pts[:m], cell_bid[:m])


class LevelOverflow(RuntimeError):
    """A level of ``grid_levels_bounded`` has more cells than its capacity: ``level`` is the first such level and
    ``needed`` the row count it needs (the counts of deeper levels belong to the truncated hierarchy)."""

    def __init__(self, level: int, needed: int, capacity: int):
        super().__init__(f"level {level} of the bounded hierarchy has {needed} cells but a capacity of {capacity} rows: "
                         f"run again with a capacity of at least {needed}")
        self.level, self.needed, self.capacity = level, needed, capacity


class BoundedLevels:
    """What ``grid_levels_bounded`` returns: per level the padded tensors of ``struct se3_level``
    (include/se3conv_levels.h) as a dict -- ``cell_ids``, ``sorted_ids`` ``[n_in]``, ``cell_ends``, ``pts``, ``batch_ids``
    ``[capacity]`` and, on random levels, ``u``, ``ids``, ``picked`` ``[capacity]`` -- and ``info [n_levels, 2]`` (true cell
    count, overflow flag), all on the device.  Nothing here has been read by the host until ``trim()``."""

    def __init__(self, levels, info, counts, n_rows, has_n_valid, keep):
        self.levels, self.info, self.n_rows = levels, info, n_rows
        self.capacities = [lv["pts"].shape[0] for lv in levels]
        self._counts, self._has_n_valid, self._keep = counts, has_n_valid, keep

    def trim(self):
        """The ONE device-to-host copy of a bounded build: reads every level size, raises ``LevelOverflow`` for the first
        level that did not fit, and otherwise returns one ``GridCells`` per level -- views of the padded buffers, no
        copies -- as ``grid_subsample`` builds them (``ids`` / ``picked`` are set on random levels and None otherwise; a
        random level's ``pts`` / ``batch_ids`` are those of its picked rows)."""
        counts = self._counts.cpu().tolist()
        present = self.n_rows
        if self._has_n_valid:
            present = min(max(counts[0][0], 0), self.n_rows)
            counts = counts[1:]
        for l, ((m, flag), cap) in enumerate(zip(counts, self.capacities)):
            if flag:
                raise LevelOverflow(l, m, cap)
        out = []
        for lv, (m, _) in zip(self.levels, counts):
            cells = GridCells(lv["cell_ids"][:present], lv["sorted_ids"][:present], lv["cell_ends"][:m], m, lv["pts"][:m],
                              lv["batch_ids"][:m])
            cells.ids = lv["ids"][:m] if "ids" in lv else None
            cells.picked = lv["picked"][:m] if "picked" in lv else None
            out.append(cells)
            present = m
        return out


def grid_levels_bounded(pts, batch_ids, cell_sizes, capacities, n_batches: int, n_valid: Optional[torch.Tensor] = None,
                        rnd=None, rnd_values=None) -> BoundedLevels:
    """A chain of grid sub-sampling levels in one library call (``se3_grid_levels``, include/se3conv_levels.h): level l is
    written into buffers of ``capacities[l]`` rows (``"input"``: the row count of ``pts`` for every level, which cannot
    overflow), the level sizes stay on the device, and nothing synchronises with the host -- the call can be captured into a
    HIP graph and replayed on another batch.  ``n_valid`` (int32 device word, optional): only rows ``[0, n_valid)`` of
    ``pts`` / ``batch_ids`` are present.  ``rnd[l]`` true: level l is one random point per cell, drawn with
    ``rnd_values[l]`` (``[capacities[l]]`` uniform numbers in [0,1); default: ``torch.rand`` on the device).
    ``pts`` float32 ``[N,3]`` and ``batch_ids`` int32 ``[N]`` are taken as they are (a conversion would be a launch of
    its own): anything else is a ValueError."""
    lib = _lib.load()
    f32, i32 = torch.float32, torch.int32
    n_levels = len(cell_sizes)
    if n_levels < 1:
        raise ValueError("grid_levels_bounded: at least one level")
    if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("grid_levels_bounded: only [N,3] point sets are supported")
    dev, n = pts.device, pts.shape[0]
    p_pts = _ptr(pts, f32, "pts")
    p_bid = _ptr(batch_ids, i32, "batch_ids", dev)
    if tuple(batch_ids.shape) != (n,):
        raise ValueError(f"grid_levels_bounded: batch_ids of shape {tuple(batch_ids.shape)} for {n} points")
    if not all(c > 0 for c in cell_sizes):
        raise ValueError("grid_levels_bounded: cell sizes must be positive")
    if isinstance(capacities, str):
        if capacities != "input":
            raise ValueError(f"grid_levels_bounded: capacities {capacities!r}; expected 'input' or one row count per level")
        capacities = [max(n, 1)] * n_levels
    capacities = [int(c) for c in capacities]
    if len(capacities) != n_levels or min(capacities) < 1:
        raise ValueError("grid_levels_bounded: one capacity >= 1 per level")
    if int(n_batches) < 1:
        raise ValueError("grid_levels_bounded: n_batches must be at least 1")
    p_valid = _ptr(n_valid, i32, "n_valid", dev)
    if n_valid is not None and n_valid.numel() != 1:
        raise ValueError("grid_levels_bounded: n_valid is one int32 word on the device")
    rnd = [bool(r) for r in rnd] if rnd is not None else [False] * n_levels
    rnd_values = list(rnd_values) if rnd_values is not None else [None] * n_levels
    if len(rnd) != n_levels or len(rnd_values) != n_levels:
        raise ValueError("grid_levels_bounded: rnd / rnd_values take one entry per level")
    for l in range(n_levels):
        u = rnd_values[l]
        if u is not None:
            _ptr(u, f32, f"rnd_values[{l}]", dev)
            if not rnd[l] or tuple(u.shape) != (capacities[l],):
                raise ValueError(f"grid_levels_bounded: rnd_values[{l}] takes [{capacities[l]}] numbers of a random level")
    levels, structs, n_in = [], (_lib.Se3Level * n_levels)(), n
    for l, cap in enumerate(capacities):
        lv = {"cell_ids": _empty(n_in, dtype=i32, device=dev), "sorted_ids": _empty(n_in, dtype=i32, device=dev),
              "cell_ends": _empty(cap, dtype=i32, device=dev), "pts": _empty((cap, 3), dtype=f32, device=dev),
              "batch_ids": _empty(cap, dtype=i32, device=dev)}
        if rnd[l]:
            lv["u"] = rnd_values[l] if rnd_values[l] is not None else torch.rand(cap, device=dev)
            lv["ids"], lv["picked"] = _empty(cap, dtype=i32, device=dev), _empty(cap, dtype=i32, device=dev)
        s = structs[l]
        s.cell_size, s.capacity = float(cell_sizes[l]), cap
        for name in ("cell_ids", "sorted_ids", "cell_ends", "pts", "batch_ids", "u", "ids", "picked"):
            setattr(s, name, lv[name].data_ptr() if name in lv else None)
        levels.append(lv)
        n_in = cap
    # the level sizes, behind the caller's n_valid word when there is one: trim() reads them all with one copy
    counts = _empty((n_levels + (n_valid is not None), 2), dtype=i32, device=dev)
    info = counts[1:] if n_valid is not None else counts
    ws = _workspace(lib.se3_grid_levels_workspace_bytes(n, int(n_batches), structs, n_levels), dev)
    _lib.check(lib.se3_grid_levels(p_pts, p_bid, n, p_valid, int(n_batches), structs, n_levels,
                                   C.c_void_p(info.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)),
               "se3_grid_levels")
    if n_valid is not None:
        counts[0].copy_(n_valid.reshape(1).expand(2))
    return BoundedLevels(levels, info, counts, n, n_valid is not None, (pts, batch_ids, n_valid, ws))


# --------------------------------------------------------------------------- farthest-point sampling
class FpsOverflow(RuntimeError):
    """``fps`` chose more samples than its capacity: ``needed`` is the row count to run again with."""

    def __init__(self, needed: int, capacity: int):
        super().__init__(f"farthest-point sampling chose {needed} samples but has a capacity of {capacity} rows: "
                         f"run again with a capacity of at least {needed}")
        self.needed, self.capacity = needed, capacity


class FpsSamples:
    """What ``fps`` returns, all on the device and of fixed size: ``ids [capacity]`` int32 (rows of ``pts`` in pick order,
    element after element; -1 behind the last sample), ``d2 [capacity]`` float32 (``d2_at_pick`` of include/se3conv_fps.h;
    -1 behind), ``starts [n_batches + 1]`` int32 (where each element's samples begin) and ``info [3]`` int32 (sample count
    M, overflow flag, bad ``batch_ids`` flag).  Nothing here has been read by the host until ``trim()``."""

    def __init__(self, ids, d2, starts, info, capacity, meta, keep):
        self.ids, self.d2, self.starts, self.info, self.capacity = ids, d2, starts, info, capacity
        self._meta, self._keep = meta, keep

    def trim(self):
        """The ONE device-to-host copy: ``(ids[:M], d2[:M], starts)`` as views.  ``ValueError`` when ``batch_ids`` were
        not sorted or out of range, ``FpsOverflow`` when M exceeds the capacity."""
        m, overflow, bad = self._meta[-3:].cpu().tolist()
        if bad:
            raise ValueError("fps: batch_ids must be non-decreasing and inside [0, num_batches)")
        if overflow:
            raise FpsOverflow(m, self.capacity)
        return self.ids[:m], self.d2[:m], self.starts


def fps(pts, batch_ids, ratio: float, num_batches: Optional[int] = None, start_u: Optional[torch.Tensor] = None,
        n_valid: Optional[torch.Tensor] = None, capacity: Optional[int] = None) -> FpsSamples:
    """Farthest-point sampling per batch element (``se3_fps``, include/se3conv_fps.h: what ``torch_cluster.fps`` is asked
    for, with a deterministic contract): element ``b`` -- the run of rows with ``batch_ids == b``, which must be sorted --
    gets ``min(n_b, ceil(n_b * ratio))`` samples (fp32 product), starting at row ``floor(start_u[b] * n_b)`` (``start_u``
    float32 ``[num_batches]`` in [0,1); None: the element's first row).  Nothing synchronises with the host, so the call can
    be captured into a HIP graph; ``n_valid`` (int32 device word): only rows ``[0, n_valid)`` are present.  ``capacity``
    (rows of the outputs) defaults to the row count of ``pts``, which cannot overflow for any ratio <= 1.  ``pts`` float32
    ``[N,3]`` and ``batch_ids`` int32 ``[N]`` are taken as they are: anything else is a ValueError.  ``num_batches=None``
    reads the largest id back (not with ``n_valid``: that would read absent rows)."""
    lib = _lib.load()
    f32, i32 = torch.float32, torch.int32
    _padded_cloud(pts, batch_ids, "fps")
    dev, n = pts.device, pts.shape[0]
    ratio = float(ratio)
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"fps: ratio {ratio}; expected 0 < ratio <= 1")
    p_valid = _valid_word(n_valid, dev, "fps")
    if num_batches is None:
        if n_valid is not None:
            raise ValueError("fps: a padded cloud (n_valid) needs num_batches")
        num_batches = int(batch_ids.max().item()) + 1 if n else 1
    nb = int(num_batches)
    if nb < 1:
        raise ValueError("fps: num_batches must be at least 1")
    p_u = _ptr(start_u, f32, "start_u", dev)
    if start_u is not None and tuple(start_u.shape) != (nb,):
        raise ValueError(f"fps: start_u of shape {tuple(start_u.shape)} for {nb} batch elements")
    cap = n if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("fps: capacity must not be negative")
    ids_buf = _empty(max(cap, 1), dtype=i32, device=dev)  # (at least one row: an empty tensor has no address)
    d2_buf = _empty(max(cap, 1), dtype=f32, device=dev)
    ids, d2 = ids_buf[:cap], d2_buf[:cap]
    meta = _empty(nb + 4, dtype=i32, device=dev)  # starts [nb + 1] | info [3]: trim() reads the flags with one copy
    starts, info = meta[:nb + 1], meta[nb + 1:]
    need = lib.se3_fps_workspace_bytes(n, nb)
    ws = _workspace(need, dev)
    _lib.check(lib.se3_fps(C.c_void_p(pts.data_ptr()), C.c_void_p(batch_ids.data_ptr()), n, p_valid, nb, ratio, p_u, cap,
                           C.c_void_p(ids_buf.data_ptr()), C.c_void_p(d2_buf.data_ptr()), C.c_void_p(starts.data_ptr()),
                           C.c_void_p(info.data_ptr()), C.c_void_p(ws.data_ptr()), need, _stream(dev)), "se3_fps")
    return FpsSamples(ids, d2, starts, info, cap, meta, (pts, batch_ids, start_u, n_valid, ws))


def _rows2d(t):
    return t.reshape(t.shape[0], -1) if t.dim() != 2 else t


def _segment_pool(cells: GridCells, x2, mode: int, want_arg: bool):
    lib = _lib.load()
    c = x2.shape[1]
    if x2.shape[0] != cells.cell_ids.shape[0]:
        raise ValueError(f"pooling {x2.shape[0]} rows through a level with {cells.cell_ids.shape[0]} input rows")
    out = _empty((cells.n_cells, c), dtype=torch.float32, device=x2.device)
    arg = _empty((cells.n_cells, c), dtype=torch.int32, device=x2.device) if want_arg else None
    _lib.check(lib.se3_segment_pool(_ptr(x2, torch.float32, "src"), _ptr(cells.sorted_ids, torch.int32, "sorted_ids"),
                                    _ptr(cells.cell_ends, torch.int32, "cell_ends"), cells.n_cells, c, mode,
                                    _ptr(out, torch.float32, "out"), _ptr(arg, torch.int32, "arg"), _stream(x2.device)),
               "se3_segment_pool")
    return out, arg


def _segment_unpool(cells: GridCells, v2, arg, mode: int):
    lib = _lib.load()
    n, c = cells.cell_ids.shape[0], v2.shape[1]
    if v2.shape[0] != cells.n_cells:
        raise ValueError(f"up-sampling {v2.shape[0]} rows through a level of {cells.n_cells} cells")
    # (two instantiations of one kernel: the padded one writes a zero row where the cell id is negative -- an absent point
    # or one of a dropped cell)
    name = "se3_segment_unpool_padded" if cells.padded else "se3_segment_unpool"
    out = _empty((n, c), dtype=torch.float32, device=v2.device)
    _lib.check(getattr(lib, name)(_ptr(v2, torch.float32, "cell_vals"), _ptr(cells.cell_ids, torch.int32, "cell_ids"),
                                  _ptr(cells.cell_ends, torch.int32, "cell_ends"), _ptr(arg, torch.int32, "arg"),
                                  n, c, mode, _ptr(out, torch.float32, "out"), _stream(v2.device)), name)
    return out


def grid_pick(cells: GridCells, u: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One random point per cell (GridSubSample.py:43-54): ``ids [n_cells]`` = positions in the cell-sorted point list
    (the reference's ``ids_``) and ``picked [n_cells]`` = those points' indices (``sorted_ids_[ids_]``).  ``u``:
    uniform numbers in [0,1), one per cell (default: drawn on the device -- the reference draws them on the host and
    copies them over); nothing here synchronises with the host."""
    lib = _lib.load()
    dev = cells.sorted_ids.device
    if u is None:
        u = torch.rand(cells.n_cells, device=dev)
    u = _as(u, torch.float32).to(dev)
    if u.shape != (cells.n_cells,):
        raise ValueError(f"grid_pick: {tuple(u.shape)} random numbers for {cells.n_cells} cells")
    i32 = torch.int32
    ids = _empty(cells.n_cells, dtype=i32, device=dev)
    picked = _empty(cells.n_cells, dtype=i32, device=dev)
    _lib.check(lib.se3_grid_pick(_ptr(cells.cell_ends, i32, "cell_ends", dev), _ptr(cells.sorted_ids, i32, "sorted_ids"),
                                 _ptr(u, torch.float32, "u"), cells.n_cells, _ptr(ids, i32, "ids"),
                                 _ptr(picked, i32, "picked"), _stream(dev)), "se3_grid_pick")
    return ids, picked


def _rows_move(lib_fn, name, src, idx, out):
    row_bytes = src[0].numel() * src.element_size() if src.shape[0] else max(1, out[0].numel() * out.element_size())
    _lib.check(lib_fn(C.c_void_p(src.data_ptr()), _ptr(idx, torch.int32, "idx", src.device), idx.shape[0], row_bytes,
                      C.c_void_p(out.data_ptr()), _stream(src.device)), name)


def rows_gather(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``src[idx]`` along dim 0 for any dtype (``se3_rows_gather``)."""
    if not src.is_cuda:
        raise ValueError("rows_gather: expected a GPU tensor (the HIP path has no CPU fallback)")
    src = src.detach().contiguous()
    out = _empty((idx.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if idx.shape[0] and out.numel():
        _rows_move(_lib.load().se3_rows_gather, "se3_rows_gather", src, idx, out)
    return out


def rows_scatter(src: torch.Tensor, idx: torch.Tensor, n_rows: int) -> torch.Tensor:
    """Zeros ``[n_rows, ...]`` with ``out[idx[r]] = src[r]`` (unique ``idx``; ``se3_rows_scatter``)."""
    if not src.is_cuda:
        raise ValueError("rows_scatter: expected a GPU tensor (the HIP path has no CPU fallback)")
    src = src.detach().contiguous()
    out = torch.zeros((int(n_rows),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if idx.shape[0] and src.numel():
        _rows_move(_lib.load().se3_rows_scatter, "se3_rows_scatter", src, idx, out)
    return out


class RowsGather(torch.autograd.Function):
    """``x[idx]`` for unique row indices (``__subsample_tensor__`` of the random grid sub-sample, GridSubSample.py:67);
    the gradient is the scatter into zeros."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.idx, ctx.n = idx, x.shape[0]
        return rows_gather(x, idx)

    @staticmethod
    def backward(ctx, g):
        return rows_scatter(g, ctx.idx, ctx.n), None


class RowsScatter(torch.autograd.Function):
    """Rows ``idx`` of a zero tensor ``[n_rows, ...]`` set to ``x`` (``__upsample_tensor__``, GridSubSample.py:83-91);
    the gradient is the gather."""

    @staticmethod
    def forward(ctx, x, idx, n_rows):
        ctx.idx = idx
        return rows_scatter(x, idx, n_rows)

    @staticmethod
    def backward(ctx, g):
        return rows_gather(g, ctx.idx), None, None


class GridPool(torch.autograd.Function):
    """``pool_tensor`` of one level step (GridSubSample.py:63-77): rows of level l -> rows of level l+1.  Through padded
    cells (``GridCells.of_level``): [n_in, ...] -> [capacity, ...] with zeros behind the kept cells, and a gradient of zero
    rows at absent points and dropped cells."""

    @staticmethod
    def forward(ctx, x, cells, method):
        mode = POOL_MODES[method]
        x2 = _rows2d(_as(x, torch.float32))
        out, arg = _segment_pool(cells, x2, mode, mode in (1, 2))
        ctx.cells, ctx.mode, ctx.arg, ctx.shape = cells, mode, arg, x.shape
        return out.reshape((cells.n_cells,) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        g2 = _rows2d(_as(g, torch.float32))
        return _segment_unpool(ctx.cells, g2, ctx.arg, ctx.mode).reshape(ctx.shape), None, None


class GridUpsample(torch.autograd.Function):
    """``upsample_tensor`` (GridSubSample.py:93: ``p_tensor[cell_ids]``); the gradient is a segment sum in fixed order
    instead of the atomics of an index_add.  Through padded cells the rows of absent points and of dropped cells get zeros,
    and the gradient is the segment sum over all ``capacity`` cells."""

    @staticmethod
    def forward(ctx, x, cells):
        x2 = _rows2d(_as(x, torch.float32))
        ctx.cells, ctx.shape = cells, x.shape
        return _segment_unpool(cells, x2, None, 3).reshape((cells.cell_ids.shape[0],) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        g2 = _rows2d(_as(g, torch.float32))
        return _segment_pool(ctx.cells, g2, 3, False)[0].reshape(ctx.shape), None


# ------------------------------------------------------------------------------ frame pooling (row f-3)
class FramePool(torch.autograd.Function):
    """``PointcloudRotEquiv.feature_pooling`` (pc/PointcloudRotEquiv.py:224-251): [N*F, C] -> [N, C].  ``n_valid``: the
    row-count word of a padded cloud -- ``x`` is then taken as it is ([n_rows * F, C] float32 on the GPU), absent points
    are not read and get zeros both ways."""

    @staticmethod
    def forward(ctx, x, n_frames, method, n_valid=None):
        mode = POOL_MODES[method]
        if n_valid is not None:
            x2 = _padded_rows(x, n_frames, "FramePool")[0]
        else:
            x2 = _rows2d(_as(x, torch.float32))
            if x2.shape[0] % n_frames:
                raise ValueError("feature_pooling: rows are not a multiple of the frame count")
        n, c, dev = x2.shape[0] // n_frames, x2.shape[1], x2.device
        out = _empty((n, c), dtype=torch.float32, device=dev)
        arg = _empty((n, c), dtype=torch.int32, device=dev) if mode in (1, 2) else None
        ctx.word = (_valid_word(n_valid, dev, "FramePool"),) if n_valid is not None else ()
        fn, name = _row_pass("se3_frame_pool", n_valid)
        _lib.check(fn(_ptr(x2, torch.float32, "x"), n, int(n_frames), *ctx.word, c, mode, _ptr(out, torch.float32, "out"),
                      _ptr(arg, torch.int32, "arg"), _stream(dev)), name)
        ctx.mode, ctx.arg, ctx.f, ctx.shape, ctx.n_valid = mode, arg, int(n_frames), x.shape, n_valid
        return out.reshape((n,) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        g2 = _rows2d(_as(g, torch.float32))
        n, c = g2.shape
        gx = _empty((n * ctx.f, c), dtype=torch.float32, device=g2.device)
        fn, name = _row_pass("se3_frame_unpool", ctx.n_valid)
        _lib.check(fn(_ptr(g2, torch.float32, "grad_out"), _ptr(ctx.arg, torch.int32, "arg"), n, ctx.f, *ctx.word, c,
                      ctx.mode, _ptr(gx, torch.float32, "grad_x"), _stream(g2.device)), name)
        return gx.reshape(ctx.shape), None, None, None


# ------------------------------------------------------------------------------------------ global pooling
# One row per batch element (include/se3conv_global_pool.h): fp64 sums in a fixed order and no atomic, so two calls give the
# same bits; with the row-count word of a padded cloud neither an absent row nor an absent id is read.  The ids are per
# POINT ([n_rows] int32), whatever the frame count.
def _point_ids(batch_ids, n_valid, dev, who: str) -> torch.Tensor:
    """The [n_rows] int32 ids as the library reads them: taken as they are with a word (a conversion would read the absent
    ones), converted without one."""
    if n_valid is None:
        batch_ids = _as(batch_ids, torch.int32)
    _ptr(batch_ids, torch.int32, "batch_ids", dev)
    if batch_ids.dim() != 1:
        raise ValueError(f"{who}: batch_ids is [n_rows], one id per point")
    return batch_ids


def global_pool(x, batch_ids, n_batches: int, mode, frames: int = 1, n_valid: Optional[torch.Tensor] = None):
    """``se3_global_pool``: ``x [n_rows * frames, C]`` -> ``(out [n_batches, C] float32, arg [n_batches, C] int32 or None,
    counts [n_batches] int32)``.  ``mode``: a name of ``POOL_MODES`` or its number; ``arg`` (the winning row) for max / min
    only.  ``n_valid``: the row-count word of a padded cloud -- ``x`` and ``batch_ids`` are then taken as they are."""
    mode = POOL_MODES[mode] if isinstance(mode, str) else int(mode)
    who = "global_pool"
    x2, n = _padded_rows(x if n_valid is not None else _rows2d(_as(x, torch.float32)), frames, who)
    c, dev, nb = x2.shape[1], x2.device, int(n_batches)
    ids = _point_ids(batch_ids, n_valid, dev, who)
    if ids.shape[0] != n:
        raise ValueError(f"{who}: {ids.shape[0]} batch ids for {n} points")
    lib = _lib.load()
    out = _empty((nb, c), dtype=torch.float32, device=dev)
    arg = _empty((nb, c), dtype=torch.int32, device=dev) if mode in (1, 2) else None
    counts = _empty((nb,), dtype=torch.int32, device=dev)
    need = lib.se3_global_pool_workspace_bytes(n, int(frames), nb, c)
    ws = _workspace(need, dev)
    _lib.check(lib.se3_global_pool(_ptr(x2, torch.float32, "x"), _ptr(ids, torch.int32, "batch_ids"), n, int(frames),
                                   _valid_word(n_valid, dev, who), nb, c, mode, _ptr(out, torch.float32, "out"),
                                   _ptr(arg, torch.int32, "arg"), _ptr(counts, torch.int32, "counts"),
                                   C.c_void_p(ws.data_ptr()), need, _stream(dev)), "se3_global_pool")
    return out, arg, counts


def global_unpool(vals, batch_ids, mode, frames: int = 1, n_valid: Optional[torch.Tensor] = None,
                  arg: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``se3_global_unpool``: ``vals [n_batches, C]`` -> ``[n_rows * frames, C]`` -- in sum mode ``vals[batch_ids[point]]``,
    otherwise the gradient of ``global_pool`` in that mode (``arg`` for max / min, ``counts`` for avg, both as the pool
    returned them).  Absent rows and rows of points with an id outside ``[0, n_batches)`` are zero."""
    mode = POOL_MODES[mode] if isinstance(mode, str) else int(mode)
    who = "global_unpool"
    v2 = _rows2d(_as(vals, torch.float32))
    if not v2.is_cuda:
        raise ValueError(f"{who}: expected [n_batches, C] values on the GPU (the HIP path has no CPU fallback)")
    nb, c, dev = v2.shape[0], v2.shape[1], v2.device
    ids = _point_ids(batch_ids, n_valid, dev, who)
    n = ids.shape[0]
    if arg is not None and tuple(arg.shape) != (nb, c) or counts is not None and tuple(counts.shape) != (nb,):
        raise ValueError(f"{who}: arg is [n_batches, C] and counts [n_batches], as global_pool returns them")
    out = _empty((n * int(frames), c), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().se3_global_unpool(_ptr(v2, torch.float32, "vals"), _ptr(ids, torch.int32, "batch_ids"),
                                             _ptr(arg, torch.int32, "arg", dev), _ptr(counts, torch.int32, "counts", dev), n,
                                             int(frames), _valid_word(n_valid, dev, who), nb, c, mode,
                                             _ptr(out, torch.float32, "out"), _stream(dev)), "se3_global_unpool")
    return out


class GlobalPool(torch.autograd.Function):
    """``global_pooling`` (pc/Pointcloud.py:58-76, pc/PointcloudRotEquiv.py:252-270): [n_rows * F, C] -> [B, C]; the gradient
    is ``se3_global_unpool``.  ``n_valid``: the word of a padded cloud."""

    @staticmethod
    def forward(ctx, x, batch_ids, n_batches, method, n_frames=1, n_valid=None):
        out, arg, counts = global_pool(x, batch_ids, n_batches, method, n_frames, n_valid)
        ctx.ids, ctx.method, ctx.f, ctx.n_valid, ctx.arg, ctx.counts, ctx.shape = batch_ids, method, int(n_frames), n_valid, arg, counts, x.shape
        return out.reshape((int(n_batches),) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        gx = global_unpool(g, ctx.ids, ctx.method, ctx.f, ctx.n_valid, ctx.arg, ctx.counts)
        return gx.reshape(ctx.shape), None, None, None, None, None


class GlobalUpsample(torch.autograd.Function):
    """``global_upsample`` (pc/Pointcloud.py:79-88): [B, C] -> [n_rows * F, C], ``x[batch_ids[point]]`` with zero rows for
    absent points; the gradient is the sum pool, in its fixed order instead of the atomics of an index_add."""

    @staticmethod
    def forward(ctx, x, batch_ids, n_frames=1, n_valid=None):
        ctx.ids, ctx.f, ctx.n_valid, ctx.shape = batch_ids, int(n_frames), n_valid, x.shape
        out = global_unpool(x, batch_ids, "sum", n_frames, n_valid)
        return out.reshape((out.shape[0],) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        # (with a word the gradient is taken as it is: its absent rows are not read)
        g2 = g.contiguous() if ctx.n_valid is not None else g
        return global_pool(g2, ctx.ids, ctx.shape[0], "sum", ctx.f, ctx.n_valid)[0].reshape(ctx.shape), None, None, None


# ------------------------------------------------------------------------------------------ group norm
def _point_rows(x2: torch.Tensor, n_valid, frames: int, who: str) -> tuple:
    """``n_rows, frames, n_valid`` of an entry point that always takes the three: those of ``_glue_rows`` with a row-count word,
    every point and a null word without one."""
    if n_valid is not None:
        return _glue_rows(x2, n_valid, frames, who)
    return (x2.shape[0] // frames, frames, C.c_void_p(0))


class GroupNorm(torch.autograd.Function):
    """``GroupNormPC`` (layers/GroupNormPC.py:34-57) on ``[n_rows * n_frames, C]``: every batch element normalised on its own
    per group of channels (the group of channel ``c`` is ``c % num_groups``), ``se3_group_norm_fwd`` / ``se3_group_norm_bwd``
    (include/se3conv_group_norm.h) -- fp64 sums in a fixed order and no atomic, so two calls give the same bits.
    ``batch_ids``: one id per POINT.  ``n_valid``: the row-count word of a padded cloud -- ``x``, the gradient and the ids are
    then taken as they are, statistics and gradients run over the present rows alone, and the absent rows get zeros."""

    @staticmethod
    def forward(ctx, x, gamma, beta, batch_ids, n_batches, num_groups, eps, n_valid=None, n_frames=1):
        f32, who = torch.float32, "GroupNorm"
        x2 = _feature_rows(x, n_valid, n_frames, who)
        if not x2.is_cuda:
            raise ValueError(f"{who}: expected [rows, C] features on the GPU (the HIP path has no CPU fallback)")
        c, dev, nb, groups, frames = x2.shape[1], x2.device, int(n_batches), int(num_groups), int(n_frames)
        ids = _point_ids(batch_ids, n_valid, dev, who)
        if frames < 1 or ids.shape[0] * frames != x2.shape[0]:
            raise ValueError(f"{who}: {ids.shape[0]} batch ids and {frames} frame(s) for {x2.shape[0]} rows")
        ga, be = _as(gamma, f32).reshape(-1), _as(beta, f32).reshape(-1)
        if ga.shape[0] != c or be.shape[0] != c:
            raise ValueError(f"{who}: gamma and beta hold one value per channel")
        lib = _lib.load()
        y = _empty_like(x2)
        mean = _empty((nb, groups), dtype=f32, device=dev)
        invstd = _empty((nb, groups), dtype=f32, device=dev)
        need = lib.se3_group_norm_workspace_bytes(ids.shape[0], frames, nb, c, groups)
        ws = _workspace(need, dev)
        _lib.check(lib.se3_group_norm_fwd(_ptr(x2, f32, "x"), _ptr(ga, f32, "gamma", dev), _ptr(be, f32, "beta", dev),
                                          _ptr(ids, torch.int32, "batch_ids"), *_point_rows(x2, n_valid, frames, who),
                                          nb, c, groups, float(eps), _ptr(y, f32, "y"),
                                          _ptr(mean, f32, "save_mean"), _ptr(invstd, f32, "save_invstd"),
                                          C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)), "se3_group_norm_fwd")
        ctx.save_for_backward(x2, ga, mean, invstd, ids)
        ctx.nb, ctx.groups, ctx.frames, ctx.n_valid = nb, groups, frames, n_valid
        ctx.gamma_shape, ctx.beta_shape = gamma.shape, beta.shape
        return y

    @staticmethod
    def backward(ctx, g):
        f32, who = torch.float32, "GroupNorm"
        x2, ga, mean, invstd, ids = ctx.saved_tensors
        g2 = _as(g, f32)
        c, dev = x2.shape[1], x2.device
        lib = _lib.load()
        dx = _empty_like(x2)
        dgamma = _empty(c, dtype=f32, device=dev)
        dbeta = _empty(c, dtype=f32, device=dev)
        need = lib.se3_group_norm_workspace_bytes(ids.shape[0], ctx.frames, ctx.nb, c, ctx.groups)
        ws = _workspace(need, dev)
        _lib.check(lib.se3_group_norm_bwd(_ptr(g2, f32, "dy", dev), _ptr(x2, f32, "x"), _ptr(ga, f32, "gamma"),
                                          _ptr(mean, f32, "save_mean"), _ptr(invstd, f32, "save_invstd"),
                                          _ptr(ids, torch.int32, "batch_ids"), *_point_rows(x2, ctx.n_valid, ctx.frames, who),
                                          ctx.nb, c, ctx.groups, _ptr(dx, f32, "dx"),
                                          _ptr(dgamma, f32, "dgamma"), _ptr(dbeta, f32, "dbeta"), C.c_void_p(ws.data_ptr()),
                                          ws.numel(), _stream(dev)), "se3_group_norm_bwd")
        ng = ctx.needs_input_grad
        return (dx if ng[0] else None, dgamma.reshape(ctx.gamma_shape) if ng[1] else None,
                dbeta.reshape(ctx.beta_shape) if ng[2] else None) + (None,) * 6


# ------------------------------------------------------------------------------------------ loss and metrics head
# include/se3conv_seg_head.h: the mean smoothed cross-entropy over the rows that count and the per-class counters of
# SemSegMetrics in one pass over the logits, the gradient in a second.  Nothing is compacted and nothing is read back: which
# classes count is a device mask, which rows exist a device word.
_counted_masks: dict = {}


def counted_mask(classes: int, not_counted, device) -> torch.Tensor:
    """The ``[classes]`` uint8 mask of ``se3_seg_loss_fwd`` from the ids of the classes that do NOT count (``p_mask_cls`` of the
    task scripts).  Uploaded once per (ids, classes, device) and kept: a later call, inside a capture too, copies nothing."""
    ids = tuple(sorted({int(i) for i in not_counted}))
    key = (ids, int(classes), str(device))
    mask = _counted_masks.get(key)
    if mask is None:
        host = torch.ones(int(classes), dtype=torch.uint8)
        for i in ids:
            if 0 <= i < int(classes):
                host[i] = 0
        mask = _counted_masks[key] = host.to(device)
    return mask


def _seg_labels(labels, n: int, dev, who: str) -> Tuple[C.c_void_p, int]:
    """Labels are taken as they are, int64 (torch's) or int32: ``(pointer, label_bits)``."""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: labels are an int64 or int32 tensor (they are not converted)")
    if tuple(labels.shape) != (n,):
        raise ValueError(f"{who}: labels of shape {tuple(labels.shape)} for {n} rows of logits")
    return _ptr(labels, labels.dtype, "labels", dev), 64 if labels.dtype == torch.int64 else 32


class SegLoss(torch.autograd.Function):
    """``CrossEntropyLoss(reduction="mean", label_smoothing=...)`` over the rows of ``logits [n_rows, classes]`` that count
    (``se3_seg_loss_fwd`` / ``se3_seg_loss_bwd``): a row counts iff it is present, its label lies in ``[0, classes)`` (so -100 is
    ignored) and ``counted`` (a ``[classes]`` uint8 device tensor, or None) is nonzero at the label.  ``n_valid``: the row-count
    word of a padded cloud -- logits and labels are then taken as they are and no absent row or label is read.  ``tallies``
    (``[3, classes]`` int64 on the device, or None): the call ADDS the counted rows' ground truth / predicted / hit counts.
    Every row that does not count gets a zero gradient."""

    @staticmethod
    def forward(ctx, logits, labels, label_smoothing=0.0, counted=None, n_valid=None, tallies=None):
        f32, who = torch.float32, "SegLoss"
        x2 = _feature_rows(logits, n_valid, 1, who)
        if not x2.is_cuda:
            raise ValueError(f"{who}: expected [rows, classes] logits on the GPU (the HIP path has no CPU fallback)")
        n, classes, dev = x2.shape[0], x2.shape[1], x2.device
        lab_ptr, bits = _seg_labels(labels, n, dev, who)
        if counted is not None and tuple(counted.shape) != (classes,):
            raise ValueError(f"{who}: counted is [classes] uint8")
        if tallies is not None and (tuple(tallies.shape) != (3, classes) or tallies.requires_grad):
            raise ValueError(f"{who}: tallies is [3, classes] int64")
        lib = _lib.load()
        loss = _empty((1,), dtype=f32, device=dev)
        count = _empty((1,), dtype=torch.int32, device=dev)
        lse = _empty((n,), dtype=torch.float64, device=dev) if ctx.needs_input_grad[0] else None
        need = lib.se3_seg_head_workspace_bytes(n, classes)
        ws = _workspace(need, dev)
        _lib.check(lib.se3_seg_loss_fwd(_ptr(x2, f32, "logits"), lab_ptr, bits, _ptr(counted, torch.uint8, "counted", dev), n,
                                        _valid_word(n_valid, dev, who), classes, float(label_smoothing), _ptr(loss, f32, "loss"),
                                        _ptr(count, torch.int32, "count"), _ptr(lse, torch.float64, "lse"),
                                        _ptr(tallies, torch.int64, "tallies", dev), C.c_void_p(ws.data_ptr()), ws.numel(),
                                        _stream(dev)), "se3_seg_loss_fwd")
        if lse is not None:
            ctx.save_for_backward(x2, labels, lse, count)
        ctx.counted, ctx.n_valid, ctx.smoothing, ctx.shape = counted, n_valid, float(label_smoothing), logits.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        f32, who = torch.float32, "SegLoss"
        x2, labels, lse, count = ctx.saved_tensors
        n, classes, dev = x2.shape[0], x2.shape[1], x2.device
        g1 = _as(g, f32).reshape(1)
        lab_ptr, bits = _seg_labels(labels, n, dev, who)
        dx = _empty_like(x2)
        _lib.check(_lib.load().se3_seg_loss_bwd(_ptr(x2, f32, "logits"), lab_ptr, bits,
                                                _ptr(ctx.counted, torch.uint8, "counted", dev), _ptr(lse, torch.float64, "lse"),
                                                _ptr(count, torch.int32, "count"), _ptr(g1, f32, "grad_loss", dev), n,
                                                _valid_word(ctx.n_valid, dev, who), classes, ctx.smoothing,
                                                _ptr(dx, f32, "grad_logits"), _stream(dev)), "se3_seg_loss_bwd")
        return dx.reshape(ctx.shape), None, None, None, None, None


def seg_loss(logits, labels, label_smoothing: float = 0.0, counted=None, n_valid: Optional[torch.Tensor] = None,
             tallies: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 0-dim float32 loss of ``SegLoss``.  ``counted``: a ``[classes]`` uint8 device tensor (nonzero: the class counts), or
    a sequence of the class ids that do NOT count (``counted_mask``), or None."""
    if counted is not None and not isinstance(counted, torch.Tensor):
        counted = counted_mask(logits.shape[-1], counted, logits.device)
    return SegLoss.apply(logits, labels, label_smoothing, counted, n_valid, tallies)


# ------------------------------------------------------------------------------- frames (row f-1)
KNN_GRID_MIN_POINTS = 8192 # below this the all-pairs scan is as fast as sorting into cells
KNN_CELL_FACTOR = 1.6       # cell size / estimated k-NN distance (1.26 covers points on a face of the cloud)


def _knn_cell_size(mn, mx, counts, k: int) -> torch.Tensor:
    """Cell size (device scalar): KNN_CELL_FACTOR x the k-NN distance a uniformly filled box of each batch element's extent
    would have -- the larger of the volume, area and length estimates, so flat and thin clouds are covered too.
    Only a speed knob: se3_knn_query_grid is exact for any cell size."""
    ext = (mx - mn).clamp_min(0).sort(dim=1, descending=True)[0]
    cnt = counts.clamp_min(1).to(torch.float32)
    e1, e2, e3 = ext[:, 0], ext[:, 1], ext[:, 2]
    c_vol = (k * e1 * e2 * e3 / (4.19 * cnt)).pow(1.0 / 3.0)
    c_area = (k * e1 * e2 / (3.14 * cnt)).sqrt()
    c_len = k * e1 / (2.0 * cnt)
    c = KNN_CELL_FACTOR * torch.stack([c_vol, c_area, c_len]).max()
    return torch.maximum(c, (e1.max() * 1e-6).clamp_min(1e-30))


def knn_query(pts, batch_ids, k: int, n_batches: Optional[int] = None, method: str = "auto", box=None,
              n_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``point_cloud_lib_ops.knn_query``: self-kNN inside each batch element, ``[N,k]`` int32 (self first,
    ascending distance, ties to the lower index, -1 padded).  ``method``: "grid" (cell grid + exact fallback),
    "scan" (all pairs inside the batch element) or "auto" (grid from KNN_GRID_MIN_POINTS points on).  ``box``: the
    cloud's ``batch_aabb`` result when the caller has it (``Pointcloud.aabb()``).  ``n_valid`` (int32 device word): a
    padded cloud (``se3_knn_query_padded``) -- the present rows' neighbours are those of the call on the present rows alone,
    absent rows get -1; the cell-grid search then needs ``n_batches``."""
    lib = _lib.load()
    if n_valid is not None:
        _padded_cloud(pts, batch_ids, "knn_query")
    pts = _as(pts, torch.float32)
    b = _as(batch_ids, torch.int32)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("knn_query: only [N,3] point sets are supported")
    if method not in ("auto", "grid", "scan"):
        raise ValueError(f"knn_query: unknown method {method!r}")
    n, dev = pts.shape[0], pts.device
    out = _empty((n, int(k)), dtype=torch.int32, device=dev)
    f32, i32 = torch.float32, torch.int32
    if not 1 <= int(k) <= 64:
        raise ValueError(f"knn_query: k = {k}; the kernels keep at most 64 neighbours per point (the reference's own "
                         "kernel has the same limit, knn_query.cu:167)")
    if method == "grid" and k > 32:
        raise ValueError("knn_query: the cell-grid search keeps at most 32 neighbours; use method='scan' or 'auto'")
    padded = n_valid is not None
    mid = (_valid_word(n_valid, dev, "knn_query"),) if padded else ()  # the padded entry points take the word behind the row count
    p_pts, p_b, p_out, stream = _ptr(pts, f32, "pts"), _ptr(b, i32, "batch_ids", dev), _ptr(out, i32, "out"), _stream(dev)

    def search(mn, num_cells, cell3, ws):
        """The search itself: through the cell grid with its parameters and workspace, all pairs with None."""
        grid = [_ptr(t, dt, name) for t, dt, name in ((mn, f32, "aabb_min"), (num_cells, i32, "num_cells"), (cell3, f32, "cell_size"))]
        space = (C.c_void_p(ws.data_ptr() if ws is not None else 0), ws.numel() if ws is not None else 0)
        if padded:
            _lib.check(lib.se3_knn_query_padded(p_pts, p_b, n, *mid, *grid, int(k), p_out, *space, stream), "se3_knn_query_padded")
        elif mn is None:
            _lib.check(lib.se3_knn_query(p_pts, p_b, n, int(k), p_out, stream), "se3_knn_query")
        else:
            _lib.check(lib.se3_knn_query_grid(p_pts, p_b, *grid, n, int(k), p_out, *space, stream), "se3_knn_query_grid")
        return out

    if method == "scan" or (method == "auto" and (n < KNN_GRID_MIN_POINTS or k > 32)) or n == 0:
        return search(None, None, None, None)
    if padded and box is None and n_batches is None:
        raise ValueError("knn_query: the cell-grid search of a padded cloud needs n_batches or the cloud's boxes")
    # boxes, then cell size / shifted minima / cell counts in ONE launch (se3_knn_grid_params: what _knn_cell_size and the
    # lines of BallQuery.py:34-38 compute -- as a dozen torch calls and a bincount they cost more than the search)
    box_mn, mx = box if box is not None else batch_aabb(pts, b, n_batches, n_valid)
    nb = box_mn.shape[0]
    mn = _empty((nb, 3), dtype=f32, device=dev)
    num_cells = _empty(3, dtype=i32, device=dev)
    cell3 = _empty(3, dtype=f32, device=dev)
    params = "se3_knn_grid_params_padded" if padded else "se3_knn_grid_params"
    _lib.check(getattr(lib, params)(p_b, n, *mid, _ptr(box_mn, f32, "box_min", dev), _ptr(mx, f32, "box_max", dev), nb, int(k),
                                    float(KNN_CELL_FACTOR), _ptr(mn, f32, "aabb_min"), _ptr(num_cells, i32, "num_cells"),
                                    _ptr(cell3, f32, "cell_size"), stream), params)
    ws_bytes = lib.se3_knn_query_padded_workspace_bytes(n, 1) if padded else lib.se3_knn_query_grid_workspace_bytes(n)
    return search(mn, num_cells, cell3, _workspace(ws_bytes, dev))


def knn_query_pair(pts_src, batch_src, pts_q, batch_q, k: int, n_valid_src: Optional[torch.Tensor] = None,
                   n_valid_q: Optional[torch.Tensor] = None) -> torch.Tensor:
    """For every query point the ``k`` nearest SOURCE points of the same batch element: ``[N_q, k]`` int32 source
    indices, ascending (distance, index), -1 padded (``se3_knn_query_pair``; the ``torch_cluster.knn`` call of
    pc/KnnNeighborhood.py:77-84).  Both batch-id arrays sorted; k <= 64.  ``n_valid_src`` / ``n_valid_q`` (int32 device
    words, either may be None = every row): PADDED clouds (``se3_knn_query_pair_padded``, include/se3conv_knn_edges.h) --
    present queries get what the call on the present rows alone gives, absent queries -1 in every column, no absent row of
    either cloud is read; the buffers are then taken as they are (float32 / int32, contiguous)."""
    lib = _lib.load()
    f32, i32 = torch.float32, torch.int32
    padded = n_valid_src is not None or n_valid_q is not None
    if padded:
        _padded_cloud(pts_src, batch_src, "knn_query_pair")
        _padded_cloud(pts_q, batch_q, "knn_query_pair")
    ps, pq = _as(pts_src, f32), _as(pts_q, f32)
    bs, bq = _as(batch_src, i32), _as(batch_q, i32)
    if ps.dim() != 2 or ps.shape[1] != 3 or pq.dim() != 2 or pq.shape[1] != 3:
        raise ValueError("knn_query_pair: only [N,3] point sets are supported")
    if not 1 <= int(k) <= 64:
        raise ValueError(f"knn_query_pair: k = {k}; at most 64 neighbours per point")
    dev = pq.device
    out = _empty((pq.shape[0], int(k)), dtype=i32, device=dev)
    if padded:
        _lib.check(lib.se3_knn_query_pair_padded(
            _ptr(ps, f32, "pts_src", dev), _ptr(bs, i32, "batch_src", dev), ps.shape[0], _valid_word(n_valid_src, dev, "knn_query_pair"),
            _ptr(pq, f32, "pts_q"), _ptr(bq, i32, "batch_q", dev), pq.shape[0], _valid_word(n_valid_q, dev, "knn_query_pair"),
            int(k), _ptr(out, i32, "out"), _stream(dev)), "se3_knn_query_pair_padded")
        return out
    _lib.check(lib.se3_knn_query_pair(_ptr(ps, f32, "pts_src", dev), _ptr(bs, i32, "batch_src", dev), ps.shape[0],
                                      _ptr(pq, f32, "pts_q"), _ptr(bq, i32, "batch_q", dev), pq.shape[0], int(k),
                                      _ptr(out, i32, "out"), _stream(dev)), "se3_knn_query_pair")
    return out


def knn_edges_bounded(ids: torch.Tensor, capacity: int, n_valid: Optional[torch.Tensor] = None,
                      neighbors_out: Optional[torch.Tensor] = None):
    """The edge list of a k-NN id table without a read-back (``se3_knn_edges_bounded``, include/se3conv_knn_edges.h).
    ``ids [n, k]`` int32 as ``knn_query`` / ``knn_query_pair`` write it (the valid entries of a row are a prefix, -1 behind
    them); ``n_valid`` (int32 device word): rows from it on are absent and have no edges.  Returns ``(neighbors
    [capacity,2] int32, ends [n] int32, info [2] int32 on the device)`` as ``ball_query_bounded`` does: sample-major
    ``(row, id)`` pairs in table order, inclusive end offsets, ``info = (true edge count, overflow flag)``; on overflow
    the head of the list is kept and ``ends`` clamped.  Rows of ``neighbors`` past the edge count are unset.  ``n * k`` is
    the capacity that cannot overflow.  ``neighbors_out``: a caller-owned contiguous ``[capacity, 2]`` int32 buffer to write
    into instead of a fresh allocation.  No host synchronisation: capturable."""
    lib = _lib.load()
    i32 = torch.int32
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.shape[1] < 1:
        raise ValueError("knn_edges_bounded: ids is an [n, k] table")
    if not 1 <= ids.shape[1] <= 64:
        raise ValueError(f"knn_edges_bounded: k = {ids.shape[1]}; at most 64 neighbours per point")
    if capacity is None or int(capacity) < 0:
        raise ValueError("knn_edges_bounded: capacity must be non-negative")
    n, k, dev = ids.shape[0], ids.shape[1], ids.device
    p_ids = _ptr(ids, i32, "ids")  # (taken as it is: a conversion would read the absent rows)
    if neighbors_out is not None:
        if neighbors_out.shape != (int(capacity), 2) or neighbors_out.dtype != i32 or not neighbors_out.is_contiguous():
            raise ValueError(f"neighbors_out must be a contiguous int32 [{int(capacity)}, 2] tensor")
        neighbors = neighbors_out
    else:
        neighbors = _empty((int(capacity), 2), dtype=i32, device=dev)
    ends = _empty(n, dtype=i32, device=dev)
    info = _empty(2, dtype=i32, device=dev)
    ws = _workspace(lib.se3_knn_edges_workspace_bytes(n), dev)
    _lib.check(lib.se3_knn_edges_bounded(p_ids, n, _valid_word(n_valid, dev, "knn_edges_bounded"), k, int(capacity),
                                         _ptr(neighbors, i32, "neighbors"), _ptr(ends, i32, "ends"), _ptr(info, i32, "info"),
                                         C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)), "se3_knn_edges_bounded")
    return neighbors, ends, info


class KNNQuery(torch.autograd.Function):
    """Drop-in for ``point_cloud_lib.custom_ops.KNNQuery`` (KNNQuery.py:11-35)."""

    @staticmethod
    def forward(ctx, p_pt_src, p_batch_id_src, p_k):
        return knn_query(p_pt_src, p_batch_id_src, p_k)

    @staticmethod
    def backward(ctx, grad):
        return None, None, None


def pca_frames(pts, knn_ids, axis_fixed=None, n_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sample_reference_frames_pca`` on the GPU: ``[N,4,9]`` frames (``[N,2,9]`` with a fixed axis 1 or 2).
    ``axis_fixed`` follows the reference: ``None`` / ``False`` / ``0`` all mean "not fixed".  ``n_valid`` (int32 device
    word): a padded cloud (``se3_pca_frames_padded``) -- absent rows get the identity in every copy and are not read."""
    lib = _lib.load()
    if n_valid is not None:
        _ptr(pts, torch.float32, "pts")
        _ptr(knn_ids, torch.int32, "knn", pts.device)
    pts = _as(pts, torch.float32)
    ids = _as(knn_ids, torch.int32)
    n, k = ids.shape
    axis = int(axis_fixed) if axis_fixed else -1
    if axis not in (-1, 1, 2):
        raise ValueError(f"axis_fixed = {axis_fixed}")
    nf = 4 if axis < 0 else 2
    frames = _empty((n, nf, 9), dtype=torch.float32, device=pts.device)
    if n_valid is not None:
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] != n:
            raise ValueError(f"pca_frames: {tuple(pts.shape)} points for {n} rows of neighbour ids")
        _lib.check(lib.se3_pca_frames_padded(_ptr(pts, torch.float32, "pts"), _ptr(ids, torch.int32, "knn", pts.device), n,
                                             _valid_word(n_valid, pts.device, "pca_frames"), k, axis,
                                             _ptr(frames, torch.float32, "frames"), _stream(pts.device)), "se3_pca_frames_padded")
        return frames
    _lib.check(lib.se3_pca_frames(_ptr(pts, torch.float32, "pts"), _ptr(ids, torch.int32, "knn", pts.device), n, k, axis,
                                  _ptr(frames, torch.float32, "frames"), _stream(pts.device)), "se3_pca_frames")
    return frames


def shuffle_frames(all_frames, n_frames: int, draws=None) -> torch.Tensor:
    """``n_frames`` of each point's frames in a uniformly random order (``se3_shuffle_frames``; the ``torch.multinomial``
    + gather of PointcloudRotEquiv.py:100-117, 146-167).  ``draws`` ``[N, n_all]`` uniform numbers (``torch.rand`` on
    the device by default)."""
    lib = _lib.load()
    all_frames = _as(all_frames, torch.float32)
    n, n_all = all_frames.shape[0], all_frames.shape[1]
    dev = all_frames.device
    if draws is None:
        draws = torch.rand((n, n_all), device=dev)
    draws = _as(draws, torch.float32)
    if tuple(draws.shape) != (n, n_all):
        raise ValueError(f"shuffle_frames: draws {tuple(draws.shape)}, expected {(n, n_all)}")
    out = _empty((n, int(n_frames), all_frames.shape[2]), dtype=torch.float32, device=dev)
    if all_frames.shape[2] != 9:
        raise ValueError("shuffle_frames: frames are [N, n_all, 9]")
    _lib.check(lib.se3_shuffle_frames(_ptr(all_frames, torch.float32, "all_frames"), _ptr(draws, torch.float32, "draws", dev), n,
                                      n_all, int(n_frames), _ptr(out, torch.float32, "out"), _stream(dev)), "se3_shuffle_frames")
    return out


# ------------------------------------------------------------------- the operator's geometry bundle
class PreparedRecords:
    """The packed 64-byte geometry records of one cloud (include/se3conv.h, struct se3conv_prepared): a function of the
    cloud's points and frames alone, so every convolution that touches the cloud -- forward and backward, every layer of a
    level -- shares one image.  The first call that meets an invalid holder fills it inside its own preparation launch.
    Kept on the cloud object (``prepared_records``); re-validated against the tensors' storage and version counters.
    ``valid`` is for eager calls; inside a HIP graph capture the records count as filled only when a call of the SAME
    capture filled them (``capture``: its id), and such a fill is not one for eager calls (it runs at replay)."""

    __slots__ = ("tensor", "valid", "key", "capture")

    def __init__(self):
        self.tensor, self.valid, self.key, self.capture = None, False, None, None

    def bind(self, pts: torch.Tensor, frames: torch.Tensor) -> "PreparedRecords":
        key = (pts.data_ptr(), version_key(pts), frames.data_ptr(), version_key(frames), tuple(frames.shape),
               str(pts.device))
        if key != self.key:
            rows = frames.shape[0] * frames.shape[1]
            if self.tensor is None or self.tensor.shape[0] != rows or self.tensor.device != pts.device:
                self.tensor = _empty((rows, 16), dtype=torch.float32, device=pts.device)
            self.key, self.valid, self.capture = key, False, None
        return self

    def filled_for(self, capture: Optional[int]) -> bool:
        """Whether a call made outside a capture (``capture`` None) or inside capture ``capture`` may read the records."""
        return self.valid if capture is None else self.capture == capture

    def mark_filled(self, capture: Optional[int]) -> None:
        if capture is None:
            self.valid = True
        else:
            self.valid, self.capture = False, capture


def prepared_records(cloud) -> Optional["PreparedRecords"]:
    """The holder of ``cloud``'s geometry records, created on first use and kept on the object (any object that takes an
    attribute: the reference's own containers and plain namespaces too); None when it cannot be attached."""
    holder = getattr(cloud, "_se3_records_", None)
    if holder is None:
        holder = PreparedRecords()
        try:
            cloud._se3_records_ = holder
        except (AttributeError, TypeError):
            return None
    return holder


def invalidate_prepared(cloud) -> None:
    """Forget the cloud's prepared records (the next convolution that touches the cloud rebuilds them): what a new step
    does implicitly by building new cloud objects; a benchmark that re-uses its clouds calls this once per step."""
    holder = getattr(cloud, "_se3_records_", None)
    if holder is not None:
        holder.valid, holder.capture = False, None


@functools.lru_cache(maxsize=1)
def _hip_get_capture_info():
    fn = C.CDLL("libamdhip64.so").hipStreamGetCaptureInfo  # the runtime torch has already loaded
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
    fn.restype = C.c_int
    return fn


def _stream_capture_id(device) -> int:
    """Id of the capture sequence the current stream of ``device`` belongs to (``hipStreamGetCaptureInfo``)."""
    status, cid = C.c_int(0), C.c_ulonglong(0)
    err = _hip_get_capture_info()(_stream(device), C.byref(status), C.byref(cid))
    if err != 0 or status.value != 1:  # hipStreamCaptureStatusActive
        raise RuntimeError(f"hipStreamGetCaptureInfo: error {err}, capture status {status.value} on a capturing stream")
    return int(cid.value)


def _capture_id(device) -> Optional[int]:
    """None outside a HIP graph capture; the capture's id while the current stream of ``device`` is being captured."""
    if device.type != "cuda" or not torch.cuda.is_current_stream_capturing():
        return None
    return _stream_capture_id(device)


@dataclass
class ConvGeometry:
    """Everything the operator reads besides features and parameters (all fp32 / int32, GPU)."""

    pts_in: torch.Tensor       # [N_in,3]
    pts_out: torch.Tensor      # [N_out,3]
    frames_in: torch.Tensor    # [N_in,F_in,9]
    frames_out: torch.Tensor   # [N_out,F_out,9]
    neighbors: torch.Tensor    # [E,2] int32
    ends: torch.Tensor         # [N_out] int32
    _transpose: Optional[Tuple[torch.Tensor, torch.Tensor]] = field(default=None, repr=False)
    # the edge relation is symmetric (a radius graph of a cloud with itself: ||s - p|| < r both ways, bit for bit):
    # the source-major edge list is then the sample-major one read the other way round, nothing to build
    symmetric: bool = False
    bounded: bool = False  # `neighbors` is a capacity-sized buffer whose rows past ends[-1] are unset
    sources: Optional[torch.Tensor] = None  # column 1 of `neighbors` as a dense array when the ball query wrote one
    edge_info: Optional[torch.Tensor] = None  # [2] int32 on the device (bounded only): true edge count, overflow flag
    # the neighbourhood's own way to the source-major list (pc.BQNeighborhood.source_major), or None
    source_major_fn: Optional[Callable[[], Optional[Tuple[torch.Tensor, torch.Tensor]]]] = field(default=None, repr=False)
    _edge_ids: Optional[torch.Tensor] = field(default=None, repr=False)  # third result of the library's transposition, if it built the list
    # holders of the clouds' packed geometry records (the same object for a cloud against itself), or None
    records_in: Optional[PreparedRecords] = field(default=None, repr=False)
    records_out: Optional[PreparedRecords] = field(default=None, repr=False)

    @staticmethod
    def build(pts_in, pts_out, frames_in, frames_out, neighbors, ends, symmetric: bool = False) -> "ConvGeometry":
        n_out = pts_out.shape[0]
        ends = _as(ends, torch.int32)
        if ends.shape[0] != n_out:
            raise ValueError(f"start_ids has {ends.shape[0]} entries, expected one per output point ({n_out})")
        fi = _as(frames_in, torch.float32).reshape(pts_in.shape[0], -1, 9)
        fo = _as(frames_out, torch.float32).reshape(n_out, -1, 9)
        nb = _as(neighbors, torch.int32)
        if nb.dim() != 2 or nb.shape[1] != 2:
            raise ValueError("neighbors must be [E,2]")
        if symmetric and pts_in.shape[0] != n_out:
            raise ValueError("a symmetric neighbourhood needs the same cloud on both sides")
        return ConvGeometry(_as(pts_in, torch.float32), _as(pts_out, torch.float32), fi, fo, nb, ends, None, symmetric)

    def transpose(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Source-major edge list ``(t_samples [E], t_ends [N_in])`` for the feature gradient."""
        if self._transpose is None:
            if self.symmetric:  # samples of source p = sources of sample p
                src = self.sources if self.sources is not None else self.neighbors[:, 1].contiguous()
                self._transpose = (src, self.ends)
            elif self.source_major_fn is not None and (own := self.source_major_fn()) is not None:
                self._transpose = own
            else:
                if self.bounded and self.edge_info is None:
                    raise ValueError("a capacity-bounded edge buffer between two clouds needs its device-side edge count "
                                     "(edge_info) to be transposed: rows past it are unset")
                # bounded: the unset tail of the buffer must not reach the sort (se3_csr_transpose_bounded)
                ts, te, self._edge_ids = csr_transpose(self.neighbors, self.pts_in.shape[0],
                                                       self.edge_info if self.bounded else None, want_edge_ids=True)
                self._transpose = (ts, te)
        return self._transpose

    def shape(self, c_in: int, c_out: int, num_basis: int, precision: Optional[str] = None) -> Se3Shape:
        # n_edges = rows of the edge buffer: an upper bound on the edge count for a bounded neighbourhood (se3conv.h)
        return Se3Shape(self.pts_in.shape[0], self.pts_out.shape[0], self.neighbors.shape[0],
                        self.frames_in.shape[1], self.frames_out.shape[1], c_in, c_out, num_basis,
                        _lib.PRECISIONS[precision or _precision])


def _geom_ptrs(g: ConvGeometry):
    f32, i32 = torch.float32, torch.int32
    dev = g.pts_out.device
    return [_ptr(g.pts_in, f32, "pts_in", dev), _ptr(g.pts_out, f32, "pts_out", dev),
            _ptr(g.frames_in, f32, "frames_in", dev), _ptr(g.frames_out, f32, "frames_out", dev),
            _ptr(g.neighbors, i32, "neighbors", dev), _ptr(g.ends, i32, "ends", dev)]


def _same_cloud(g: ConvGeometry) -> bool:
    """The library's own test (api.hip, ``same_cloud``): one set of records serves both sides and ``geom_out`` is not
    written -- whichever cloud objects, and hence holders, the two sides came from."""
    return (g.pts_in.data_ptr() == g.pts_out.data_ptr() and g.frames_in.data_ptr() == g.frames_out.data_ptr()
            and g.pts_in.shape[0] == g.pts_out.shape[0] and g.frames_in.shape[1] == g.frames_out.shape[1])


def _prepared(geom: ConvGeometry, feat_words: Optional[torch.Tensor], feat_words_valid: bool):
    """struct se3conv_prepared of a call (or None), the holders the call fills, and the capture it is enqueued in (None
    outside one): once the call has been enqueued, ``h.mark_filled(capture)`` for each holder."""
    r_in, r_out = geom.records_in, geom.records_out
    if r_in is None and r_out is None and feat_words is None:
        return None, (), None
    p = _lib.Se3Prepared()
    filled = []
    capture = _capture_id(geom.pts_out.device) if (r_in is not None or r_out is not None) else None
    if _same_cloud(geom):
        r_out = None  # (the library reads the in-side records for both sides and never writes geom_out)
    if r_in is not None:
        r_in.bind(geom.pts_in, geom.frames_in)
        p.geom_in, p.geom_in_valid = r_in.tensor.data_ptr(), int(r_in.filled_for(capture))
        filled.append(r_in)
    if r_out is not None and r_out is not r_in:
        r_out.bind(geom.pts_out, geom.frames_out)
        p.geom_out, p.geom_out_valid = r_out.tensor.data_ptr(), int(r_out.filled_for(capture))
        filled.append(r_out)
    elif r_out is r_in and r_in is not None:
        p.geom_out, p.geom_out_valid = p.geom_in, 1  # (ignored for a cloud against itself; valid by the time it is read otherwise)
    if feat_words is not None:
        p.feat_words, p.feat_words_valid = feat_words.data_ptr(), int(feat_words_valid)
    return p, tuple(filled), capture


def _scalar(t, name, dev) -> torch.Tensor:
    t = torch.as_tensor(t, dtype=torch.float32)
    return t.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous()


def se3conv_forward(geom: ConvGeometry, feat, proj_axes, proj_biases, conv_weights, rho, nu, save_t: bool = True,
                    precision: Optional[str] = None, feat_words: Optional[torch.Tensor] = None):
    """Raw forward: returns ``(out [N_out*F_out, C_out], T or None)``.  ``T`` is fp32 in "fp32" precision
    and an opaque same-size buffer of packed hi/lo words in "bf16x3" (pass it back with the same precision).
    ``feat_words`` (int32, one word per feature, split-bf16 modes): receives the packed feature words for ``se3conv_backward``."""
    lib = _lib.load()
    f32 = torch.float32
    dev = geom.pts_out.device
    feat = _as(feat, f32)
    a, b, w = _as(proj_axes, f32), _as(proj_biases, f32), _as(conv_weights, f32)
    if a.shape[0] != 9:
        raise ValueError(f"proj_axes_ has {a.shape[0]} rows; only the 9-D ('6D') descriptor is implemented")
    c_in, kb, c_out = w.shape
    if feat.shape != (geom.pts_in.shape[0] * geom.frames_in.shape[1], c_in):
        raise ValueError(f"features are {tuple(feat.shape)}, expected "
                         f"({geom.pts_in.shape[0] * geom.frames_in.shape[1]}, {c_in})")
    shp = geom.shape(c_in, c_out, kb, precision)
    rows = geom.pts_out.shape[0] * geom.frames_out.shape[1]
    out = _empty((rows, c_out), dtype=f32, device=dev)
    # T is kept for the weight gradient only on the K = 32 kernels' own layout; other K run as slices of 32 inside the
    # library, which recomputes T in backward (include/se3conv.h)
    t_save = _empty((rows, c_in, kb), dtype=f32, device=dev) if (save_t and kb == 32) else None
    ws = _workspace(lib.se3conv_fwd_workspace_bytes(C.byref(shp), 1 if save_t else 0), dev)
    rho_t, nu_t = _scalar(rho, "rho", dev), _scalar(nu, "nu", dev)
    prep, filled, capture = _prepared(geom, feat_words, False)
    _lib.check(lib.se3conv_fwd_prepared(*_geom_ptrs(geom), _ptr(feat, f32, "features", dev), _ptr(a, f32, "proj_axes_", dev),
                                        _ptr(b, f32, "proj_biases_", dev), _ptr(w, f32, "conv_weights_", dev),
                                        _ptr(rho_t, f32, "norm_neigh_dist_"), _ptr(nu_t, f32, "norm_num_neighs_"),
                                        C.byref(shp), _ptr(out, f32, "out"), _ptr(t_save, f32, "t_save"),
                                        C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev),
                                        C.byref(prep) if prep is not None else None), "se3conv_fwd")
    for h in filled:
        h.mark_filled(capture)
    return out, t_save


def se3conv_backward(geom: ConvGeometry, feat, proj_axes, proj_biases, conv_weights, rho, nu, t_save, grad_out,
                     want_feat=True, want_params=True, precision: Optional[str] = None,
                     feat_words: Optional[torch.Tensor] = None):
    """Raw backward: returns ``(dX, dA, dbeta, dW)`` (None where not requested).  ``feat_words``: what the forward call of
    the same features wrote (see ``se3conv_forward``), or None."""
    lib = _lib.load()
    f32, i32 = torch.float32, torch.int32
    dev = geom.pts_out.device
    feat = _as(feat, f32)
    a, b, w = _as(proj_axes, f32), _as(proj_biases, f32), _as(conv_weights, f32)
    g = _as(grad_out, f32)
    c_in, kb, c_out = w.shape
    shp = geom.shape(c_in, c_out, kb, precision)
    d_x = _empty_like(feat) if want_feat else None
    d_a = _empty_like(a) if want_params else None
    d_b = _empty_like(b) if want_params else None
    d_w = _empty_like(w) if want_params else None
    t_samples, t_ends = geom.transpose() if want_feat else (None, None)
    ws = _workspace(lib.se3conv_bwd_workspace_bytes(C.byref(shp), int(want_feat), int(want_params),
                                                    int(t_save is not None)), dev)
    rho_t, nu_t = _scalar(rho, "rho", dev), _scalar(nu, "nu", dev)
    prep, filled, capture = _prepared(geom, feat_words, feat_words is not None)
    _lib.check(lib.se3conv_bwd_prepared(*_geom_ptrs(geom), _ptr(t_samples, i32, "t_samples"), _ptr(t_ends, i32, "t_ends"),
                                        _ptr(geom._edge_ids if want_feat else None, i32, "t_edge_ids"),
                                        _ptr(feat, f32, "features", dev), _ptr(a, f32, "proj_axes_", dev),
                                        _ptr(b, f32, "proj_biases_", dev), _ptr(w, f32, "conv_weights_", dev),
                                        _ptr(rho_t, f32, "rho"), _ptr(nu_t, f32, "nu"), _ptr(t_save, f32, "t_save"),
                                        _ptr(g, f32, "grad_out", dev), C.byref(shp), _ptr(d_x, f32, "grad_feat"),
                                        _ptr(d_a, f32, "grad_axes"), _ptr(d_b, f32, "grad_biases"),
                                        _ptr(d_w, f32, "grad_weights"), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev),
                                        C.byref(prep) if prep is not None else None), "se3conv_bwd")
    for h in filled:
        h.mark_filled(capture)
    return d_x, d_a, d_b, d_w


class SE3ConvFunction(torch.autograd.Function):
    """The fused operator as one autograd node (replaces the chain matmul -> GELU -> FeatBasisProj
    -> einsum -> scalings of PNEConvLayerRotEquiv.py:199-216).  Differentiable w.r.t. features and
    the three parameters; geometry carries no gradient (reference: built under no_grad, :67)."""

    @staticmethod
    def forward(ctx, feat, proj_axes, proj_biases, conv_weights, geom: ConvGeometry, rho, nu):
        need_params = any(ctx.needs_input_grad[1:4])
        ctx.precision = _precision
        save_t = need_params
        if save_t:
            # T ([rows, C_in, K]: 0.8 GB per layer at the headline shape, the largest activation a layer would keep) is only
            # saved where backward has a use for it: when the feature gradient is wanted too, the library takes the weight
            # gradient from U, the tensor its transposed pass produces anyway (se3conv_bwd_needs_t, include/se3conv.h)
            c_in, kb, c_out = conv_weights.shape
            shp = geom.shape(c_in, c_out, kb, ctx.precision)
            save_t = _lib.load().se3conv_bwd_needs_t(C.byref(shp), int(bool(ctx.needs_input_grad[0]))) != 0
        # the packed feature words of the split-bf16 modes go to backward with the features (the parameter gradients gather
        # them again): one split per step instead of two, for one more word per feature kept
        fw = None
        if need_params and ctx.precision != "fp32" and conv_weights.shape[1] == 32 and feat.is_cuda:
            fw = _empty(feat.numel(), dtype=torch.int32, device=feat.device)
        out, t_save = se3conv_forward(geom, feat, proj_axes, proj_biases, conv_weights, rho, nu,
                                      save_t=save_t, precision=ctx.precision, feat_words=fw)
        ctx.geom = geom
        ctx.in_dtype = feat.dtype
        ctx.save_for_backward(feat, proj_axes, proj_biases, conv_weights, _scalar(rho, "rho", out.device),
                              _scalar(nu, "nu", out.device), t_save if t_save is not None else torch.empty(0),
                              fw if fw is not None else torch.empty(0))
        ctx.has_t = t_save is not None
        ctx.has_fw = fw is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feat, a, b, w, rho, nu, t_save, fw = ctx.saved_tensors
        want_feat = ctx.needs_input_grad[0]
        want_params = any(ctx.needs_input_grad[1:4])
        d_x, d_a, d_b, d_w = se3conv_backward(ctx.geom, feat, a, b, w, rho, nu, t_save if ctx.has_t else None,
                                              grad_out, want_feat, want_params, precision=ctx.precision,
                                              feat_words=fw if ctx.has_fw else None)
        if d_x is not None:
            d_x = d_x.to(ctx.in_dtype)
        ng = ctx.needs_input_grad
        return (d_x, d_a if ng[1] else None, d_b if ng[2] else None, d_w if ng[3] else None, None, None, None)


# ------------------------------------------------------------------ API-parity ops (a1, a3, a4, a5)
def rot_tensors(geom: ConvGeometry, rho, rel_rot: str = "6D"):
    """``get_rot_tenors`` materialised on the GPU: ``desc [E',D]``, ``neighbs [E',2] int32`` sorted by
    output row, ``ends [N_out*F_out] int32``.  ``rel_rot`` = the factory's ``p_rel_rot``: "6D" (D = 9), "matrix"
    (D = 12) or "quaternion" (D = 7)."""
    lib = _lib.load()
    if rel_rot not in _lib.REL_ROT:
        raise ValueError(f"rel_rot {rel_rot!r}; expected one of {sorted(_lib.REL_ROT)}")
    mode, dims = _lib.REL_ROT[rel_rot]
    dev = geom.pts_out.device
    shp = geom.shape(1, 1, 32)
    ff = shp.f_in * shp.f_out
    e2 = geom.neighbors.shape[0] * ff
    desc = _empty((e2, dims), dtype=torch.float32, device=dev)
    fe_nb = _empty((e2, 2), dtype=torch.int32, device=dev)
    fe_ends = torch.zeros(geom.pts_out.shape[0] * shp.f_out, dtype=torch.int32, device=dev)
    rho_t = _scalar(rho, "rho", dev)
    _lib.check(lib.se3_rot_tensors_rel(*_geom_ptrs(geom), _ptr(rho_t, torch.float32, "rho"), C.byref(shp), mode,
                                       _ptr(desc, torch.float32, "desc"), _ptr(fe_nb, torch.int32, "fe_neighbors"),
                                       _ptr(fe_ends, torch.int32, "fe_ends"), _stream(dev)), "se3_rot_tensors_rel")
    return desc, fe_nb, fe_ends


class FeatBasisProj(torch.autograd.Function):
    """Drop-in for ``point_cloud_lib.custom_ops.FeatBasisProj`` (FeatBasisProj.py:4-65)."""

    @staticmethod
    def forward(p_ctx, p_pt_basis, p_pt_features, p_neighbors, p_start_ids):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        basis, feat = _as(p_pt_basis, f32), _as(p_pt_features, f32)
        nb, ends = _as(p_neighbors, i32), _as(p_start_ids, i32)
        p_ctx.save_for_backward(basis, feat, nb, ends)
        p_ctx.dtypes = (p_pt_basis.dtype, p_pt_features.dtype)
        dev = feat.device
        rows, ch, kb = ends.shape[0], feat.shape[1], basis.shape[1]
        out = _empty((rows, ch, kb), dtype=f32, device=dev)
        _lib.check(lib.se3_feat_basis_proj(_ptr(basis, f32, "pt_basis", dev), _ptr(feat, f32, "pt_features"),
                                           _ptr(nb, i32, "neighbors", dev), _ptr(ends, i32, "start_ids", dev),
                                           nb.shape[0], rows, feat.shape[0], ch, kb, _ptr(out, f32, "out"),
                                           _stream(dev)), "se3_feat_basis_proj")
        return out

    @staticmethod
    def backward(p_ctx, p_grads):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        basis, feat, nb, ends = p_ctx.saved_tensors
        g = _as(p_grads, f32)
        dev = feat.device
        g_feat = _empty_like(feat)
        g_basis = _empty_like(basis)
        _lib.check(lib.se3_feat_basis_proj_grad(
            _ptr(basis, f32, "pt_basis", dev), _ptr(feat, f32, "pt_features"), _ptr(nb, i32, "neighbors"),
            _ptr(ends, i32, "start_ids"), _ptr(g, f32, "grads", dev), nb.shape[0], ends.shape[0], feat.shape[0],
            feat.shape[1], basis.shape[1], _ptr(g_feat, f32, "g_feat"), _ptr(g_basis, f32, "g_basis"), _stream(dev)),
            "se3_feat_basis_proj_grad")
        return g_basis.to(p_ctx.dtypes[0]), g_feat.to(p_ctx.dtypes[1]), None, None


# ------------------------------------------- point-neighbourhood embeddings and max aggregation (include/se3conv_pne.h)
def _pne_call(kind: str, kpts, sigma):
    """enum value, kernel points, their count and sigma as the entry points of se3conv_pne.h take them."""
    if kind not in _lib.PNE_KINDS:
        raise ValueError(f"embedding kind {kind!r}; expected one of {sorted(_lib.PNE_KINDS)}")
    if not kind.startswith("kp_"):
        return _lib.PNE_KINDS[kind], None, 0, 0.0
    if kpts is None or kpts.dim() != 2 or kpts.shape[1] != 3 or not 1 <= kpts.shape[0] <= _lib.PNE_MAX_KPTS:
        raise ValueError(f"{kind}: kernel points are [J,3] with 1 <= J <= {_lib.PNE_MAX_KPTS}")
    return _lib.PNE_KINDS[kind], _as(kpts, torch.float32), kpts.shape[0], float(sigma)


class PneEmbed(torch.autograd.Function):
    """``phi [E,K]`` of ``se3_pne_embed_fwd``: the embedding of every edge's relative position, activation included --
    ``kind`` is a key of ``_lib.PNE_KINDS`` ("mlp_linear", "mlp_relu", "mlp_gelu", "mlp_sin", "mlp_softmax", "kp_gauss",
    "kp_linear", "kp_box").  Gradients go to ``proj_axes`` and ``proj_biases`` only, as in the reference."""

    @staticmethod
    def forward(ctx, pts, samples, neighbors, proj_axes, proj_biases, norm_dist, kind, kpts=None, sigma=0.0):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        code, kp, n_kp, sig = _pne_call(kind, kpts, sigma)
        x, y, nb = _as(pts, f32), _as(samples, f32), _as(neighbors, i32)
        a, b = _as(proj_axes, f32), _as(proj_biases, f32).reshape(-1)
        dev = x.device
        if x.dim() != 2 or x.shape[1] != 3 or y.dim() != 2 or y.shape[1] != 3:
            raise ValueError("PneEmbed: only [N,3] point sets are supported")
        if nb.dim() != 2 or nb.shape[1] != 2:
            raise ValueError("neighbors must be [E,2]")
        k = b.shape[0]
        if tuple(a.shape) != ((n_kp if kp is not None else 3), k):
            raise ValueError(f"{kind}: proj_axes of shape {tuple(a.shape)}, expected {((n_kp if kp is not None else 3), k)}")
        rho = _scalar(norm_dist, "norm_dist", dev)
        phi = _empty((nb.shape[0], k), dtype=f32, device=dev)
        _lib.check(lib.se3_pne_embed_fwd(_ptr(x, f32, "pts"), _ptr(y, f32, "samples", dev), _ptr(nb, i32, "neighbors", dev),
                                         nb.shape[0], _ptr(rho, f32, "norm_dist"), code, _ptr(kp, f32, "kernel_pts", dev), n_kp,
                                         sig, _ptr(a, f32, "proj_axes", dev), _ptr(b, f32, "proj_biases", dev), k,
                                         _ptr(phi, f32, "phi"), _stream(dev)), "se3_pne_embed_fwd")
        ctx.save_for_backward(x, y, nb, a, b, rho, *(() if kp is None else (kp,)))
        ctx.call = (code, n_kp, sig, proj_axes.dtype, proj_biases.dtype, tuple(proj_biases.shape))
        return phi

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        x, y, nb, a, b, rho, *rest = ctx.saved_tensors
        kp = rest[0] if rest else None
        code, n_kp, sig, dt_a, dt_b, shape_b = ctx.call
        g = _as(g, f32)
        dev = x.device
        k = b.shape[0]
        d_a, d_b = _empty_like(a), _empty_like(b)
        ws = _workspace(lib.se3_pne_embed_workspace_bytes(nb.shape[0], code, n_kp, k), dev)
        _lib.check(lib.se3_pne_embed_bwd(_ptr(g, f32, "grad_phi", dev), _ptr(x, f32, "pts"), _ptr(y, f32, "samples"),
                                         _ptr(nb, i32, "neighbors"), nb.shape[0], _ptr(rho, f32, "norm_dist"), code,
                                         _ptr(kp, f32, "kernel_pts"), n_kp, sig, _ptr(a, f32, "proj_axes"),
                                         _ptr(b, f32, "proj_biases"), k, _ptr(d_a, f32, "dA"), _ptr(d_b, f32, "dbeta"),
                                         C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)), "se3_pne_embed_bwd")
        return None, None, None, d_a.to(dt_a), d_b.reshape(shape_b).to(dt_b), None, None, None, None


class LinearPNE(torch.autograd.Function):
    """Drop-in for ``point_cloud_lib.custom_ops.LinearPNE`` (PNE.py:3-61): ``rho (x_src - y_smp) @ A + b`` per edge."""

    @staticmethod
    def forward(p_ctx, p_pts, p_samples, p_neighbors, p_proj_axes, p_proj_biases, p_norm_dist):
        return PneEmbed.forward(p_ctx, p_pts, p_samples, p_neighbors, p_proj_axes, p_proj_biases, p_norm_dist, "mlp_linear")

    @staticmethod
    def backward(p_ctx, p_grads):
        return PneEmbed.backward(p_ctx, p_grads)[:6]


class KPPNE(torch.autograd.Function):
    """Drop-in for ``point_cloud_lib.custom_ops.KPPNE`` (PNE.py:64-164): the correlation of every edge with the kernel points
    (``p_corr_func`` "gauss", "linear" or "box"), projected by ``p_proj_axes [J,K]``."""

    @staticmethod
    def forward(p_ctx, p_pts, p_samples, p_neighbors, p_kpts, p_sigma, p_proj_axes, p_proj_biases, p_norm_dist, p_corr_func):
        if p_corr_func not in ("gauss", "linear", "box"):
            raise ValueError(f"correlation function {p_corr_func!r}; expected 'gauss', 'linear' or 'box'")
        return PneEmbed.forward(p_ctx, p_pts, p_samples, p_neighbors, p_proj_axes, p_proj_biases, p_norm_dist,
                                "kp_" + p_corr_func, p_kpts, p_sigma)

    @staticmethod
    def backward(p_ctx, p_grads):
        g = PneEmbed.backward(p_ctx, p_grads)
        return None, None, None, None, None, g[3], g[4], None, None


def neigh_transposition(neighbors_i32: torch.Tensor, n_src: int, cache=None):
    """``(t_samples, t_ends, t_edge_ids)`` of ``se3_csr_transpose`` for ``NeighConvMax``; with ``cache`` (the neighbourhood
    object) built once and kept on it, as the convolution's backward keeps its own on the geometry."""
    key = (neighbors_i32.data_ptr(), neighbors_i32.shape[0], int(n_src))
    held = getattr(cache, "_se3_max_transpose", None) if cache is not None else None
    if held is not None and held[0] == key:
        return held[1]
    tr = csr_transpose(neighbors_i32, int(n_src), want_edge_ids=True)
    if cache is not None:
        try:
            cache._se3_max_transpose = (key, tr)
        except AttributeError:
            pass
    return tr


class NeighConvMax(torch.autograd.Function):
    """``out[m,o] = max_e sum_k phi[e,k] G[src_e,k,o]`` over the edges of sample ``m`` (``se3_neigh_max_fwd``): the reference's
    ``TransformNeighConv`` + ``scatter_max`` on transformed features ``G [N,K,C_out]`` (``feat @ W.reshape(C_in, K * C_out)``), which
    costs ``K * C_out`` per edge and never forms an ``E x C_in x C_out`` kernel.  Always ``M = len(ends)`` rows; a sample without edges
    gets zeros.  ``cache``: an object (the neighbourhood) that keeps the source-major transposition the backward needs."""

    @staticmethod
    def forward(ctx, phi, G, neighbors, ends, n_src, cache=None):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        ph, g3 = _as(phi, f32), _as(G, f32)
        nb, en = _as(neighbors, i32), _as(ends, i32)
        dev = ph.device
        e, k = ph.shape
        if g3.dim() != 3 or g3.shape[0] != int(n_src) or g3.shape[1] != k:
            raise ValueError(f"NeighConvMax: G of shape {tuple(g3.shape)}, expected [{int(n_src)}, {k}, C_out]")
        if nb.dim() != 2 or nb.shape[1] != 2 or nb.shape[0] != e:
            raise ValueError("neighbors must be [E,2], one row per row of phi")
        m, c = en.shape[0], g3.shape[2]
        out = _empty((m, c), dtype=f32, device=dev)
        arg = _empty((m, c), dtype=i32, device=dev)
        _lib.check(lib.se3_neigh_max_fwd(_ptr(ph, f32, "phi"), _ptr(g3, f32, "G", dev), _ptr(nb, i32, "neighbors", dev),
                                         _ptr(en, i32, "ends", dev), e, m, int(n_src), k, c, _ptr(out, f32, "out"),
                                         _ptr(arg, i32, "arg"), _stream(dev)), "se3_neigh_max_fwd")
        ctx.save_for_backward(ph, g3, nb, en, arg)
        ctx.cache, ctx.dtypes = cache, (phi.dtype, G.dtype)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g, _g_arg=None):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        ph, g3, nb, en, arg = ctx.saved_tensors
        g = _as(g, f32)
        dev = ph.device
        e, k = ph.shape
        n_src, c = g3.shape[0], g3.shape[2]
        if e:
            ts, te, tid = neigh_transposition(nb, n_src, ctx.cache)
        else:  # nothing to transpose: every source has no incoming edge
            ts, te, tid = None, torch.zeros(n_src, dtype=i32, device=dev), None
        dphi, dg = _empty_like(ph), _empty_like(g3)
        _lib.check(lib.se3_neigh_max_bwd(_ptr(g, f32, "grad_out", dev), _ptr(arg, i32, "arg"), _ptr(ph, f32, "phi"),
                                         _ptr(g3, f32, "G"), _ptr(nb, i32, "neighbors"), _ptr(en, i32, "ends"),
                                         _ptr(ts, i32, "t_samples"), _ptr(te, i32, "t_ends"), _ptr(tid, i32, "t_edge_ids"), e,
                                         en.shape[0], n_src, k, c, _ptr(dphi, f32, "dphi"), _ptr(dg, f32, "dG"), _stream(dev)),
                   "se3_neigh_max_bwd")
        return dphi.to(ctx.dtypes[0]), dg.to(ctx.dtypes[1]), None, None, None, None


# ------------------------------------------- attention over the basis functions (include/se3conv_basis_att.h)
def _key_rows(key: torch.Tensor, v: int) -> Tuple[torch.Tensor, int]:
    """``key [N,V]`` as the library reads it and its row stride in floats: a float32 view with unit inner stride (the last
    third of a ``[N,3V]`` projection) is passed as it is, anything else is made contiguous."""
    k = key.detach()
    if k.dtype == torch.float32 and k.dim() == 2 and k.stride(1) == 1 and k.stride(0) >= v and k.shape[0] > 1:
        return k, k.stride(0)
    return k.to(torch.float32).contiguous(), v


class BasisAttention(torch.autograd.Function):
    """The attention stage of ``MultiHeadAttLayer`` / ``LoRAttConvLayer`` (``se3_basis_att_fwd`` / ``_bwd``): with ``T [N,2V,K]`` as
    ``FeatBasisProj`` gives it for ``2V`` channels (value rows first, query rows second), ``key [N,V]`` and ``pe [K,V]`` or ``[1,K,V]``,

        s[n,k,h] = sum_{i in head h} (Tq[n,i,k] + pe[k,i]) * key[n,i],   att = softmax_k(s),   out[n,i] = sum_k Tv[n,i,k] * att[n,k,h(i)]

    and returns ``out [N,V]`` (no ``1/sqrt(D)``, as the reference).  Gradients go to ``T``, ``key`` and ``pe``.  ``T`` is read in its own
    layout: no transposed copy and no ``N x K x V`` intermediate."""

    @staticmethod
    def forward(ctx, T, key, pe, num_heads):
        lib = _lib.load()
        f32 = torch.float32
        for name, x in (("T", T), ("key", key), ("pe", pe)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise ValueError(f"BasisAttention: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
        t = _as(T, f32)
        if t.dim() != 3 or t.shape[1] % 2:
            raise ValueError(f"BasisAttention: T of shape {tuple(T.shape)}, expected [N, 2V, K]")
        n, v, k = t.shape[0], t.shape[1] // 2, t.shape[2]
        h = int(num_heads)
        if h < 1 or v % h:
            raise ValueError(f"BasisAttention: {h} heads do not divide the value size {v}")
        if not 1 <= k <= _lib.BASIS_ATT_MAX_BASIS:
            raise ValueError(f"BasisAttention: {k} basis functions, expected 1 .. {_lib.BASIS_ATT_MAX_BASIS}")
        if tuple(key.shape) != (n, v):
            raise ValueError(f"BasisAttention: key of shape {tuple(key.shape)}, expected {(n, v)}")
        if tuple(pe.shape) not in ((k, v), (1, k, v)):
            raise ValueError(f"BasisAttention: pe of shape {tuple(pe.shape)}, expected {(k, v)} or {(1, k, v)}")
        kr, stride = _key_rows(key, v)
        p = _as(pe, f32).reshape(k, v)
        dev = t.device
        att = _empty((n, k, h), dtype=f32, device=dev)
        out = _empty((n, v), dtype=f32, device=dev)
        _lib.check(lib.se3_basis_att_fwd(_ptr(t, f32, "T"), C.c_void_p(kr.data_ptr()), stride, _ptr(p, f32, "pe", dev), n, v, h, k,
                                         _ptr(att, f32, "att"), _ptr(out, f32, "out"), _stream(dev)), "se3_basis_att_fwd")
        ctx.save_for_backward(t, kr, p, att)
        ctx.call = (h, stride, T.dtype, key.dtype, pe.dtype, tuple(pe.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f32 = torch.float32
        t, kr, p, att = ctx.saved_tensors
        h, stride, dt_t, dt_key, dt_pe, shape_pe = ctx.call
        n, v, k = t.shape[0], t.shape[1] // 2, t.shape[2]
        g = _as(g, f32)
        dev = t.device
        d_t, d_key, d_pe = _empty_like(t), _empty((n, v), dtype=f32, device=dev), _empty_like(p)
        ws = _workspace(lib.se3_basis_att_workspace_bytes(n, v, h, k), dev)
        _lib.check(lib.se3_basis_att_bwd(_ptr(g, f32, "grad_out", dev), _ptr(t, f32, "T"), C.c_void_p(kr.data_ptr()), stride,
                                         _ptr(p, f32, "pe"), _ptr(att, f32, "att"), n, v, h, k, _ptr(d_t, f32, "dT"),
                                         _ptr(d_key, f32, "dkey"), _ptr(d_pe, f32, "dpe"), C.c_void_p(ws.data_ptr()), ws.numel(),
                                         _stream(dev)), "se3_basis_att_bwd")
        return d_t.to(dt_t), d_key.to(dt_key), d_pe.reshape(shape_pe).to(dt_pe), None


class FusedBasisAttention(torch.autograd.Function):
    """``FeatBasisProj -> BasisAttention`` as one edge-wise operator (``se3_att_fused_fwd`` / ``_bwd``, include/se3conv_att_fused.h):
    with ``phi [E,K]``, ``x = linear_kqv_(f) [N,3V]`` (value | query | key), ``pe [K,V]`` or ``[1,K,V]`` and the edges (sample, source)
    of one cloud grouped by sample,

        c[e,h] = sum_{i in h} xq[p_e,i] key[s,i]      att[s,:,h] = softmax_k(sum_{e in s} phi[e,k] c[e,h] + sum_{i in h} pe[k,i] key[s,i])
        a[e,h] = sum_k phi[e,k] att[s,k,h]            out[s,i] = sum_{e in s} a[e,h(i)] xv[p_e,i]

    which is what the two operators compute through ``T [N,2V,K]`` -- ``T`` is linear in ``phi``, so it never exists.  Returns
    ``out [N,V]``; gradients go to ``phi``, ``x`` and ``pe``.  ``cache``: an object (the neighbourhood) that keeps the source-major
    transposition the backward needs (``neigh_transposition``)."""

    @staticmethod
    def forward(ctx, phi, x, pe, neighbors, ends, num_heads, cache=None):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        for name, t in (("phi", phi), ("x", x), ("pe", pe), ("neighbors", neighbors), ("ends", ends)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"FusedBasisAttention: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
        ph, xr = _as(phi, f32), _as(x, f32)
        nb, en = _as(neighbors, i32), _as(ends, i32)
        if ph.dim() != 2 or xr.dim() != 2 or xr.shape[1] % 3:
            raise ValueError(f"FusedBasisAttention: phi of shape {tuple(phi.shape)} and x of shape {tuple(x.shape)}, expected [E, K] and [N, 3V]")
        (e, k), n, v = ph.shape, xr.shape[0], xr.shape[1] // 3
        h = int(num_heads)
        if h < 1 or v < 1 or v % h:
            raise ValueError(f"FusedBasisAttention: {h} heads do not divide the value size {v}")
        if not 1 <= k <= _lib.BASIS_ATT_MAX_BASIS:
            raise ValueError(f"FusedBasisAttention: {k} basis functions, expected 1 .. {_lib.BASIS_ATT_MAX_BASIS}")
        if tuple(pe.shape) not in ((k, v), (1, k, v)):
            raise ValueError(f"FusedBasisAttention: pe of shape {tuple(pe.shape)}, expected {(k, v)} or {(1, k, v)}")
        if nb.dim() != 2 or nb.shape[1] != 2 or nb.shape[0] != e:
            raise ValueError("FusedBasisAttention: neighbors must be [E,2], one row per row of phi")
        if tuple(en.shape) != (n,):
            raise ValueError(f"FusedBasisAttention: ends of shape {tuple(ends.shape)} for {n} rows of x (samples and sources are one cloud)")
        p = _as(pe, f32).reshape(k, v)
        dev = xr.device
        att = _empty((n, k, h), dtype=f32, device=dev)
        out = _empty((n, v), dtype=f32, device=dev)
        _lib.check(lib.se3_att_fused_fwd(_ptr(ph, f32, "phi", dev), _ptr(xr, f32, "x"), _ptr(p, f32, "pe", dev),
                                         _ptr(nb, i32, "neighbors", dev), _ptr(en, i32, "ends", dev), n, e, v, h, k,
                                         _ptr(att, f32, "att"), _ptr(out, f32, "out"), _stream(dev)), "se3_att_fused_fwd")
        ctx.save_for_backward(ph, xr, p, nb, en, att)
        ctx.cache = cache
        ctx.call = (h, phi.dtype, x.dtype, pe.dtype, tuple(pe.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f32, i32 = torch.float32, torch.int32
        ph, xr, p, nb, en, att = ctx.saved_tensors
        h, dt_phi, dt_x, dt_pe, shape_pe = ctx.call
        (e, k), n, v = ph.shape, xr.shape[0], xr.shape[1] // 3
        g = _as(g, f32)
        dev = xr.device
        if e:
            ts, te, tid = neigh_transposition(nb, n, ctx.cache)
        else:  # nothing to transpose: no source has an incoming edge
            ts, te, tid = None, torch.zeros(n, dtype=i32, device=dev), None
        d_phi, d_x, d_pe = _empty_like(ph), _empty_like(xr), _empty_like(p)
        ws = _workspace(lib.se3_att_fused_workspace_bytes(n, e, v, h, k), dev)
        _lib.check(lib.se3_att_fused_bwd(_ptr(g, f32, "grad_out", dev), _ptr(ph, f32, "phi"), _ptr(xr, f32, "x"), _ptr(p, f32, "pe"),
                                         _ptr(att, f32, "att"), _ptr(nb, i32, "neighbors"), _ptr(en, i32, "ends"),
                                         _ptr(ts, i32, "t_samples"), _ptr(te, i32, "t_ends"), _ptr(tid, i32, "t_edge_ids"), n, e, v, h, k,
                                         _ptr(d_phi, f32, "dphi"), _ptr(d_x, f32, "dx"), _ptr(d_pe, f32, "dpe"),
                                         C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)), "se3_att_fused_bwd")
        return d_phi.to(dt_phi), d_x.to(dt_x), d_pe.reshape(shape_pe).to(dt_pe), None, None, None, None


# ------------------------------------------------------------------ row-wise glue of a block (row f-3)
def _glue_ws(c: int, dev) -> torch.Tensor:
    return _workspace(_lib.load().se3_glue_workspace_bytes(int(c)), dev)


class BatchNormTrain(torch.autograd.Function):
    """Training-mode ``torch.nn.BatchNorm1d`` on ``[rows, C]`` (layers/BatchNormPC.py:22-32): channel sums in fp64 and
    a fixed order, running statistics updated in place, 3 launches forward and 3 backward.  ``n_valid``, ``n_frames``: the
    feature rows of a padded cloud ([n_rows * n_frames, C], taken as they are) -- statistics and gradient over the present
    rows alone, bit for bit those of the call on the trimmed tensor, zeros at the absent rows."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, num_batches_tracked=None, n_valid=None,
                n_frames=1):
        f32 = torch.float32
        x2 = _feature_rows(x, n_valid, n_frames, "BatchNormTrain")
        c, dev = x2.shape[1], x2.device
        y = _empty_like(x2)
        mean = _empty(c, dtype=f32, device=dev)
        invstd = _empty(c, dtype=f32, device=dev)
        w = _as(weight, f32) if weight is not None else None
        b = _as(bias, f32) if bias is not None else None
        ws = _glue_ws(c, dev)
        fn, name = _row_pass("se3_bn_fwd", n_valid)
        _lib.check(fn(_ptr(x2, f32, "x"), _ptr(w, f32, "weight", dev), _ptr(b, f32, "bias", dev),
                      *_glue_rows(x2, n_valid, int(n_frames), "BatchNormTrain"), c, float(eps), float(momentum),
                      _ptr(running_mean, f32, "running_mean", dev), _ptr(running_var, f32, "running_var", dev),
                      _ptr(num_batches_tracked, torch.int64, "num_batches_tracked", dev), _ptr(y, f32, "y"),
                      _ptr(mean, f32, "mean"), _ptr(invstd, f32, "invstd"), C.c_void_p(ws.data_ptr()), ws.numel(),
                      _stream(dev)), name)
        ctx.save_for_backward(x2, w if w is not None else torch.empty(0, device=dev), mean, invstd)
        ctx.has_w, ctx.n_valid, ctx.frames = w is not None, n_valid, int(n_frames)
        ctx.mark_non_differentiable(*[t for t in (running_mean, running_var, num_batches_tracked) if t is not None])
        return y

    @staticmethod
    def backward(ctx, g):
        f32 = torch.float32
        x2, w, mean, invstd = ctx.saved_tensors
        g2 = _as(g, f32)
        c, dev = x2.shape[1], x2.device
        dx = _empty_like(x2)
        dgamma = _empty(c, dtype=f32, device=dev)
        dbeta = _empty(c, dtype=f32, device=dev)
        ws = _glue_ws(c, dev)
        fn, name = _row_pass("se3_bn_bwd", ctx.n_valid)
        _lib.check(fn(_ptr(g2, f32, "dy", dev), _ptr(x2, f32, "x"), _ptr(mean, f32, "mean"), _ptr(invstd, f32, "invstd"),
                      _ptr(w if ctx.has_w else None, f32, "weight"), *_glue_rows(x2, ctx.n_valid, ctx.frames, "BatchNormTrain"),
                      c, _ptr(dx, f32, "dx"), _ptr(dgamma, f32, "dgamma"), _ptr(dbeta, f32, "dbeta"),
                      C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)), name)
        ng = ctx.needs_input_grad
        return (dx if ng[0] else None, dgamma if ng[1] else None, dbeta if ng[2] else None) + (None,) * 7


class SkipDropPath(torch.autograd.Function):
    """``drop_path(x * gamma_) + y`` of layers/SkipConnection.py with the per-batch gate of layers/DropPathPC.py:30-46
    (``gate [B]`` holds keep-mask / keep_prob -- or, with ``gate_keep = keep_prob > 0``, the uniform draws themselves, the
    kernel then evaluates floor(keep + u) / keep; ``row_batch [rows]`` int32 maps rows to batch elements; both None: no drop
    path) -- one launch forward, two backward.  ``n_valid``, ``n_frames``: the feature rows of a padded cloud
    ([n_rows * n_frames, C], taken as they are, ``row_batch`` too) -- the batch id of an absent row is never used to index
    the gate, and the absent rows get zeros."""

    @staticmethod
    def forward(ctx, x, y, gamma, gate, row_batch, gate_keep=0.0, n_valid=None, n_frames=1):
        f32, i32 = torch.float32, torch.int32
        x2, y2 = _feature_rows(x, n_valid, n_frames, "SkipDropPath"), _as(y, f32)
        if x2.shape != y2.shape:
            raise ValueError("SkipDropPath: x and y must be [rows, C] of the same shape")
        c, dev = x2.shape[1], x2.device
        ga = _as(gamma, f32).reshape(-1)
        gt = _as(gate, f32) if gate is not None else None
        rb = None
        if gate is not None:
            rb = row_batch if n_valid is not None else _as(row_batch, i32)
        if gt is not None and (rb is None or rb.shape[0] != x2.shape[0]):
            raise ValueError("SkipDropPath: one batch id per row expected")
        out = _empty_like(x2)
        fn, name = _row_pass("se3_skip_fwd", n_valid)
        _lib.check(fn(_ptr(x2, f32, "x"), _ptr(y2, f32, "y", dev), _ptr(ga, f32, "gamma", dev), _ptr(gt, f32, "gate", dev),
                      float(gate_keep), _ptr(rb, i32, "row_batch", dev), *_glue_rows(x2, n_valid, int(n_frames), "SkipDropPath"),
                      c, _ptr(out, f32, "out"), _stream(dev)), name)
        ctx.save_for_backward(x2, ga, gt if gt is not None else torch.empty(0, device=dev),
                              rb if rb is not None else torch.empty(0, dtype=i32, device=dev))
        ctx.gated, ctx.gamma_shape, ctx.gate_keep = gt is not None, gamma.shape, float(gate_keep)
        ctx.n_valid, ctx.frames = n_valid, int(n_frames)
        return out

    @staticmethod
    def backward(ctx, g):
        f32, i32 = torch.float32, torch.int32
        x2, ga, gt, rb = ctx.saved_tensors
        g2 = _as(g, f32)
        c, dev = x2.shape[1], x2.device
        ng = ctx.needs_input_grad
        dx = _empty_like(x2) if ng[0] else None
        dgamma = _empty(c, dtype=f32, device=dev)
        ws = _glue_ws(c, dev)
        fn, name = _row_pass("se3_skip_bwd", ctx.n_valid)
        _lib.check(fn(_ptr(g2, f32, "g", dev), _ptr(x2, f32, "x"), _ptr(ga, f32, "gamma"),
                      _ptr(gt if ctx.gated else None, f32, "gate"), ctx.gate_keep,
                      _ptr(rb if ctx.gated else None, i32, "row_batch"), *_glue_rows(x2, ctx.n_valid, ctx.frames, "SkipDropPath"),
                      c, _ptr(dx, f32, "dx"), _ptr(dgamma, f32, "dgamma"), C.c_void_p(ws.data_ptr()), ws.numel(),
                      _stream(dev)), name)
        return (dx, (g2 if ng[1] else None), (dgamma.reshape(ctx.gamma_shape) if ng[2] else None)) + (None,) * 5


class BiasGelu(torch.autograd.Function):
    """``GELU(z + bias)`` (exact erf, torch.nn.GELU default) behind a bias-free GEMM: the bias add, the activation and
    the bias gradient's channel sum in one pass each way (layers/ResNetFormer.py:79-81)."""

    @staticmethod
    def forward(ctx, z, bias):
        lib = _lib.load()
        f32 = torch.float32
        z2 = _as(z, f32)
        rows, c = z2.shape
        dev = z2.device
        b = _as(bias, f32) if bias is not None else None
        out = _empty_like(z2)
        _lib.check(lib.se3_affine_act(_ptr(z2, f32, "z"), C.c_void_p(0), C.c_void_p(0), _ptr(b, f32, "bias", dev), rows, c, 1,
                                      _ptr(out, f32, "out"), _stream(dev)), "se3_affine_act")
        ctx.save_for_backward(z2, b if b is not None else torch.empty(0, device=dev))
        ctx.has_b = b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        f32 = torch.float32
        z2, b = ctx.saved_tensors
        g2 = _as(g, f32)
        rows, c = z2.shape
        dev = z2.device
        dz = _empty_like(z2)
        db = _empty(c, dtype=f32, device=dev)
        ws = _glue_ws(c, dev)
        _lib.check(lib.se3_bias_gelu_bwd(_ptr(g2, f32, "g", dev), _ptr(z2, f32, "z"), _ptr(b if ctx.has_b else None, f32, "bias"),
                                         rows, c, _ptr(dz, f32, "dz"), _ptr(db, f32, "dbias"), C.c_void_p(ws.data_ptr()),
                                         ws.numel(), _stream(dev)), "se3_bias_gelu_bwd")
        return dz, (db if (ctx.has_b and ctx.needs_input_grad[1]) else None)


class Linear(torch.autograd.Function):
    """``x @ weight.T (+ bias)`` with the weight gradient on the library's row-split TN GEMM (``se3_linear_wgrad``): the
    forward and the input gradient are plain BLAS GEMMs (fine as they are, 20-35 us at 131 k rows), the weight gradient --
    a reduction over every row of the cloud into a ``[n_out, n_in]`` matrix -- is what the generic heuristics run on a
    handful of workgroups (0.28-0.36 ms at 131 k rows against ~0.03 here).  The block's ``torch.nn.Linear`` layers
    (layers/ResNetFormer.py:42-49, 80-86).

    ``n_frames`` (an integer): the bias gradient is ``channel_sums`` over the present rows (``n_valid``; None: every row)
    instead of ``g.sum(0)`` -- on the feature rows of a padded cloud, and wherever a captured step shall hold no memset node.
    The rest is the same there: the GEMMs are row-wise (absent rows stay finite: they hold the bias), and the weight
    gradient runs over all rows, the gradient rows of absent points being zero (pc.py: the invariant)."""

    @staticmethod
    def forward(ctx, x, weight, bias, n_valid=None, n_frames=None):
        if n_valid is not None and n_frames is None:
            raise ValueError("Linear: a row-count word needs the frame count of the rows")
        ctx.save_for_backward(x, weight)
        ctx.has_b, ctx.n_valid, ctx.frames = bias is not None, n_valid, n_frames
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        f32 = torch.float32
        gx = gw = gb = None
        g2 = _as(g, f32)
        if ctx.needs_input_grad[0]:
            gx = g2 @ weight
        if ctx.needs_input_grad[1]:
            lib = _lib.load()
            x2 = _as(x, f32)
            rows, n_in = x2.shape
            n_out = weight.shape[0]
            dev = x2.device
            gw = _empty(n_out, n_in, dtype=f32, device=dev)
            ws = _workspace(lib.se3_linear_wgrad_workspace_bytes(rows, n_out, n_in), dev)
            _lib.check(lib.se3_linear_wgrad(_ptr(g2, f32, "grad_y", dev), _ptr(x2, f32, "x"), rows, n_out, n_in,
                                            _ptr(gw, f32, "grad_w"), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)),
                       "se3_linear_wgrad")
        if ctx.has_b and ctx.needs_input_grad[2]:
            gb = g2.sum(0) if ctx.frames is None else channel_sums(g2, ctx.n_valid, ctx.frames)
        return gx, gw, gb, None, None


# ------------------------------ random levels and channel sums on padded clouds (include/se3conv_padded_rows.h)
def rows_gather_padded(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``src[idx]`` along dim 0 with a zero row where ``idx < 0`` (``se3_rows_gather_padded``)."""
    if not src.is_cuda:
        raise ValueError("rows_gather_padded: expected a GPU tensor (the HIP path has no CPU fallback)")
    src = src.detach().contiguous()
    out = _empty((idx.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if idx.shape[0] and out.numel():
        _lib.check(_lib.load().se3_rows_gather_padded(
            C.c_void_p(src.data_ptr()), _ptr(idx, torch.int32, "idx", src.device), idx.shape[0],
            out[0].numel() * out.element_size(), C.c_void_p(out.data_ptr()), _stream(src.device)), "se3_rows_gather_padded")
    return out


def rows_unpick_padded(src: torch.Tensor, cell_ids: torch.Tensor, picked: torch.Tensor) -> torch.Tensor:
    """``out[r] = src[cell_ids[r]]`` where row ``r`` is the one its cell picked (``picked[cell_ids[r]] == r``), zero rows
    elsewhere (``se3_rows_unpick_padded``): the scatter of ``rows_scatter`` written as a gather."""
    if not src.is_cuda:
        raise ValueError("rows_unpick_padded: expected a GPU tensor (the HIP path has no CPU fallback)")
    src = src.detach().contiguous()
    if src.shape[0] != picked.shape[0]:
        raise ValueError(f"rows_unpick_padded: {src.shape[0]} rows for {picked.shape[0]} cells")
    out = _empty((cell_ids.shape[0],) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if cell_ids.shape[0] and out.numel():
        _lib.check(_lib.load().se3_rows_unpick_padded(
            C.c_void_p(src.data_ptr()), _ptr(cell_ids, torch.int32, "cell_ids", src.device),
            _ptr(picked, torch.int32, "picked", src.device), cell_ids.shape[0], out[0].numel() * out.element_size(),
            C.c_void_p(out.data_ptr()), _stream(src.device)), "se3_rows_unpick_padded")
    return out


class RowsGatherPadded(torch.autograd.Function):
    """Pooling through a padded random level: ``x[picked]``, zero rows behind the kept cells; the gradient is
    ``rows_unpick_padded``."""

    @staticmethod
    def forward(ctx, x, cell_ids, picked):
        ctx.cell_ids, ctx.picked = cell_ids, picked
        return rows_gather_padded(x, picked)

    @staticmethod
    def backward(ctx, g):
        return rows_unpick_padded(g, ctx.cell_ids, ctx.picked), None, None


class RowsUnpickPadded(torch.autograd.Function):
    """Up-sampling through a padded random level (``rows_unpick_padded``); the gradient is ``rows_gather_padded``."""

    @staticmethod
    def forward(ctx, x, cell_ids, picked):
        ctx.picked = picked
        return rows_unpick_padded(x, cell_ids, picked)

    @staticmethod
    def backward(ctx, g):
        return rows_gather_padded(g, ctx.picked), None, None


def channel_sums(x2: torch.Tensor, n_valid: Optional[torch.Tensor] = None, n_frames: int = 1) -> torch.Tensor:
    """``x2[:present].sum(0)`` of a [n_rows * frames, C] float32 matrix (``se3_channel_sums_padded``): fp64 partial sums in a
    fixed order, and -- unlike torch's multi-block column sum, which zeroes its semaphores -- no memset node in a captured
    graph."""
    lib = _lib.load()
    f32 = torch.float32
    x2, n_rows = _padded_rows(x2, n_frames, "channel_sums")
    c, dev = x2.shape[1], x2.device
    out = _empty(c, dtype=f32, device=dev)
    ws = _glue_ws(c, dev)
    _lib.check(lib.se3_channel_sums_padded(_ptr(x2, f32, "x"), n_rows, int(n_frames), _valid_word(n_valid, dev, "channel_sums"), c,
                                           _ptr(out, f32, "sums"), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev)),
               "se3_channel_sums_padded")
    return out
