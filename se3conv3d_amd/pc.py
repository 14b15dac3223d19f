"""Geometry containers the accelerated path reads (mirror of point_cloud_lib/pc).

Only what the convolution and the benchmark stack need:

  * ``Pointcloud`` / ``PointcloudRotEquiv``  (pc/Pointcloud.py:5-48, pc/PointcloudRotEquiv.py:13-52):
    ``pts_``, ``batch_ids_``, ``local_frames_ [N,F,9]``, ``n_frames_``,
    ``batch_ids_considering_frames_``; frames sampled in the constructor -- random rotations, rotations
    about a fixed axis (pc/RotationFunctions.py:428-508) or PCA frames from a self-kNN neighbourhood
    (``KnnNeighborhood`` + ``sample_reference_frames_pca``, scope row f-1, HIP kernels in csrc/frames.hip).
  * ``Neighborhood`` / ``BQNeighborhood``    (pc/Neighborhood.py, pc/BQNeighborhood.py:13-64) on the HIP ball query.
  * ``GridSubSample`` / ``PointHierarchy`` / ``PointHierarchyRotEquiv`` (pc/GridSubSample.py:40-93,
    pc/Grid.py:37-57, pc/PointHierarchy.py:10-93, pc/PointHierarchyRotEquiv.py:7-44): grid-average and
    random one-point-per-cell sub-sampling (``se3_grid_subsample`` / ``se3_grid_pick``), neighbourhood memo
    (ball query and k-NN).

Padded feature rows (``p_padded_rows=True`` on a padded cloud or hierarchy, include/se3conv_padded_rows.h).  The feature
tensors of such a cloud are padded like its points: ``[n_rows * F, C]`` of which the first ``n_valid_ * F`` rows exist.  What
a network gets:

  * Every library pass on a flagged cloud -- batch norm, skip connection, drop path, frame pooling, ``pool_tensor`` /
    ``upsample_tensor`` -- reads no absent row and leaves ZEROS at the absent rows of what it returns, so the convolution's
    "absent feature rows are finite" obligation holds by construction.
  * Stock torch ops between the library passes (Linear, GELU) are row-wise: they keep absent rows finite.
  * The caller's obligations: the level-0 input features are finite in every row of the buffer, and the loss ignores the
    absent rows (``present_mask``), so that the gradient arriving there is zero.
"""
from __future__ import annotations

import math
import os
from abc import ABC, abstractmethod

import torch

from . import ops

_FRAME_POOL_TORCH = os.environ.get("SE3_FRAME_POOL", "torch") != "lib"


# ------------------------------------------------------------------------------------------ frames
def quaternion_to_matrix(q: torch.Tensor) -> torch.Tensor:
    """Real-part-first quaternions -> rotation matrices (pc/RotationFunctions.py:57-88)."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    m = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def sample_reference_frames(n_origins: int, n_frames: int, axis_fixed=None, dtype=None, device=None) -> torch.Tensor:
    """Random frames ``[n_origins, n_frames, 9]`` (pc/RotationFunctions.py:428-508).  Note the
    reference treats ``axis_fixed = 0`` as "not fixed" (``not axis_fixed``); kept."""
    n = n_origins * n_frames
    if axis_fixed is None or not axis_fixed:
        o = torch.randn((n, 4), dtype=dtype, device=device)
        s = (o * o).sum(1)
        sign = torch.where(o[:, 0] < 0, -torch.ones_like(s), torch.ones_like(s))
        o = o / (torch.sqrt(s) * sign)[:, None]
        return quaternion_to_matrix(o).reshape(n_origins, n_frames, 9)
    ang = torch.rand(n, device=device) * 2 * math.pi
    c, s, z, o = torch.cos(ang), torch.sin(ang), torch.zeros_like(ang), torch.ones_like(ang)
    if axis_fixed == 1:
        rows = (c, z, s, z, o, z, -s, z, c)
    elif axis_fixed == 2:
        rows = (c, -s, z, s, c, z, z, z, o)
    else:
        raise ValueError(f"axis_fixed = {axis_fixed}")
    return torch.stack(rows, -1).reshape(n_origins, n_frames, 9)


# ------------------------------------------------------------------------------------------ clouds
def _repeat_rows(t, times):
    """``t.repeat_interleave(times)`` for a 1-D tensor as one copy kernel (repeat_interleave is four launches and, without
    an output size, a read-back)."""
    return t[:, None].expand(-1, int(times)).reshape(-1)


def is_padded(cloud) -> bool:
    """Whether ``cloud`` is a padded cloud: buffers of which only the first ``n_valid_`` rows (a device word) exist."""
    return getattr(cloud, "n_valid_", None) is not None


def refuse_padded(cloud, what: str) -> None:
    """The loud end of what padded clouds do not support yet (limits table)."""
    if is_padded(cloud):
        hint = " (or pass p_native=True on a cloud built with p_padded_rows=True)" if what.startswith("global_") else ""
        raise NotImplementedError(f"{what} on a padded cloud (p_n_valid) is not implemented: it reads every row of the "
                                  "buffers, and the present-row count is a device word -- build the hierarchy with "
                                  f"p_padded=False for it{hint}")


def padded_rows(cloud) -> bool:
    """Whether the feature tensors of ``cloud`` are padded like its points (``p_padded_rows=True``): the row-wise passes then
    skip the absent rows and write zeros there instead of refusing."""
    return bool(getattr(cloud, "padded_rows_", False))


def refuse_unflagged(cloud, what: str) -> None:
    """``refuse_padded`` unless the cloud was built with ``p_padded_rows=True``."""
    if not padded_rows(cloud):
        refuse_padded(cloud, what)


def present_mask(cloud, per_frame: bool = False) -> torch.Tensor:
    """Bool ``[n_rows]`` (``per_frame``: ``[n_rows * F]``, one entry per feature row) that is True at the present rows of
    ``cloud``: ``arange < word`` built with torch ops, no read-back -- what a loss uses to ignore the absent rows.  All True
    for an ordinary cloud."""
    n = int(cloud.pts_.shape[0])
    f = int(getattr(cloud, "n_frames_", 1)) if per_frame else 1
    idx = torch.arange(n * f, device=cloud.pts_.device)
    if not is_padded(cloud):
        return idx >= 0
    return idx < torch.clamp(cloud.n_valid_, 0, n) * f


def _batches_of(cloud):
    """The batch count a grid sub-sample of ``cloud`` has: its own (every batch element that holds a point keeps a cell, so
    the largest id survives); None for foreign cloud objects."""
    return cloud.num_batches() if hasattr(cloud, "num_batches") else None


class Pointcloud(object):
    """``p_n_valid`` (extension, keyword): a PADDED cloud -- ``p_pts`` / ``p_batch_ids`` are buffers of which only the rows
    ``[0, p_n_valid)`` exist, ``p_n_valid`` being a 1-element int32 device tensor (``n_valid_``; None for an ordinary
    cloud).  Boxes, self-k-NN, PCA frames and ball-query neighbourhoods of such a cloud never read the other rows and never
    read the count back (include/se3conv_padded.h), so they capture into a HIP graph that follows the word.  The buffers
    are taken as they are (float32 / int32, contiguous) and ``num_batches`` is required.

    What the cloud caches -- boxes, the k-NN table, shared source grids -- is keyed on the word's storage and version counter.
    A graph replay rewrites the words, points and batch ids of the clouds a captured build made without moving a version:
    such held clouds are for reading (``pts_``, ``n_valid_``, ``local_frames_``, the neighbourhoods built in the capture), not
    for further eager queries, which could meet a box, table or grid of the replay before.  Query a fresh ``Pointcloud`` over
    the same buffers instead (or call ``ops.forget_source_grids(cloud)`` and drop ``_se3_aabb`` / ``_se3_knn_ids``).

    ``p_padded_rows=True`` (extension, keyword, needs ``p_n_valid``; attribute ``padded_rows_``): the feature tensors of this
    cloud are padded like its points.  The row-wise glue (blocks.py, ``feature_pooling``) then skips the absent rows and
    writes zeros there (include/se3conv_padded_rows.h; the invariant a network gets: module docstring).  Without it that
    glue refuses a padded cloud."""

    def __init__(self, p_pts, p_batch_ids, **kwargs):
        self.pts_with_grads_ = bool(kwargs.pop("requires_grad", False))
        self.n_valid_ = kwargs.pop("p_n_valid", None)
        self.padded_rows_ = bool(kwargs.pop("p_padded_rows", False))
        if self.padded_rows_ and self.n_valid_ is None:
            raise ValueError("p_padded_rows=True needs p_n_valid: only a padded cloud has padded feature rows")
        # num_batches (extension): the batch count when the caller knows it (a hierarchy level has its parent's) -- spares
        # the read-back of batch_size_ the native calls' table sizes would otherwise cost once per cloud
        known_batches = kwargs.pop("num_batches", None)
        self.pts_ = torch.as_tensor(p_pts, **kwargs)
        self.batch_ids_ = torch.as_tensor(p_batch_ids, **kwargs)
        if self.n_valid_ is not None:
            if known_batches is None:
                raise ValueError("a padded cloud (p_n_valid) needs num_batches: the batch ids of absent rows say nothing, and "
                                 "reading the largest present one would be a read-back")
            w = self.n_valid_
            if not isinstance(w, torch.Tensor) or w.dtype != torch.int32 or w.numel() != 1 or w.device != self.pts_.device:
                raise ValueError("p_n_valid is a 1-element int32 tensor on the device of the points")
            ops._padded_cloud(self.pts_, self.batch_ids_, "Pointcloud")
            self.batch_size_ = torch.tensor(int(known_batches))  # (on the host: absent rows' ids are not looked at)
        else:
            self.batch_size_ = torch.max(self.batch_ids_) + 1
        if known_batches is not None:
            self._num_batches = int(known_batches)
        if self.pts_with_grads_:
            self.pts_.requires_grad = True

    def to_device(self, p_device):
        self.pts_ = self.pts_.to(p_device)
        self.batch_ids_ = self.batch_ids_.to(p_device)
        self.batch_size_ = self.batch_size_.to(p_device)
        if self.n_valid_ is not None:
            self.n_valid_ = self.n_valid_.to(p_device)

    @staticmethod
    def _pool_rows_by(ids, p_in_tensor, p_pooling_method, n_out):
        how = {"avg": "mean", "max": "amax", "min": "amin", "sum": "sum"}[p_pooling_method]
        idx = ids.to(torch.int64).reshape((-1,) + (1,) * (p_in_tensor.dim() - 1)).expand_as(p_in_tensor)
        out = torch.zeros((n_out,) + tuple(p_in_tensor.shape[1:]), dtype=p_in_tensor.dtype, device=p_in_tensor.device)
        return out.scatter_reduce(0, idx, p_in_tensor, how, include_self=False)

    def global_pooling(self, p_in_tensor, p_pooling_method="avg", p_native=False):
        """One row per batch element (pc/Pointcloud.py:58-76; classification heads -- [B, C] outputs, plain torch).
        ``p_native=True`` (extension, keyword): the library's kernels instead (``ops.GlobalPool``,
        include/se3conv_global_pool.h) -- fp64 sums in a fixed order, so two runs give the same bits, and on a cloud built
        with ``p_padded_rows=True`` the pass follows the row-count word and captures into a graph."""
        if p_native:
            return self._global_pool_native(p_in_tensor, p_pooling_method, getattr(self, "n_frames_", 1), "global_pooling")
        refuse_padded(self, "global_pooling")
        return self._pool_rows_by(self.batch_ids_, p_in_tensor, p_pooling_method, self.num_batches())

    def _global_pool_native(self, p_in_tensor, p_pooling_method, n_frames, what):
        if p_pooling_method not in ops.POOL_MODES:
            raise ValueError(p_pooling_method)
        refuse_unflagged(self, what)
        return ops.GlobalPool.apply(p_in_tensor, self.batch_ids_, self.num_batches(), p_pooling_method, n_frames, self.n_valid_)

    def global_upsample(self, p_in_tensor, p_native=False):
        """pc/Pointcloud.py:79-88.  ``p_native=True``: ``ops.GlobalUpsample`` -- zero rows for the absent points of a padded
        cloud, and a gradient that is a sum in fixed order."""
        if p_native:
            refuse_unflagged(self, "global_upsample")
            return ops.GlobalUpsample.apply(p_in_tensor, self.batch_ids_, getattr(self, "n_frames_", 1), self.n_valid_)
        refuse_padded(self, "global_upsample")
        return torch.index_select(p_in_tensor, 0, self.batch_ids_.to(torch.int64))

    def num_batches(self) -> int:
        """``batch_size_`` as a host integer, read back once per cloud (the native calls size their per-batch
        tables with it; the reference re-reads it from the device in every ball query, ball_query.cu:46)."""
        if getattr(self, "_num_batches", None) is None:
            self._num_batches = int(self.batch_size_)
        return self._num_batches

    def aabb(self):
        """Per-batch bounding boxes ``(min, max) [B,3]`` of the points, computed once per cloud (the reference recomputes
        them in every ball query, BallQuery.py:35-36; a cloud is the source of three or four queries per step)."""
        box = getattr(self, "_se3_aabb", None)
        # (points or batch ids replaced or changed in place: new boxes)
        key = (self.pts_.data_ptr(), ops.version_key(self.pts_), self.batch_ids_.data_ptr(),
               ops.version_key(self.batch_ids_))
        if self.n_valid_ is not None:
            # a padded cloud: the boxes of the present rows -- recomputed when the count word changes, and inside a graph
            # capture once per capture (a replay must follow the word; boxes from an earlier node of the same graph do)
            key += (self.n_valid_.data_ptr(), ops.version_key(self.n_valid_))
            if torch.cuda.is_current_stream_capturing():
                key += (ops._capture_id(self.pts_.device),)
                held = getattr(self, "_se3_aabb_captured", None)
                if held is None or held[2] != key:
                    mn, mx = ops.batch_aabb(self.pts_, self.batch_ids_, self.num_batches(), n_valid=self.n_valid_)
                    held = self._se3_aabb_captured = (mn, mx, key)
                return held[0], held[1]
        if box is None or box[2] != key:
            mn, mx = ops.batch_aabb(self.pts_, self.batch_ids_, self.num_batches(), n_valid=self.n_valid_)
            box = (mn, mx, key)
            self._se3_aabb = box
        return box[0], box[1]


class PointcloudRotEquiv(Pointcloud):
    """Point cloud with ``n_frames`` SO(3) reference frames per point."""

    def __init__(self, p_pts, p_batch_ids, p_ref_frames_config, ref_frames_pts=None, standard_knn=False, **kwargs):
        super().__init__(p_pts, p_batch_ids, **kwargs)
        kwargs.pop("num_batches", None)  # (consumed by Pointcloud.__init__; the rest are torch.as_tensor keywords)
        kwargs.pop("p_n_valid", None)
        kwargs.pop("p_padded_rows", None)
        self.neigh_cache_ = {}
        self.local_frames_pca_cache_ = {}
        self.local_frames_config_ = p_ref_frames_config
        self.standard_knn_ = standard_knn
        self.ref_frames_pts = ref_frames_pts
        frames = self.get_local_ref_frames()
        self.n_frames_ = frames.shape[1]
        self.local_frames_ = torch.as_tensor(frames, **kwargs)
        self.batch_ids_considering_frames_ = _repeat_rows(self.batch_ids_, self.n_frames_)

    def get_ref_frame_neighborhood(self, p_neigh_method, **kwargs):
        """kNN / ball-query neighbourhood used to build PCA frames, memoised (PointcloudRotEquiv.py:54-75)."""
        key = str(p_neigh_method) + str(kwargs.get("neigh_k" if p_neigh_method == "knn" else "bq_radius"))
        if key not in self.neigh_cache_:
            if p_neigh_method == "knn":
                self.neigh_cache_[key] = KnnNeighborhood(self, self, kwargs["neigh_k"], p_keep_empty=True,
                                                         p_standard_knn=getattr(self, "standard_knn_", False))
            elif p_neigh_method == "ball_query":
                self.neigh_cache_[key] = BQNeighborhood(self, self, kwargs["bq_radius"])
            else:
                raise ValueError(p_neigh_method)
        return self.neigh_cache_[key]

    def get_local_ref_frames(self):
        cfg = self.local_frames_config_
        if not hasattr(self, "neigh_cache_"):
            self.neigh_cache_, self.local_frames_pca_cache_ = {}, {}
        if self.ref_frames_pts is not None:
            refuse_padded(self, "frames from ref_frames_pts")
            # PointcloudRotEquiv.py:80-128: a cloud with ONE point per batch element (classification heads) takes its
            # frames from the whole element's points, `ref_frames_pts [(B m), 3]`: the PCA of all m points
            # (sample_global_reference_frames_pca, RotationFunctions.py:265-304) or plain random frames
            n_el = self.pts_.shape[0]
            if cfg.get("pca", False):
                if cfg.get("fixed_axis"):
                    raise NotImplementedError("Sampling global ref frames with fixed axes is not implemented")  # as the reference
                if "se3-all" not in self.local_frames_pca_cache_:
                    ref = torch.as_tensor(self.ref_frames_pts, dtype=torch.float32, device=self.pts_.device).reshape(-1, 3)
                    if n_el == 0 or ref.shape[0] % n_el:
                        raise ValueError("ref_frames_pts must hold the same number of points for every batch element")
                    m = ref.shape[0] // n_el
                    # the covariance of "the k listed points" with every element listing all of its own points
                    ids = torch.arange(n_el * m, dtype=torch.int32, device=ref.device).reshape(n_el, m)
                    self.local_frames_pca_cache_["se3-all"] = ops.pca_frames(ref, ids, None)
                return self._shuffled_pca_frames(cfg["n_frames"])
            return sample_reference_frames(1, cfg["n_frames"], axis_fixed=cfg.get("fixed_axis"), device=self.pts_.device)
        if cfg.get("pca", False):
            # PointcloudRotEquiv.py:131-167: all PCA frames once ("se3-all"), then a random permutation per point
            # (torch.multinomial without replacement) and the first n_frames
            if "se3-all" not in self.local_frames_pca_cache_:
                if cfg["neigh_method"] == "knn" and "neigh_k" in cfg["neigh_kwargs"]:
                    # the [N, k] id table straight into the PCA kernel; the neighbourhood OBJECT (its (sample, source)
                    # list and offsets: seven more launches) is built from the same table when somebody asks for it
                    # (get_ref_frame_neighborhood)
                    ids = self._self_knn_ids(cfg["neigh_kwargs"]["neigh_k"])
                    self.local_frames_pca_cache_["se3-all"] = ops.pca_frames(self.pts_, ids, cfg.get("fixed_axis"),
                                                                             n_valid=self.n_valid_)
                else:
                    refuse_padded(self, "PCA frames from a ball-query neighbourhood")
                    nbh = self.get_ref_frame_neighborhood(cfg["neigh_method"], **cfg["neigh_kwargs"])
                    self.local_frames_pca_cache_["se3-all"] = sample_reference_frames_pca(
                        self.pts_, nbh, axis_fixed=cfg.get("fixed_axis"), device=self.pts_.device)
            return self._shuffled_pca_frames(cfg["n_frames"])
        return sample_reference_frames(self.pts_.shape[0], cfg["n_frames"], axis_fixed=cfg.get("fixed_axis"),
                                       device=self.pts_.device)

    def _shuffled_pca_frames(self, n_frames):
        """A random permutation of the cached PCA frames per point (torch.multinomial without replacement), first
        ``n_frames`` kept (PointcloudRotEquiv.py:100-117, 146-167)."""
        all_frames = self.local_frames_pca_cache_["se3-all"]
        # a uniformly random permutation per point = the order of n_all independent uniform draws (the distribution of
        # multinomial without replacement on equal weights): torch.rand + one launch (se3_shuffle_frames) instead of the
        # ~15 launches of torch.multinomial's top-k path (0.14 ms per cloud of a DFaust step's six,
        # profiles/r06_frames_ctor_kernel_stats.csv) or the sort + gather that first replaced it
        return ops.shuffle_frames(all_frames, n_frames)

    def _self_knn_ids(self, k):
        """``[N, k]`` int32 ids of the cloud's self-k-NN (``ops.knn_query``), memoised per k; what KnnNeighborhood builds
        its lists from.  Not while a HIP graph is being captured: a table cached before would be baked into the graph, one
        cached during the capture holds nothing until the first replay."""
        grid = self.pts_.shape[0] >= ops.KNN_GRID_MIN_POINTS and k <= 32
        query = lambda: ops.knn_query(self.pts_, self.batch_ids_, int(k), self.num_batches(), box=self.aabb() if grid else None,
                                      n_valid=self.n_valid_)
        if self.pts_.is_cuda and torch.cuda.is_current_stream_capturing():
            return query()
        cache = self.__dict__.setdefault("_se3_knn_ids", {})
        key = (int(k), self.pts_.data_ptr(), ops.version_key(self.pts_))
        if self.n_valid_ is not None:
            key += (self.n_valid_.data_ptr(), ops.version_key(self.n_valid_))
        if key not in cache:
            cache.clear()
            cache[key] = query()
        return cache[key]

    @classmethod
    def from_frames(cls, p_pts, p_batch_ids, p_frames, p_ref_frames_config=None, p_n_valid=None, num_batches=None,
                    p_padded_rows=False):
        """Cloud with externally supplied frames ``[N,F,9]`` (e.g. PCA frames computed upstream).  ``p_n_valid``,
        ``num_batches``, ``p_padded_rows``: as in the constructor (a padded cloud; the frames of absent rows are not
        looked at)."""
        self = cls.__new__(cls)
        extra = {}
        if p_n_valid is not None:
            extra["p_n_valid"] = p_n_valid
        if num_batches is not None:
            extra["num_batches"] = num_batches
        if p_padded_rows:
            extra["p_padded_rows"] = True
        Pointcloud.__init__(self, p_pts, p_batch_ids, **extra)
        self.local_frames_ = torch.as_tensor(p_frames).reshape(self.pts_.shape[0], -1, 9)
        self.n_frames_ = self.local_frames_.shape[1]
        self.local_frames_config_ = p_ref_frames_config or {"pca": False, "n_frames": self.n_frames_,
                                                            "fixed_axis": False}
        self.ref_frames_pts = None
        self.batch_ids_considering_frames_ = _repeat_rows(self.batch_ids_, self.n_frames_)
        return self

    def to_device(self, p_device):
        super().to_device(p_device)
        self.local_frames_ = self.local_frames_.to(p_device)
        self.batch_ids_considering_frames_ = self.batch_ids_considering_frames_.to(p_device)

    def global_pooling(self, p_in_tensor, p_pooling_method="avg", p_native=False):
        """Rows are per (point, frame) here (pc/PointcloudRotEquiv.py:252-270).  ``p_native``: as in ``Pointcloud`` -- the
        kernel takes the per-point ids and the frame count, no ``[N * F]`` copy of the ids."""
        if p_native:
            return super().global_pooling(p_in_tensor, p_pooling_method, p_native=True)
        refuse_padded(self, "global_pooling")
        return self._pool_rows_by(self.batch_ids_considering_frames_, p_in_tensor, p_pooling_method, self.num_batches())

    def global_upsample(self, p_in_tensor, p_native=False):
        if p_native:
            return super().global_upsample(p_in_tensor, p_native=True)
        refuse_padded(self, "global_upsample")
        return torch.index_select(p_in_tensor, 0, self.batch_ids_considering_frames_.to(torch.int64))

    def global_pooling_specific_feature_pooling(self, p_in_tensor, p_global_pooling_method="avg",
                                                p_feature_pooling_method="avg", p_native=False):
        """Frames first, then batch elements (pc/PointcloudRotEquiv.py:195-222).  ``p_native=True``: ``ops.FramePool``, then
        ``ops.GlobalPool`` over the per-point rows -- two kernels forward, two backward."""
        if p_native:
            if p_feature_pooling_method not in ops.POOL_MODES:
                raise ValueError(p_feature_pooling_method)
            refuse_unflagged(self, "global_pooling_specific_feature_pooling")
            pooled = ops.FramePool.apply(p_in_tensor, self.n_frames_, p_feature_pooling_method, self.n_valid_)
            return self._global_pool_native(pooled, p_global_pooling_method, 1, "global_pooling_specific_feature_pooling")
        refuse_padded(self, "global_pooling_specific_feature_pooling")
        pooled = self.feature_pooling(p_in_tensor, p_pooling_method=p_feature_pooling_method)
        return self._pool_rows_by(self.batch_ids_, pooled, p_global_pooling_method, self.num_batches())

    def feature_pooling(self, p_in_tensor, p_pooling_method="avg"):
        """Pool the F per-frame feature rows of every point (pc/PointcloudRotEquiv.py:224-251), one HIP kernel
        forward and one backward."""
        if p_pooling_method not in ops.POOL_MODES:
            raise ValueError(p_pooling_method)
        refuse_unflagged(self, "feature_pooling")
        # Launched eagerly, a custom autograd.Function costs more in Python than this pass costs on the GPU (fwd + bwd
        # 0.099 ms through the library against 0.057 ms of stock torch ops at 65 k points, profiles/r03_next_rows.txt): outside
        # a graph capture the reduction over the frame axis is torch's own (max / min route their gradient to the winning
        # frame like torch_scatter: torch.max / torch.min with indices, not amax); inside a capture -- where the launch
        # count is what matters -- it is the library's one-kernel form.  SE3_FRAME_POOL=lib forces the library everywhere.
        # A padded cloud always takes the library's kernel: torch's reduction would read the absent rows.
        x = p_in_tensor
        if (not padded_rows(self) and _FRAME_POOL_TORCH and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and
                x.shape[0] % self.n_frames_ == 0 and not torch.cuda.is_current_stream_capturing()):
            v = x.reshape(x.shape[0] // self.n_frames_, self.n_frames_, x.shape[1])
            if p_pooling_method == "avg":
                return v.sum(1) / float(self.n_frames_)
            if p_pooling_method == "sum":
                return v.sum(1)
            return (v.max(1) if p_pooling_method == "max" else v.min(1))[0]
        return ops.FramePool.apply(p_in_tensor, self.n_frames_, p_pooling_method, self.n_valid_)


# ----------------------------------------------------------------------------------- neighbourhoods
class Neighborhood(ABC):
    def __init__(self, p_pc_src, p_samples):
        self.pc_src_ = p_pc_src
        self.samples_ = p_samples
        self.neighbors_ = None
        self.start_ids_ = None
        self.__compute_neighborhood__()

    @abstractmethod
    def __compute_neighborhood__(self):
        pass


class BQNeighborhood(Neighborhood):
    """Ball-query neighbourhood: ``neighbors_ [E,2]`` (col0 sample, col1 source) int64 like the
    reference, ``start_ids_ [M]`` = inclusive end offsets, ``radius_``.

    ``p_capacity`` (extension): build into an edge buffer of that many rows without reading the edge count back to the
    host -- no synchronisation, capturable in a HIP graph.  ``neighbors_`` then has ``p_capacity`` rows of which the
    first ``num_edges()`` are edges (``start_ids_`` never points past them); ``overflowed()`` tells whether the buffer
    was too small (the list is then truncated: rebuild with a larger one).

    ``p_max_neighbors > 0``: every sample keeps at most that many of its neighbours, a seeded uniform subset
    (``ops.ball_query_capped``, at most ``ops.MAX_CAPPED_NEIGHBORS``; zero or less = no limit, as in the reference).
    ``degrees_ [M]`` then holds the uncapped degrees and ``seed_`` the seed (``p_seed``, or one drawn from torch's default CPU
    generator); ``p_seed_tensor`` is a 1-element int32 device tensor added to it on the device (a captured build draws fresh
    subsets when it is updated).  A capped list is not symmetric, also for a cloud against itself, and a second query
    with the roles swapped would draw another subset: ``symmetric_`` is False, ``source_major()`` is None, and backward
    reads the library's transposition of this very list.

    Padded clouds (``Pointcloud(..., p_n_valid=)``, either side): the query is ``ops.ball_query_padded`` -- absent rows are
    never read, absent sources never listed, absent samples have no edges -- and so is ``source_major()``'s second query.
    ``p_capacity`` is then required (``ValueError``), and ``p_max_neighbors > 0`` is not implemented."""

    def __init__(self, p_pc_src, p_samples, p_radius, p_max_neighbors=0, p_capacity=None, p_seed=None, p_seed_tensor=None):
        self.radius_ = p_radius
        self.max_neighbors_ = p_max_neighbors
        self.capacity_ = p_capacity
        self.edge_info_ = None
        self.degrees_ = None
        self.seed_ = None
        self.seed_tensor_ = p_seed_tensor
        if p_max_neighbors > 0:
            self.seed_ = ops.draw_seed() if p_seed is None else int(p_seed)
        # a cloud against itself: (s, p) is an edge iff (p, s) is -- the operator's backward then needs no
        # source-major copy of the edge list (ops.ConvGeometry.transpose)
        self.symmetric_ = p_pc_src is p_samples and p_max_neighbors <= 0
        self.padded_ = is_padded(p_pc_src) or is_padded(p_samples)
        if self.padded_ and p_max_neighbors > 0:
            raise NotImplementedError("BQNeighborhood: p_max_neighbors > 0 on padded clouds (p_n_valid) is not implemented: "
                                      "the capped query has no row-count words")
        if self.padded_ and p_capacity is None:
            raise ValueError("BQNeighborhood: padded clouds (p_n_valid) need p_capacity -- the edge count of a padded query "
                             "is never read back to size the list")
        super().__init__(p_pc_src, p_samples)

    def __compute_neighborhood__(self):
        # same call as ops.BallQuery.apply (which stays for code that uses the op directly), without the autograd node --
        # the edge list carries no gradient.  The kernels read the int32 list (``neighbors_i32_``); the int64
        # ``neighbors_`` the reference exposes is materialised on first access only (33 MB at the headline shape).
        self.sources_i32_ = None
        # the source cloud's boxes: computed once per cloud (Pointcloud.aabb), not once per query
        src_box = self.pc_src_.aabb() if hasattr(self.pc_src_, "aabb") and ops.ball_query_needs_grid(self.pc_src_.pts_.shape[0]) else None
        if self.padded_:
            res = ops.ball_query_padded(self.pc_src_.pts_, self.samples_.pts_, self.pc_src_.batch_ids_,
                                        self.samples_.batch_ids_, self.radius_, int(self.capacity_), self.pc_src_.num_batches(),
                                        n_valid_src=getattr(self.pc_src_, "n_valid_", None),
                                        n_valid_dst=getattr(self.samples_, "n_valid_", None), want_sources=self.symmetric_,
                                        src_box=src_box, grids=ops.source_grids(self.pc_src_))
            nb, self.start_ids_, self.edge_info_ = res[:3]
            if self.symmetric_:
                self.sources_i32_ = res[3]
        elif self.max_neighbors_ > 0:
            res = ops.ball_query_capped(self.pc_src_.pts_, self.samples_.pts_, self.pc_src_.batch_ids_,
                                        self.samples_.batch_ids_, self.radius_, int(self.max_neighbors_), self.seed_,
                                        capacity=None if self.capacity_ is None else int(self.capacity_),
                                        n_batches=self.pc_src_.num_batches(), want_degrees=True, src_box=src_box,
                                        grids=ops.source_grids(self.pc_src_), seed_tensor=self.seed_tensor_)
            nb, self.start_ids_ = res[:2]
            if self.capacity_ is not None:
                self.edge_info_ = res[2]
            self.degrees_ = res[-1]
        elif self.capacity_ is not None:
            res = ops.ball_query_bounded(self.pc_src_.pts_, self.samples_.pts_, self.pc_src_.batch_ids_,
                                         self.samples_.batch_ids_, self.radius_, int(self.capacity_),
                                         self.pc_src_.num_batches(), want_sources=self.symmetric_, src_box=src_box,
                                         grids=ops.source_grids(self.pc_src_))
            nb, self.start_ids_, self.edge_info_ = res[:3]
            if self.symmetric_:
                self.sources_i32_ = res[3]
        else:
            nb, self.start_ids_ = ops.ball_query(self.pc_src_.pts_, self.samples_.pts_, self.pc_src_.batch_ids_,
                                                 self.samples_.batch_ids_, self.radius_, self.pc_src_.num_batches(),
                                                 src_box=src_box)
        self.neighbors_i32_ = nb
        self._neighbors64 = None

    @property
    def neighbors_(self):
        if getattr(self, "_neighbors64", None) is None and getattr(self, "neighbors_i32_", None) is not None:
            self._neighbors64 = self.neighbors_i32_.to(torch.int64)
        return self._neighbors64

    @neighbors_.setter
    def neighbors_(self, value):  # the base class initialises it to None; code may also attach its own list
        self._neighbors64 = value
        if value is not None:
            self.neighbors_i32_ = None

    def source_major(self):
        """The source-major copy of the edge list the operator's backward reads -- ``(t_samples [rows], t_ends [N_src])`` -- or
        ``None`` when the library's transposition of the list is the better way to get it.  Long segments (an
        up-convolution: every source has hundreds of edges) are the case se3_csr_transpose is slow for; the list is then a
        SECOND ball query with the clouds' roles swapped: ``||(s - p) / r|| < 1`` is bit for bit the same predicate both
        ways, so it finds exactly the same edges, grouped by source, in an order that depends on the points only
        (deterministic; not ascending in the sample id, which no consumer needs).  Capacity-bounded like the forward list
        (same row count, hence the same overflow flag: both queries find the same E edges), no host synchronisation:
        capturable.  After an overflow the two lists are truncated differently (sample-major / source-major order), i.e.
        backward would differentiate another sub-graph than forward ran on: ``overflowed()`` must be checked and the step
        redone with a larger buffer -- as for any overflowed neighbourhood (include/se3conv.h, se3_csr_transpose_bounded)."""
        if self.symmetric_ or self.max_neighbors_ > 0 or getattr(self, "neighbors_i32_", None) is None:
            return None
        n_src, n_smp = self.pc_src_.pts_.shape[0], self.samples_.pts_.shape[0]
        rows = int(self.neighbors_i32_.shape[0])
        # segments of 16 entries and up (rows of the edge buffer per source: an up-convolution has hundreds, two clouds of
        # one size ~30, a down-convolution ~4): the second query is cheaper than the library's transposition there (0.2
        # against 0.32 ms at 65 k points x 31 edges); shorter segments are the transposition's good case, and the case the
        # edge-major feature gradient wants its edge ids for
        if n_src == 0 or rows < 16 * n_src:
            return None
        cached = getattr(self, "_source_major", None)
        if cached is None:
            box = self.samples_.aabb() if hasattr(self.samples_, "aabb") and ops.ball_query_needs_grid(n_smp) else None
            if getattr(self, "padded_", False):
                _, t_ends, info, t_samples = ops.ball_query_padded(
                    self.samples_.pts_, self.pc_src_.pts_, self.samples_.batch_ids_, self.pc_src_.batch_ids_, self.radius_, rows,
                    self.samples_.num_batches(), n_valid_src=getattr(self.samples_, "n_valid_", None),
                    n_valid_dst=getattr(self.pc_src_, "n_valid_", None), want_sources=True, src_box=box,
                    grids=ops.source_grids(self.samples_))
            else:
                _, t_ends, info, t_samples = ops.ball_query_bounded(
                    self.samples_.pts_, self.pc_src_.pts_, self.samples_.batch_ids_, self.pc_src_.batch_ids_, self.radius_, rows,
                    self.samples_.num_batches(), want_sources=True, src_box=box, grids=ops.source_grids(self.samples_))
            cached = self._source_major = (t_samples, t_ends, info)
        return cached[0], cached[1]

    def num_edges(self) -> int:
        """Number of edges as a host integer (one device read-back for a capacity-bounded build)."""
        info = getattr(self, "edge_info_", None)
        if info is None:
            nb = self.neighbors_i32_ if getattr(self, "neighbors_i32_", None) is not None else self._neighbors64
            return int(nb.shape[0])
        return min(int(info[0]), int(self.capacity_))

    def overflowed(self) -> bool:
        info = getattr(self, "edge_info_", None)
        return info is not None and bool(info[1] != 0)


class KnnNeighborhood(Neighborhood):
    """k-NN neighbourhood (pc/KnnNeighborhood.py:14-135): the k nearest SOURCE points of every sample inside its
    batch element, k <= 64.  A cloud against itself is the reference's own kernel path (:38-75): ``neighbors_ [N*k, 2]``
    int32 (centre, neighbour; the point itself first, -1 where the batch element is too small), ``start_ids_`` =
    ``(arange + 1) * k`` when empty slots are kept.  Two different clouds are the reference's ``torch_cluster.knn``
    path (:77-135): ``neighbors_`` int64 ``(sample, source)`` in ascending distance per sample, without the missing
    entries unless ``p_keep_empty`` (then -1 in column 1, column 0 = the sample).

    ``p_capacity`` (extension): the list without empty slots built on the device into an edge buffer of that many rows
    (``ops.knn_edges_bounded``, include/se3conv_knn_edges.h) -- no boolean-mask index, no read-back of the edge count, so
    the build captures into a HIP graph.  ``neighbors_i32_ [p_capacity, 2]`` then holds ``num_edges()`` edges in front of an
    unset tail, ``start_ids_`` never points past them, ``edge_info_ [2]`` is (true edge count, overflow flag) on the
    device, and ``num_edges()`` / ``overflowed()`` are the only read-backs; ``neighbors_`` is materialised on first access.
    After an overflow the list is truncated (its head is kept): rebuild with a larger buffer.  ``rows of samples * k`` is
    the capacity that can never overflow.  The same edges in the same order as the unbounded build.  Not with
    ``p_keep_empty=True`` (``ValueError``).

    Padded clouds (``Pointcloud(..., p_n_valid=)``, either side, a padded cloud against itself included) need
    ``p_capacity``: the id table then comes from the padded queries (``ops.knn_query(..., n_valid=)``,
    ``ops.knn_query_pair(..., n_valid_src=, n_valid_q=)``) -- absent rows are never read, absent sources never listed,
    absent samples have no edges.  Without ``p_capacity`` they are refused (``NotImplementedError``).

    ``symmetric_`` is False and ``source_major()`` is None: a k-NN list is not symmetric, also for a cloud against itself,
    so the convolution's backward reads the library's transposition of this list (``se3_csr_transpose_bounded`` on
    ``edge_info_`` for a bounded one)."""

    MAX_K = 64  # neighbours a query keeps in registers; the reference's kernel has the same limit (knn_query.cu:167)

    def __init__(self, p_pc_src, p_samples, p_k, p_keep_empty=False, p_standard_knn=False, p_capacity=None):
        # p_standard_knn (the evaluation scripts pass it, test_scannet_rot.py:110): the reference then takes
        # torch_cluster.knn instead of its own sweep kernel -- another EXACT k-NN; the search here is exact already,
        # so the flag only changes which of several equidistant candidates may come first there
        if not 1 <= int(p_k) <= self.MAX_K:
            raise NotImplementedError(f"KnnNeighborhood: k = {p_k}; the HIP k-NN keeps at most {self.MAX_K} neighbours "
                                      "per point (the limit of the reference's own kernel; its torch_cluster fallback "
                                      "for larger k is not implemented)")
        self.padded_ = is_padded(p_pc_src) or is_padded(p_samples)
        if self.padded_ and p_capacity is None:
            raise NotImplementedError("KnnNeighborhood between padded clouds (p_n_valid) is not implemented without "
                                      "p_capacity, a padded cloud against itself included: the list without empty slots "
                                      "would be sized by a read-back -- pass p_capacity (rows of samples * k cannot "
                                      "overflow) for the list built on the device")
        if p_capacity is not None and p_keep_empty:
            raise ValueError("KnnNeighborhood: p_capacity builds the list without empty slots; it does not go with "
                             "p_keep_empty=True")
        if p_capacity is not None and int(p_capacity) < 0:
            raise ValueError("KnnNeighborhood: p_capacity must be non-negative")
        self.k_ = int(p_k)
        self.keep_empty_ = p_keep_empty
        self.standard_knn_ = p_standard_knn
        self.capacity_ = None if p_capacity is None else int(p_capacity)
        self.edge_info_ = None
        self.neighbors_i32_ = None
        # a k-NN list is not symmetric, also for a cloud against itself: backward reads the library's transposition of it
        self.symmetric_ = False
        super().__init__(p_pc_src, p_samples)

    def __compute_neighborhood__(self):
        self_query = self.pc_src_ is self.samples_
        if self_query:
            # the op behind ops.KNNQuery (which stays for code that uses it directly), with what the cloud already knows:
            # its batch count and its boxes (no device read-back, no second pass over the points)
            pc = self.pc_src_
            if hasattr(pc, "_self_knn_ids"):
                ids = pc._self_knn_ids(self.k_)  # the table the cloud's PCA frames were built from, when they were
            else:
                grid = pc.pts_.shape[0] >= ops.KNN_GRID_MIN_POINTS and self.k_ <= 32 and hasattr(pc, "aabb")
                ids = ops.knn_query(pc.pts_, pc.batch_ids_, self.k_, pc.num_batches() if hasattr(pc, "num_batches") else None,
                                    box=pc.aabb() if grid else None, n_valid=getattr(pc, "n_valid_", None))
        else:  # (the words of padded clouds, which only a bounded build is handed; None = every row)
            ids = ops.knn_query_pair(self.pc_src_.pts_, self.pc_src_.batch_ids_, self.samples_.pts_,
                                     self.samples_.batch_ids_, self.k_, n_valid_src=getattr(self.pc_src_, "n_valid_", None),
                                     n_valid_q=getattr(self.samples_, "n_valid_", None))
        if self.capacity_ is not None:
            # the list, its offsets and its edge count from the table on the device: no mask index, no read-back
            self._neighbors_dtype = torch.int32 if self_query else torch.int64
            self.neighbors_i32_, self.start_ids_, self.edge_info_ = ops.knn_edges_bounded(
                ids, self.capacity_, n_valid=getattr(self.samples_, "n_valid_", None))
            self._neighbors = None
            return
        n = ids.shape[0]
        centers = torch.arange(n, dtype=torch.int32, device=ids.device)[:, None].expand(-1, self.k_)
        self.neighbors_ = torch.stack((centers.reshape(-1), ids.reshape(-1)), -1)
        if self.keep_empty_:
            self.start_ids_ = torch.arange(n, dtype=torch.int32, device=ids.device) * self.k_ + self.k_
        else:
            mask = self.neighbors_[:, 1] >= 0
            self.neighbors_ = self.neighbors_[mask]
            self.start_ids_ = torch.cumsum(mask.reshape(n, self.k_).sum(1), 0).to(torch.int32)
        if not self_query:
            self.neighbors_ = self.neighbors_.to(torch.int64)  # what torch_cluster.knn returns

    @property
    def neighbors_(self):
        """The list as the reference exposes it.  A capacity-bounded build materialises it on first access, all
        ``p_capacity`` rows, in the dtype the unbounded build has (int32 for a cloud against itself, int64 between two)."""
        if getattr(self, "_neighbors", None) is None and getattr(self, "neighbors_i32_", None) is not None:
            self._neighbors = self.neighbors_i32_.to(self._neighbors_dtype)
        return getattr(self, "_neighbors", None)

    @neighbors_.setter
    def neighbors_(self, value):  # the base class initialises it to None; the unbounded build and callers attach their own
        self._neighbors = value
        if value is not None:
            self.neighbors_i32_ = None

    def source_major(self):
        """None: the source-major list of a k-NN neighbourhood is the library's transposition of this very list (a second
        query with the roles swapped would find other edges)."""
        return None

    def num_edges(self) -> int:
        """Number of edges as a host integer (one device read-back for a capacity-bounded build)."""
        if self.edge_info_ is None:
            return int(self.neighbors_.shape[0])
        return min(int(self.edge_info_[0]), int(self.capacity_))

    def overflowed(self) -> bool:
        """Whether ``p_capacity`` was too small (one read-back; the list is then truncated: rebuild with a larger one)."""
        return self.edge_info_ is not None and bool(self.edge_info_[1] != 0)


def sample_reference_frames_pca(points, p_neighborhood, axis_fixed=False, dtype=None, device=None):
    """PCA frames from a fixed-k neighbourhood (pc/RotationFunctions.py:307-406), one HIP kernel."""
    ids = p_neighborhood.neighbors_[:, 1].reshape(-1, p_neighborhood.k_)
    return ops.pca_frames(points, ids, axis_fixed)


# --------------------------------------------------------------------------------------- hierarchy
class GridSubSample(object):
    """Grid sub-sampling (pc/GridSubSample.py, pc/Grid.py, pc/BoundingBox.py): one library call builds the cell ids, the
    per-cell point lists and the cell averages (``ops.grid_subsample``).

    ``p_rnd_sample=False``: a level point is the average of its cell (``grid_avg``).  ``p_rnd_sample=True``: ONE random
    point represents each cell (GridSubSample.py:43-54) -- ``ids_`` are its positions in the cell-sorted point list
    ``sorted_ids_`` exactly as in the reference, ``__subsample_tensor__`` gathers those rows whatever the method
    (:66-67), ``__upsample_tensor__`` scatters rows back into zeros (:83-91).  The index choice runs on the device
    (``se3_grid_pick``, no host synchronisation); ``p_rnd_values`` (extension) supplies the uniform numbers in [0,1)
    instead of ``torch.rand`` on the device, one per cell in ascending cell-key order."""

    def __init__(self, p_pc_src, p_cell_size, p_rnd_sample=False, p_rnd_values=None):
        self.pc_src_ = p_pc_src
        self.cell_size_ = p_cell_size
        self.rnd_sample_ = bool(p_rnd_sample)
        self.cells_ = ops.grid_subsample(p_pc_src.pts_, p_pc_src.batch_ids_, p_cell_size, p_pc_src.num_batches())
        self.cell_ids_ = self.cells_.cell_ids
        self.sorted_ids_ = self.cells_.sorted_ids
        self.num_out_ = self.cells_.n_cells
        self.ids_ = None
        if self.rnd_sample_:
            self.ids_, self.picked_ = ops.grid_pick(self.cells_, p_rnd_values)

    @classmethod
    def from_cells(cls, p_pc_src, p_cell_size, p_cells, p_rnd_sample=False):
        """The object the constructor builds, from ``ops.GridCells`` that exist already (one level of
        ``ops.grid_levels_bounded(...).trim()``; a random level carries its ``ids`` / ``picked``)."""
        self = cls.__new__(cls)
        self.pc_src_ = p_pc_src
        self.cell_size_ = p_cell_size
        self.rnd_sample_ = bool(p_rnd_sample)
        self.cells_ = p_cells
        self.cell_ids_ = p_cells.cell_ids
        self.sorted_ids_ = p_cells.sorted_ids
        self.num_out_ = p_cells.n_cells
        self.ids_ = None
        if self.rnd_sample_:
            if getattr(p_cells, "picked", None) is None:
                raise ValueError("GridSubSample.from_cells: a random sub-sample needs the cells' ids / picked")
            self.ids_, self.picked_ = p_cells.ids, p_cells.picked
        return self

    def __subsample_tensor__(self, p_tensor, p_method="avg"):
        if self.rnd_sample_:
            return ops.RowsGather.apply(p_tensor, self.picked_)
        if p_method not in ("avg", "max"):
            raise ValueError(p_method)
        if p_tensor is self.pc_src_.pts_ and p_method == "avg" and not p_tensor.requires_grad:
            return self.cells_.pts
        if p_tensor is self.pc_src_.batch_ids_ and p_method == "max":
            return self.cells_.batch_ids.to(p_tensor.dtype)
        if not p_tensor.is_floating_point():
            return ops.GridPool.apply(p_tensor.to(torch.float32), self.cells_, p_method).to(p_tensor.dtype)
        return ops.GridPool.apply(p_tensor, self.cells_, p_method)

    def __upsample_tensor__(self, p_tensor):
        if self.rnd_sample_:
            if p_tensor.dim() != 2:
                raise ValueError("__upsample_tensor__ of a random grid sub-sample takes [cells, C] tensors (as the reference)")
            return ops.RowsScatter.apply(p_tensor, self.picked_, self.cell_ids_.shape[0])
        if not p_tensor.is_floating_point():
            return p_tensor[self.cell_ids_.to(torch.int64)]
        return ops.GridUpsample.apply(p_tensor, self.cells_)


class FPSSubSample(object):
    """Farthest-point sub-sampling (pc/FPSSubSample.py, which calls ``torch_cluster.fps``): ``ops.fps`` under the contract
    of include/se3conv_fps.h -- per batch element ``min(n_b, ceil(n_b * p_ratio))`` points, each the farthest from those
    picked before it.

    ``ids_`` (int64, as ``torch_cluster`` returns them) are the picked rows of the source cloud in pick order, element after
    element; ``picked_`` the same as int32 for the library's gathers; ``d2_`` the squared distance of every pick to the
    picks before it (extension: the squared coverage radius of every prefix).  ``p_random_start=True`` starts every element
    at a random row, drawn with ``torch.rand`` on the device (the reference's default); ``p_start_values`` (extension, like
    ``p_rnd_values`` of ``GridSubSample``) supplies those numbers in [0,1), one per batch element;
    ``p_random_start=False`` starts at each element's first row.  ``__subsample_tensor__`` gathers the picked rows of a
    tensor of any dtype whatever the method, as the reference indexes (``p_tensor[ids_]``); ``__upsample_tensor__``
    (extension: the reference's method is an unimplemented ``pass``) scatters the rows back into zeros."""

    def __init__(self, p_pc_src, p_ratio, p_random_start=True, p_start_values=None):
        refuse_padded(p_pc_src, "FPSSubSample")
        self.pc_src_ = p_pc_src
        self.ratio_ = float(p_ratio)
        self.random_start_ = bool(p_random_start)
        pts, bid = ops._as(p_pc_src.pts_, torch.float32), ops._as(p_pc_src.batch_ids_, torch.int32)
        n_batches = p_pc_src.num_batches() if hasattr(p_pc_src, "num_batches") else None
        u = None
        if p_start_values is not None:
            if not self.random_start_:
                raise ValueError("FPSSubSample: p_start_values are the draws of a random start (p_random_start=True)")
            u = ops._as(p_start_values, torch.float32).to(pts.device)
        elif self.random_start_:
            if n_batches is None:
                n_batches = int(bid.max().item()) + 1 if bid.numel() else 1
            u = torch.rand(n_batches, device=pts.device)
        ids, self.d2_, self.starts_ = ops.fps(pts, bid, self.ratio_, n_batches, start_u=u).trim()
        self.picked_ = ids
        self.ids_ = ids.to(torch.int64)
        self.num_in_ = int(pts.shape[0])
        self.num_out_ = int(ids.shape[0])

    def __subsample_tensor__(self, p_tensor, p_method="avg"):
        return ops.RowsGather.apply(p_tensor, self.picked_)

    def __upsample_tensor__(self, p_tensor):
        return ops.RowsScatter.apply(p_tensor, self.picked_, self.num_in_)


def _make_sub_sample(p_point_cloud, p_samp_method, p_id, **kwargs):
    """The sub-sampling object of one hierarchy step (pc/PointHierarchy.py:46-52).  A callable method (extension) is
    called with the level's cloud and the level id and returns that object itself."""
    if callable(p_samp_method):
        return p_samp_method(p_point_cloud, p_id)
    if p_samp_method == "grid_avg":
        return GridSubSample(p_point_cloud, kwargs["grid_radii"][p_id], False)
    if p_samp_method == "grid_rnd":
        return GridSubSample(p_point_cloud, kwargs["grid_radii"][p_id], True)
    if p_samp_method == "fps":
        raise NotImplementedError("farthest-point sub-sampling by name (\"fps\", fps_ratios=) is not dispatched: pass a "
                                  "callable instead, PointHierarchy(pc, n, lambda cloud, i: FPSSubSample(cloud, ratios[i])) "
                                  "(INTEGRATION.md)")
    raise ValueError(f"unknown sub-sample method {p_samp_method!r} (grid_avg, grid_rnd, or a callable)")


class PaddedSubSample(object):
    """The sub-sampling step between two PADDED levels (``PointHierarchy(..., p_padded=True)``): the tensors of
    ``struct se3_level`` as ``ops.grid_levels_bounded`` wrote them (``level_`` -- ``cell_ids``, ``sorted_ids``,
    ``cell_ends``, ``pts``, ``batch_ids`` and on random levels ``u``, ``ids``, ``picked``), every one of capacity size, and
    the level's size and overflow flag on the device (``info_ [2]``).  Pooling and up-sampling feature rows through it
    needs ``p_padded_rows`` (``PointHierarchy(..., p_padded=True, p_padded_rows=True)``): ``[n_in, ...]`` floating-point
    tensors padded like the source level become ``[capacity, ...]`` tensors padded like this one and back -- averaged
    levels through ``ops.GridPool`` / ``ops.GridUpsample`` over all ``capacity`` cells (``cells_``; ``avg`` / ``max``), random
    levels through
    ``ops.RowsGatherPadded`` / ``ops.RowsUnpickPadded``; no absent row or dropped cell is read, and their rows are zero."""

    def __init__(self, p_pc_src, p_cell_size, p_level, p_info, p_rnd_sample=False, p_padded_rows=False):
        self.pc_src_, self.cell_size_, self.level_, self.info_ = p_pc_src, p_cell_size, p_level, p_info
        self.rnd_sample_ = bool(p_rnd_sample)
        self.padded_rows_ = bool(p_padded_rows)
        self.cells_ = ops.GridCells.of_level(p_level)
        self.cell_ids_, self.sorted_ids_ = p_level["cell_ids"], p_level["sorted_ids"]
        self.capacity_ = int(p_level["pts"].shape[0])

    def __subsample_tensor__(self, p_tensor, p_method="avg"):
        if self.padded_rows_:
            if p_tensor is self.pc_src_.pts_ and p_method == "avg" and not p_tensor.requires_grad:
                return self.level_["pts"]
            if p_tensor is self.pc_src_.batch_ids_ and p_method == "max":
                return self.level_["batch_ids"]
            if not p_tensor.is_floating_point():
                raise ValueError("pool_tensor on padded levels takes floating-point tensors only (the level's points and "
                                 "batch ids are its own buffers)")
            if self.rnd_sample_:
                return ops.RowsGatherPadded.apply(p_tensor, self.cell_ids_, self.level_["picked"])
            if p_method not in ("avg", "max"):
                raise ValueError(p_method)
            return ops.GridPool.apply(p_tensor, self.cells_, p_method)
        raise NotImplementedError("pool_tensor on padded levels (p_padded=True) is not implemented: the pooled rows would "
                                  "need the level's present-row count, which is a device word")

    def __upsample_tensor__(self, p_tensor):
        if self.padded_rows_:
            if not p_tensor.is_floating_point():
                raise ValueError("upsample_tensor on padded levels takes floating-point tensors only")
            if self.rnd_sample_:
                if p_tensor.dim() != 2:
                    raise ValueError("__upsample_tensor__ of a random grid sub-sample takes [cells, C] tensors (as the "
                                     "reference)")
                return ops.RowsUnpickPadded.apply(p_tensor, self.cell_ids_, self.level_["picked"])
            return ops.GridUpsample.apply(p_tensor, self.cells_)
        raise NotImplementedError("upsample_tensor on padded levels (p_padded=True) is not implemented: the absent rows' "
                                  "cell ids are -1")


class PointHierarchy(object):
    """``p_subsample_method``: ``"grid_avg"``, ``"grid_rnd"``, or (extension) a callable ``(level_cloud, level_id) ->
    sub-sample object``, e.g. ``lambda cloud, i: FPSSubSample(cloud, 0.25)``; a callable builds level after level and takes
    neither ``p_capacities`` nor ``p_padded``.

    ``p_capacities`` (extension): None builds level after level, each with its own read-back of the level size.
    ``"input"`` or one row count per level builds ALL levels with one library call into buffers of those sizes
    (``ops.grid_levels_bounded``; ``"input"``: the row count of level 0, which cannot overflow) and reads every level size
    back with one copy; the clouds and sub-sample objects are the same, bit for bit.  ``ops.LevelOverflow`` when a level
    does not fit.  Neighbourhoods and frames are then built on the trimmed levels (on the padded ones: ``p_padded``).

    ``p_padded=True`` (extension, needs ``p_capacities``): nothing is trimmed and nothing is read back.  Every level cloud is
    the capacity-sized buffer of its level as a PADDED cloud (``Pointcloud(..., p_n_valid=)``) whose ``n_valid_`` word holds
    ``min(level size, capacity)``; frames and ball-query neighbourhoods of the levels never read the absent rows
    (include/se3conv_padded.h), so that hierarchy, frames, neighbourhoods and convolutions capture into one HIP graph that
    can be replayed on a batch with another point count.  Level 0 may be a padded cloud itself.  ``level_sizes()`` and
    ``overflowed()`` are the read-backs, done only when asked.  ``pool_tensor`` / ``upsample_tensor`` are not implemented
    on padded levels unless the hierarchy is flagged:

    ``p_padded_rows=True`` (extension, needs ``p_padded``): every level cloud the hierarchy builds carries the flag
    (``Pointcloud(..., p_padded_rows=True)``: feature tensors padded like the points, the glue skips absent rows and writes
    zeros there), and ``pool_tensor`` / ``upsample_tensor`` work on such tensors (``PaddedSubSample``)."""

    def __init__(self, p_point_cloud, p_num_sub_samples, p_subsample_method="grid_avg", p_capacities=None, p_padded=False,
                 p_padded_rows=False, **kwargs):
        self.sub_sampled_objs_ = []
        self.pcs_ = [p_point_cloud]
        self.padded_ = bool(p_padded)
        self.padded_rows_ = bool(p_padded_rows)
        if self.padded_rows_ and not self.padded_:
            raise ValueError("PointHierarchy: p_padded_rows=True needs p_padded=True")
        self.level_info_ = None
        cur = p_point_cloud
        if callable(p_subsample_method) and (p_capacities is not None or self.padded_):
            raise ValueError("PointHierarchy: a callable sub-sample method builds level after level; it takes neither "
                             "p_capacities nor p_padded (bounded levels are grid levels)")
        if self.padded_:
            if p_capacities is None:
                raise ValueError("PointHierarchy: p_padded=True needs p_capacities ('input' or one row count per level)")
            if p_subsample_method not in ("grid_avg", "grid_rnd"):
                _make_sub_sample(p_point_cloud, p_subsample_method, 0, **kwargs)  # (raises: the methods' one error text)
            if p_num_sub_samples > 0:
                rnd = p_subsample_method == "grid_rnd"
                radii = [kwargs["grid_radii"][i] for i in range(p_num_sub_samples)]
                built = ops.grid_levels_bounded(cur.pts_, cur.batch_ids_, radii, p_capacities, cur.num_batches(),
                                                n_valid=getattr(cur, "n_valid_", None), rnd=[rnd] * p_num_sub_samples)
                self.level_info_ = built.info
                self._levels_keep = built
                for i, lv in enumerate(built.levels):
                    # the level's row-count word: min(true cell count, capacity), formed on the device
                    word = torch.clamp(built.info[i, 0:1], max=int(built.capacities[i]))
                    samp = PaddedSubSample(cur, radii[i], lv, built.info[i], rnd, self.padded_rows_)
                    cur = self.__padded_level_cloud__(cur, lv["pts"], lv["batch_ids"], word)
                    self.sub_sampled_objs_.append(samp)
                    self.pcs_.append(cur)
        elif p_capacities is None:
            for i in range(p_num_sub_samples):
                new_pc, samp = self.__create_sub_sample__(cur, p_subsample_method, i, **kwargs)
                self.sub_sampled_objs_.append(samp)
                self.pcs_.append(new_pc)
                cur = new_pc
        elif p_num_sub_samples > 0:
            if p_subsample_method not in ("grid_avg", "grid_rnd"):
                _make_sub_sample(p_point_cloud, p_subsample_method, 0, **kwargs)  # (raises: the methods' one error text)
            rnd = p_subsample_method == "grid_rnd"
            radii = [kwargs["grid_radii"][i] for i in range(p_num_sub_samples)]
            levels = ops.grid_levels_bounded(ops._as(cur.pts_, torch.float32), ops._as(cur.batch_ids_, torch.int32), radii,
                                             p_capacities, cur.num_batches(), rnd=[rnd] * p_num_sub_samples).trim()
            for i, cells in enumerate(levels):
                samp = GridSubSample.from_cells(cur, radii[i], cells, rnd)
                cur = self.__level_cloud__(cur, samp)
                self.sub_sampled_objs_.append(samp)
                self.pcs_.append(cur)
        self.neigh_cache_ = {}

    def __create_sub_sample__(self, p_point_cloud, p_samp_method, p_id, **kwargs):
        samp = _make_sub_sample(p_point_cloud, p_samp_method, p_id, **kwargs)
        return self.__level_cloud__(p_point_cloud, samp), samp

    def __level_cloud__(self, p_point_cloud, p_samp):
        new_pts = p_samp.__subsample_tensor__(p_point_cloud.pts_, "avg")
        new_bid = p_samp.__subsample_tensor__(p_point_cloud.batch_ids_, "max")
        return Pointcloud(new_pts, new_bid, num_batches=_batches_of(p_point_cloud))

    def __padded_level_cloud__(self, p_point_cloud, p_pts, p_batch_ids, p_word):
        return Pointcloud(p_pts, p_batch_ids, p_n_valid=p_word, num_batches=_batches_of(p_point_cloud),
                          p_padded_rows=self.padded_rows_)

    def level_sizes(self):
        """Present rows of every level as host integers (level 0 included): the read-back of a padded hierarchy, done
        only when asked.  An ordinary hierarchy answers from its shapes."""
        if not self.padded_:
            return [int(pc.pts_.shape[0]) for pc in self.pcs_]
        words = [pc.n_valid_.reshape(1) if is_padded(pc) else None for pc in self.pcs_]
        vals = torch.cat([w for w in words if w is not None]).cpu().tolist() if any(w is not None for w in words) else []
        out = []
        for pc, w in zip(self.pcs_, words):
            n = int(pc.pts_.shape[0])
            out.append(n if w is None else min(max(int(vals.pop(0)), 0), n))
        return out

    def overflowed(self) -> bool:
        """Whether a level of a padded hierarchy had more cells than its capacity (one read-back; the level and every
        deeper one are then those of the truncated hierarchy: build again with larger capacities)."""
        return self.level_info_ is not None and bool((self.level_info_[:, 1] != 0).any())

    def create_neighborhood(self, p_pc_src_id, p_pc_dest_id, p_neigh_method, **kwargs):
        """Memoised per (source level, destination level, method + its parameter), pc/PointHierarchy.py:60-79 (the k-NN
        keyword is spelled ``neihg_k`` there; ``neigh_k`` is accepted too).  ``bq_max_neighbors`` (> 0) and ``bq_seed`` cap a ball-query
        neighbourhood (``BQNeighborhood``); they enter the key only then.  ``bq_capacity`` / ``knn_capacity`` (extension): a
        capacity-bounded list (``p_capacity`` of the neighbourhood classes); the capacity enters the key."""
        cap = int(kwargs.get("bq_max_neighbors", 0) or 0) if p_neigh_method == "ball_query" else 0
        if p_neigh_method == "ball_query":
            param = kwargs["bq_radius"]
        elif p_neigh_method == "knn":
            param = kwargs["neihg_k"] if "neihg_k" in kwargs else kwargs["neigh_k"]
        else:
            raise ValueError(f"unknown neighbourhood method {p_neigh_method!r} (ball_query, knn)")
        key = f"{p_pc_src_id}_{p_pc_dest_id}_{p_neigh_method}{param}"
        capacity = kwargs.get("bq_capacity") if p_neigh_method == "ball_query" else kwargs.get("knn_capacity")
        if capacity is not None:  # (extension: a capacity-bounded list, *Neighborhood(p_capacity=); padded levels need it)
            key += f"_cap{int(capacity)}"
        if cap > 0:  # (a capped neighbourhood is another list, and so is one drawn with another seed)
            key += f"_max{cap}_seed{kwargs.get('bq_seed')}"
        if key not in self.neigh_cache_:
            src, dst = self.pcs_[p_pc_src_id], self.pcs_[p_pc_dest_id]
            self.neigh_cache_[key] = BQNeighborhood(src, dst, param, cap, p_capacity=capacity, p_seed=kwargs.get("bq_seed")) \
                if p_neigh_method == "ball_query" else KnnNeighborhood(src, dst, param, p_capacity=capacity)
        return self.neigh_cache_[key]

    def clear_neigh_cache(self):
        self.neigh_cache_ = {}

    def pool_tensor(self, p_tensor, p_pc_src_id, p_pc_dest_id, p_pool_method):
        assert p_pc_dest_id - p_pc_src_id == 1
        return self.sub_sampled_objs_[p_pc_src_id].__subsample_tensor__(p_tensor, p_pool_method)

    def upsample_tensor(self, p_tensor, p_pc_src_id, p_pc_dest_id):
        assert p_pc_src_id - p_pc_dest_id == 1
        return self.sub_sampled_objs_[p_pc_dest_id].__upsample_tensor__(p_tensor)


class PointHierarchyRotEquiv(PointHierarchy):
    """Every level gets its own freshly sampled frames (pc/PointHierarchyRotEquiv.py:31-44)."""

    def __level_cloud__(self, p_point_cloud, p_samp):
        new_pts = p_samp.__subsample_tensor__(p_point_cloud.pts_, "avg")
        new_bid = p_samp.__subsample_tensor__(p_point_cloud.batch_ids_, "max")
        return PointcloudRotEquiv(new_pts, new_bid, p_point_cloud.local_frames_config_,
                                  num_batches=_batches_of(p_point_cloud))

    def __padded_level_cloud__(self, p_point_cloud, p_pts, p_batch_ids, p_word):
        return PointcloudRotEquiv(p_pts, p_batch_ids, p_point_cloud.local_frames_config_, p_n_valid=p_word,
                                  num_batches=_batches_of(p_point_cloud), p_padded_rows=self.padded_rows_)
