"""The augmentation pipeline on the device (include/se3conv_augment.h): the classes and config dictionaries of the reference's
``point_cloud_lib.augment``, run on a whole batch at once.

Every batch element is augmented on its own, as the reference's loaders do per scene inside ``Dataset.__getitem__``; every
random choice is a column of ``draws [steps, n_batches, AUG_DRAWS]`` (column 0: the step's gate, ``u <= p_prob``) or a hashed
function of a seed word, nothing is read back, and the steps that remove points (``CropPtsAug``, ``CropBoxAug``,
``DropAug(p_keep_zeros=False)``) write into padded clouds: the result keeps its ``n_rows``, the surviving count is the device
word ``n_valid_``, and ``Pointcloud(pts_, batch_ids_, p_n_valid=n_valid_)`` takes it as it is.  There is no CPU fallback.

``AugPipeline.augment_batch`` folds consecutive affine steps (rotations, centre, linear, mirror, translation, std-dev
normalisation) into one table per element, takes statistics only in front of a step that needs them (of the cloud under
the table: the transformed cloud is not written for that), and writes points only in front of a step that is not affine
(``NoiseAug`` is added in that same pass) and at the end.

Differences from the reference, all stated in the header: ``CropBoxAug`` draws its box once (an element whose box holds no
point comes out empty, the reference draws again); ``CropPtsAug`` breaks distance ties by row order; the Gaussian numbers are
Box-Muller on hashed words; ``RotationAug3D`` makes its quaternion from four uniform draws; ``LinearAug``'s per-epoch value
tables are taken in float32.

``ElasticDistortionAug`` (include/se3conv_elastic.h) is opt-in, ``AugPipeline(p_elastic=True)``; without the switch the name is
refused as before.  It is a switch because the step needs a grid buffer the caller sizes (``grid_capacity``, in cells: nothing
is read back to size it, an element that does not fit stays undistorted and ``overflow_`` says so), and because its random
field is the hash's, reproducible from (seed, step, element), not torch's ``randn`` stream."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

AUG_DRAWS = _lib.AUG_DRAWS
_AFFINE = ("rot_axis", "rot_3d", "center", "linear", "mirror", "translation", "stdnorm")
_NEEDS_STATS = ("center", "translation", "stdnorm", "crop_box")


# ------------------------------------------------------------------------------------------------- the entry points, one by one
def _cloud(pts, batch_ids, who):
    ops._padded_cloud(pts, batch_ids, who)
    return pts.device, int(pts.shape[0])


def _consts(values) -> C.Array:
    arr = (C.c_double * _lib.AUG_CONSTS)()
    for i, v in enumerate(values):
        arr[i] = float(v)
    return arr


def _seed_word(seed_tensor, dev):
    if seed_tensor is not None and (seed_tensor.numel() != 1 or seed_tensor.dtype != torch.int32):
        raise ValueError("seed_tensor must be a 1-element int32 tensor")
    return ops._ptr(seed_tensor, torch.int32, "seed_tensor", dev)


def aug_stats(pts, batch_ids, n_batches: int, affine=None, n_valid=None):
    """``(counts [B] int32, stats [B, 12] = min | max | mean | unbiased std)`` of ``pts @ M_b + t_b`` per element
    (``se3_aug_stats``): fixed order of additions in float64, bit-reproducible, the same bits on a padded cloud."""
    dev, n = _cloud(pts, batch_ids, "aug_stats")
    lib = _lib.load()
    counts = ops._empty(n_batches, dtype=torch.int32, device=dev)
    stats = ops._empty((n_batches, 12), dtype=torch.float32, device=dev)
    nbytes = lib.se3_aug_stats_workspace_bytes(n, n_batches)
    ws = ops._workspace(nbytes, dev)
    _lib.check(lib.se3_aug_stats(ops._ptr(pts, torch.float32, "pts"), ops._ptr(batch_ids, torch.int32, "batch_ids", dev), n,
                                 ops._valid_word(n_valid, dev, "aug_stats"), n_batches, ops._ptr(affine, torch.float32, "affine", dev),
                                 ops._ptr(counts, torch.int32, "counts"), ops._ptr(stats, torch.float32, "stats"),
                                 C.c_void_p(ws.data_ptr()), nbytes, ops._stream(dev)), "se3_aug_stats")
    return counts, stats


def aug_affine_step(kind: str, consts, prob: float, draws, affine, counts=None, stats=None):
    """Compose one step into ``affine [B, 12]`` in place (``se3_aug_affine_step``)."""
    dev = affine.device
    _lib.check(_lib.load().se3_aug_affine_step(_lib.AUG_KINDS[kind], _consts(consts), float(prob), ops._ptr(draws, torch.float32, "draws", dev),
                                               ops._ptr(counts, torch.int32, "counts", dev), ops._ptr(stats, torch.float32, "stats", dev),
                                               affine.shape[0], ops._ptr(affine, torch.float32, "affine"), ops._stream(dev)),
               "se3_aug_affine_step")
    return affine


def aug_apply(x, batch_ids, n_batches: int, affine=None, linear_only: bool = False, noise=None, seed: int = 0, seed_tensor=None,
              step: int = 0, ones_mask=None, n_valid=None):
    """``x @ M_b + t_b`` per row into a new tensor (``se3_aug_apply``).  ``noise``: None or ``(draws [B, AUG_DRAWS], prob, sigma,
    clip or None[, scale])``, ``scale`` 1 for points and sigma for an extra tensor (NoiseAug.py:58-61); ``ones_mask``: uint8 per row, rows with 0 come out as ones."""
    dev, n = _cloud(x, batch_ids, "aug_apply")
    y = ops._empty((n, 3), dtype=torch.float32, device=dev)
    nd, nprob, nsigma, nclip = (None, 0.0, 0.0, -1.0) if noise is None else (noise[0], noise[1], noise[2], -1.0 if noise[3] is None else noise[3])
    nscale = noise[4] if noise is not None and len(noise) > 4 else 1.0
    _lib.check(_lib.load().se3_aug_apply(
        ops._ptr(x, torch.float32, "x"), ops._ptr(batch_ids, torch.int32, "batch_ids", dev), n, ops._valid_word(n_valid, dev, "aug_apply"),
        n_batches, ops._ptr(affine, torch.float32, "affine", dev), int(bool(linear_only)), ops._ptr(nd, torch.float32, "noise draws", dev),
        float(nprob), float(nsigma), float(nclip), float(nscale), int(seed) & 0xFFFFFFFF, _seed_word(seed_tensor, dev), int(step),
        ops._ptr(ones_mask, torch.uint8, "ones_mask", dev), ops._ptr(y, torch.float32, "y"), ops._stream(dev)), "se3_aug_apply")
    return y


def aug_keep_mask(kind: str, consts, prob: float, pts, batch_ids, n_batches: int, draws, stats=None, seed: int = 0, seed_tensor=None,
                  step: int = 0, n_valid=None):
    """One byte per row, 1 = keep (``se3_aug_keep_mask``): ``"drop"``, ``"crop_box"``, ``"crop_pts"``."""
    dev, n = _cloud(pts, batch_ids, "aug_keep_mask")
    mask = ops._empty(n, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().se3_aug_keep_mask(
        _lib.AUG_KINDS[kind], _consts(consts), float(prob), ops._ptr(pts, torch.float32, "pts"),
        ops._ptr(batch_ids, torch.int32, "batch_ids", dev), n, ops._valid_word(n_valid, dev, "aug_keep_mask"), n_batches,
        ops._ptr(draws, torch.float32, "draws", dev), ops._ptr(stats, torch.float32, "stats", dev), int(seed) & 0xFFFFFFFF,
        _seed_word(seed_tensor, dev), int(step), ops._ptr(mask, torch.uint8, "mask"), ops._stream(dev)), "se3_aug_keep_mask")
    return mask


def aug_compact(mask, batch_ids, n_batches: int, n_valid=None, idx_in=None):
    """``(idx [n_rows] int32, n_out [1] int32, counts [B] int32, idx_orig)``: the kept rows in order, -1 behind them
    (``se3_aug_compact``); with ``idx_in`` (the ``idx`` of an earlier compaction) ``idx_orig`` is the composition, else None."""
    dev, n = mask.device, int(mask.shape[0])
    lib = _lib.load()
    idx = ops._empty(n, dtype=torch.int32, device=dev)
    idx_orig = ops._empty(n, dtype=torch.int32, device=dev) if idx_in is not None else None
    n_out = ops._empty(1, dtype=torch.int32, device=dev)
    counts = ops._empty(n_batches, dtype=torch.int32, device=dev)
    nbytes = lib.se3_aug_compact_workspace_bytes(n)
    ws = ops._workspace(nbytes, dev)
    _lib.check(lib.se3_aug_compact(ops._ptr(mask, torch.uint8, "mask"), ops._ptr(batch_ids, torch.int32, "batch_ids", dev), n,
                                   ops._valid_word(n_valid, dev, "aug_compact"), n_batches, ops._ptr(idx_in, torch.int32, "idx_in", dev),
                                   ops._ptr(idx, torch.int32, "idx"), ops._ptr(idx_orig, torch.int32, "idx_orig"), ops._ptr(n_out, torch.int32, "n_out"),
                                   ops._ptr(counts, torch.int32, "counts"), C.c_void_p(ws.data_ptr()), nbytes, ops._stream(dev)),
               "se3_aug_compact")
    return idx, n_out, counts, idx_orig


def _octaves(values, what) -> C.Array:
    if not 1 <= len(values) <= _lib.ELASTIC_MAX_OCTAVES:
        raise ValueError(f"{what}: 1 to {_lib.ELASTIC_MAX_OCTAVES} octaves, got {len(values)}")
    return (C.c_double * len(values))(*[float(v) for v in values])


def aug_elastic_plan(counts, stats, draws, prob: float, granularity, grid_capacity: int):
    """``(grid_table [B, L, 4] int64 = (nx, ny, nz, offset), overflow [1] int32, workspace)`` (``se3_elastic_plan``): the noise
    grid of every (element, octave) laid into ``grid_capacity`` cells; offset -1 for an element that is not distorted; the
    workspace holds the tile prefix ``aug_elastic_grids`` deals its tiles by."""
    dev, nb = stats.device, int(stats.shape[0])
    lib = _lib.load()
    g = _octaves(granularity, "p_granularity")
    table = ops._empty((nb, len(g), 4), dtype=torch.int64, device=dev)
    overflow = ops._empty(1, dtype=torch.int32, device=dev)
    nbytes = lib.se3_elastic_workspace_bytes(nb, len(g))
    ws = ops._workspace(nbytes, dev)
    _lib.check(lib.se3_elastic_plan(ops._ptr(counts, torch.int32, "counts", dev), ops._ptr(stats, torch.float32, "stats"),
                                    ops._ptr(draws, torch.float32, "draws", dev), float(prob), g, len(g), nb, int(grid_capacity),
                                    ops._ptr(table, torch.int64, "grid_table"), ops._ptr(overflow, torch.int32, "overflow"),
                                    C.c_void_p(ws.data_ptr()), nbytes, ops._stream(dev)), "se3_elastic_plan")
    return table, overflow, ws


def aug_elastic_grids(grid_table, workspace, grid_capacity: int, seed: int = 0, seed_tensor=None, step: int = 0, noise_in=None, grid=None):
    """``grid [grid_capacity, 4]`` float32 (``se3_elastic_grids``): the blurred noise of every placed entry of ``grid_table``,
    lanes 0..2 the displacement along x, y, z.  ``noise_in`` (same layout): raw numbers in place of the hash's; ``grid``: a
    buffer to write into (rows behind the placed total are left as they are)."""
    dev, (nb, nl) = grid_table.device, (int(grid_table.shape[0]), int(grid_table.shape[1]))
    cap = int(grid_capacity)
    if grid is None:
        grid = ops._empty((max(cap, 1), 4), dtype=torch.float32, device=dev)   # (one row at least: a pointer to hand on)
    for name, buf in (("grid", grid), ("noise_in", noise_in)):
        if buf is not None and (buf.dim() != 2 or buf.shape[1] != 4 or buf.shape[0] < cap):
            raise ValueError(f"{name}: expected [>= {cap}, 4], got {tuple(buf.shape)}")
    _lib.check(_lib.load().se3_elastic_grids(
        ops._ptr(grid_table, torch.int64, "grid_table"), nb, nl, cap, int(seed) & 0xFFFFFFFF, _seed_word(seed_tensor, dev), int(step),
        ops._ptr(noise_in, torch.float32, "noise_in", dev), ops._ptr(grid, torch.float32, "grid", dev), C.c_void_p(workspace.data_ptr()),
        int(workspace.numel()), ops._stream(dev)), "se3_elastic_grids")
    return grid


def aug_elastic_displace(x, batch_ids, n_batches: int, stats, grid_table, magnitude, grid, n_valid=None):
    """The rows of every distorted element moved through their octaves in turn, the others copied (``se3_elastic_displace``)."""
    dev, n = _cloud(x, batch_ids, "aug_elastic_displace")
    m = _octaves(magnitude, "p_magnitude")
    if tuple(grid_table.shape) != (n_batches, len(m), 4):
        raise ValueError(f"grid_table: expected {(n_batches, len(m), 4)}, got {tuple(grid_table.shape)}")
    y = ops._empty((n, 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().se3_elastic_displace(
        ops._ptr(x, torch.float32, "x"), ops._ptr(batch_ids, torch.int32, "batch_ids", dev), n, ops._valid_word(n_valid, dev, "aug_elastic_displace"),
        n_batches, ops._ptr(stats, torch.float32, "stats", dev), ops._ptr(grid_table, torch.int64, "grid_table", dev), len(m), m,
        ops._ptr(grid, torch.float32, "grid", dev), ops._ptr(y, torch.float32, "y"), ops._stream(dev)), "se3_elastic_displace")
    return y


# ------------------------------------------------------------------------------------------------------------------ the classes
class Augmentation:
    """Base class (the reference's ``Augmentation``): ``prob_``, ``apply_extra_tensors_``, the epoch counter of the per-epoch
    value tables.  ``kind_`` names the step of the header, ``_consts()`` its constants for the current epoch."""
    kind_: Optional[str] = None

    def __init__(self, p_prob, p_apply_extra_tensors, **kwargs):
        self.prob_ = p_prob
        self.apply_extra_tensors_ = p_apply_extra_tensors
        self.epoch_iter_ = 0

    def increase_epoch_counter(self):
        self.epoch_iter_ += 1

    def reset_epoch_counter(self):
        self.epoch_iter_ = 0

    def _consts(self) -> list:
        raise NotImplementedError


class RotationAug(Augmentation):
    kind_ = "rot_axis"

    def __init__(self, p_prob=1.0, p_axis=0, p_min_angle=0, p_max_angle=2 * np.pi, p_angle_values=None, p_apply_extra_tensors=[], **kwargs):
        if p_axis not in (0, 1, 2):
            raise ValueError(f"RotationAug: p_axis {p_axis}")
        self.axis_, self.min_angle_, self.max_angle_, self.angle_values_ = p_axis, p_min_angle, p_max_angle, p_angle_values
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        if self.angle_values_ is not None:
            return [self.axis_, self.angle_values_[self.epoch_iter_], 0.0, 1.0]
        return [self.axis_, self.min_angle_, self.max_angle_, 0.0]


class RotationAug3D(Augmentation):
    kind_ = "rot_3d"

    def __init__(self, p_prob=1.0, p_apply_extra_tensors=[], p_axis=None, **kwargs):
        if p_axis not in (None, 0, 1, 2):
            raise ValueError(f"RotationAug3D: p_axis {p_axis}")
        self.axis_ = p_axis
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return [-1.0 if self.axis_ is None else self.axis_]


class CenterAug(Augmentation):
    kind_ = "center"

    def __init__(self, p_axes=[True, True, True], p_method="mean", p_apply_extra_tensors=[], **kwargs):
        if p_method != "mean":  # (the reference's "max" / "min" subtract the tuple torch.max returns: they raise there)
            raise NotImplementedError(f"CenterAug: p_method {p_method!r}")
        self.axes_, self.method_ = p_axes, p_method
        super().__init__(1.0, p_apply_extra_tensors)

    def _consts(self):
        return [float(bool(a)) for a in self.axes_]


class LinearAug(Augmentation):
    kind_ = "linear"

    def __init__(self, p_prob=1.0, p_min_a=0.9, p_max_a=1.1, p_min_b=-0.1, p_max_b=0.1, p_a_values=None, p_b_values=None,
                 p_channel_independent=False, p_apply_extra_tensors=[], **kwargs):
        self.min_a_, self.max_a_, self.min_b_, self.max_b_ = p_min_a, p_max_a, p_min_b, p_max_b
        self.a_values_, self.b_values_, self.channel_independent_ = p_a_values, p_b_values, p_channel_independent
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        c = [self.max_a_ - self.min_a_, self.min_a_, self.max_b_ - self.min_b_, self.min_b_,
             float(bool(self.channel_independent_) and self.a_values_ is None), 0.0] + [0.0] * 6
        if self.a_values_ is not None:
            c[5] = 1.0
            c[6:9] = np.broadcast_to(np.asarray(self.a_values_[self.epoch_iter_], dtype=np.float64), (3,)).tolist()
            c[9:12] = np.broadcast_to(np.asarray(self.b_values_[self.epoch_iter_], dtype=np.float64), (3,)).tolist()
        return c


class MirrorAug(Augmentation):
    kind_ = "mirror"

    def __init__(self, p_prob=1.0, p_mirror_prob=0.5, p_axes=[True, True, False], p_apply_extra_tensors=[], **kwargs):
        self.axes_, self.mirror_prob_ = p_axes, p_mirror_prob
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return [self.mirror_prob_] + [float(bool(a)) for a in self.axes_]


class TranslationAug(Augmentation):
    kind_ = "translation"

    def __init__(self, p_prob=1.0, p_max_aabb_ratio=1.0, p_apply_extra_tensors=[], **kwargs):
        self.max_aabb_ratio_ = p_max_aabb_ratio
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return np.broadcast_to(np.asarray(self.max_aabb_ratio_, dtype=np.float64), (3,)).tolist()


class STDDevNormAug(Augmentation):
    kind_ = "stdnorm"

    def __init__(self, p_new_std=1.0, p_apply_extra_tensors=[], **kwargs):
        self.stddev_ = p_new_std
        super().__init__(1.0, p_apply_extra_tensors)

    def _consts(self):
        return [self.stddev_]


class NoiseAug(Augmentation):
    kind_ = "noise"

    def __init__(self, p_prob=1.0, p_stddev=0.005, p_clip=None, p_apply_extra_tensors=[], **kwargs):
        self.stddev_, self.clip_ = p_stddev, p_clip
        super().__init__(p_prob, p_apply_extra_tensors)


class DropAug(Augmentation):
    kind_ = "drop"

    def __init__(self, p_prob=1.0, p_apply_extra_tensors=[], p_drop_prob=0.05, p_keep_zeros=True, **kwargs):
        self.drop_prob_, self.keep_zeros_ = p_drop_prob, p_keep_zeros
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return [self.drop_prob_]


class CropBoxAug(Augmentation):
    kind_ = "crop_box"

    def __init__(self, p_prob=1.0, p_min_crop_size=0.5, p_max_crop_size=1.0, p_apply_extra_tensors=[], **kwargs):
        self.min_crop_size_, self.max_crop_size_ = p_min_crop_size, p_max_crop_size
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return [self.max_crop_size_ - self.min_crop_size_, self.min_crop_size_]


class CropPtsAug(Augmentation):
    kind_ = "crop_pts"

    def __init__(self, p_prob=1.0, p_max_pts=0, p_crop_ratio=1.0, p_apply_extra_tensors=[], **kwargs):
        self.max_pts_, self.crop_ratio_ = p_max_pts, p_crop_ratio
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return [self.max_pts_, self.crop_ratio_]


class ElasticDistortionAug(Augmentation):
    """One blurred noise grid per octave, sampled at the points the octave before moved (include/se3conv_elastic.h).  The
    reference returns the extra tensors untouched whatever their flags (ElasticDistortionAug.py:91), and so does this one."""
    kind_ = "elastic"

    def __init__(self, p_prob=1.0, p_granularity=[0.1], p_magnitude=[0.2], p_apply_extra_tensors=[], **kwargs):
        if len(p_granularity) != len(p_magnitude) or not 1 <= len(p_granularity) <= _lib.ELASTIC_MAX_OCTAVES:
            raise ValueError(f"ElasticDistortionAug: p_granularity and p_magnitude are lists of one length, 1 to {_lib.ELASTIC_MAX_OCTAVES} "
                             f"octaves; got {len(p_granularity)} and {len(p_magnitude)}")
        if not all(float(g) > 0 for g in p_granularity):
            raise ValueError(f"ElasticDistortionAug: p_granularity {list(p_granularity)}")
        self.granularity_, self.magnitude_ = list(p_granularity), list(p_magnitude)
        super().__init__(p_prob, p_apply_extra_tensors)

    def _consts(self):
        return self.granularity_ + self.magnitude_


OPT_IN = ("ElasticDistortionAug",)   # names AugPipeline knows only with p_elastic=True; refused as not implemented without


class AugmentedBatch:
    """What ``AugPipeline.augment_batch`` returns.  ``pts_ [n_rows, 3]`` and ``batch_ids_`` are padded like the input;
    ``n_valid_`` is the device word of present rows (None when nothing can remove points and none was given); ``idx_`` the
    original row of every surviving row (-1 behind them; None without a removal); ``extra_tensors_`` the extra tensors, the
    cropped ones padded like the points; ``affine_`` the composed table of the last write of the points (None: none was
    needed); ``overflow_`` the flag of the elastic grid, a device word (bit 0: an element did not fit into ``grid_capacity`` and
    stayed undistorted, bit 1: an element's box was not finite; the OR over the pipeline's elastic steps), None for a
    pipeline without that step."""

    def __init__(self, pts, batch_ids, n_valid, idx, extra_tensors, affine, cropped, extra_n_valid, overflow=None):
        self.pts_, self.batch_ids_, self.n_valid_, self.idx_ = pts, batch_ids, n_valid, idx
        self.extra_tensors_, self.affine_, self.overflow_ = extra_tensors, affine, overflow
        self.cropped_ = cropped   # per extra tensor: whether it went through a compaction
        self.extra_n_valid_ = extra_n_valid   # per extra tensor: the device word of ITS present rows (the points' word only for
        #                                       those that went through every removing step; None: all rows)


class AugPipeline:
    """The reference's ``AugPipeline``: ``create_pipeline(list of dict)`` with the classes looked up by ``name``.

    ``p_elastic=True`` makes ``ElasticDistortionAug`` known, so that the reference's ScanNet training lists are taken
    unchanged.  It is a switch and off by default for two reasons: the step needs a grid the caller sizes (``augment_batch(...,
    grid_capacity=cells)``; a pipeline that holds the step cannot run without it), and its random field comes from the hash of
    (seed, step, element), not from torch's ``randn`` stream as in the reference."""

    def __init__(self, p_elastic: bool = False):
        self.elastic_ = bool(p_elastic)
        self.aug_classes_ = {sub.__name__: sub for sub in Augmentation.__subclasses__() if self.elastic_ or sub.__name__ not in OPT_IN}
        self.pipeline_: List[Augmentation] = []
        self._identity = {}   # (device, n_batches) -> the identity table; made on first use, copied (never zero-filled) afterwards

    def create_pipeline(self, p_dict_list):
        pipeline = []
        for cur_dict in p_dict_list:
            name = cur_dict["name"]
            if name in OPT_IN and not self.elastic_:
                raise NotImplementedError(f"{name} is not implemented on the device")
            if name not in self.aug_classes_:
                raise KeyError(f"unknown augmentation {name!r}: known are {sorted(self.aug_classes_)}")
            pipeline.append(self.aug_classes_[name](**cur_dict))
        self.pipeline_ = pipeline

    def increase_epoch_counter(self):
        for cur_aug in self.pipeline_:
            cur_aug.increase_epoch_counter()

    def reset_epoch_counter(self):
        for cur_aug in self.pipeline_:
            cur_aug.reset_epoch_counter()

    def removes_points(self) -> bool:
        return any(a.kind_ in ("crop_box", "crop_pts") or (a.kind_ == "drop" and not a.keep_zeros_) for a in self.pipeline_)

    def elastic_capacity(self, extent, n_batches: int = 1) -> int:
        """Cells that ``n_batches`` elements of box ``extent`` (3 numbers) need in the largest elastic step of the pipeline, however
        the steps in front of it turn the cloud (they may scale it, by ``LinearAug``'s largest factor, and rotate it, so every axis
        is given the scaled diagonal): a host-side upper bound for ``grid_capacity``, 0 without an elastic step."""
        diag = float(np.sqrt(sum(float(e) ** 2 for e in extent)))
        cells = 0
        for at, aug in enumerate(self.pipeline_):
            if aug.kind_ != "elastic":
                continue
            scale = 1.0
            for prev in self.pipeline_[:at]:
                if prev.kind_ == "linear":
                    factors = [prev.min_a_, prev.max_a_] if prev.a_values_ is None else prev.a_values_
                    scale *= max(float(np.max(np.abs(v))) for v in factors)
                elif prev.kind_ == "stdnorm":
                    raise ValueError("elastic_capacity: STDDevNormAug in front of ElasticDistortionAug rescales the cloud by its own "
                                     "statistics; size grid_capacity by hand")
                elif prev.kind_ == "elastic":
                    scale *= 1.0 + sum(abs(float(m)) for m in prev.magnitude_)   # (|blurred normal| < 1 in all but vanishing cases)
            cells = max(cells, sum((int(diag * scale / float(g)) + 4) ** 3 for g in aug.granularity_))
        return cells * int(n_batches)

    def augment_batch(self, pts, batch_ids, n_batches: int, extra_tensors: Sequence = (), n_valid=None, seed: Optional[int] = None,
                      seed_tensor=None, draws=None, grid_capacity=None) -> AugmentedBatch:
        """Augment every element of a batch on its own.  ``pts [n_rows, 3]`` float32 and ``batch_ids [n_rows]`` int32 (sorted)
        on the GPU, ``n_valid`` the device word of a padded cloud; ``draws [steps, n_batches, AUG_DRAWS]`` uniform numbers
        (``torch.rand`` on the device when None); ``seed`` (drawn when None) plus the device word ``seed_tensor`` key the hashed
        numbers of ``NoiseAug`` and ``DropAug``, so a captured call draws fresh ones when the word changes between replays.
        No host synchronisation; capturable.  ``grid_capacity``: the cells of the noise grids of ONE ``ElasticDistortionAug``
        step over the whole batch (all elements, all octaves; 16 bytes each); required when the pipeline holds that step, not
        looked at otherwise.  Elements that do not fit stay as they are and set bit 0 of ``overflow_``."""
        dev, n = _cloud(pts, batch_ids, "augment_batch")
        steps = len(self.pipeline_)
        if any(a.kind_ == "elastic" for a in self.pipeline_) and (grid_capacity is None or int(grid_capacity) < 0):
            raise ValueError("augment_batch: the pipeline holds ElasticDistortionAug, which needs grid_capacity (cells of its noise grids)")
        if draws is None:
            draws = torch.rand((steps, n_batches, AUG_DRAWS), dtype=torch.float32, device=dev)
        if tuple(draws.shape) != (steps, n_batches, AUG_DRAWS):
            raise ValueError(f"draws: expected {(steps, n_batches, AUG_DRAWS)}, got {tuple(draws.shape)}")
        ops._ptr(draws, torch.float32, "draws", dev)
        seed = ops.draw_seed() if seed is None else int(seed)
        extras = list(extra_tensors)
        for e in extras:
            if not isinstance(e, torch.Tensor) or not e.is_cuda:
                raise ValueError("extra tensors: expected GPU tensors (the HIP path has no CPU fallback)")
        table, etables, idx, last = None, [None] * len(extras), None, None
        cropped, overflow = [False] * len(extras), None
        # An extra tensor follows the points' rows only through the removing steps it is flagged for (CropPtsAug.py:67-69 and
        # the like leave the others at their length), so each carries the ids and the count of ITS rows: its pending table is
        # written with those, whatever has happened to the points since.  `in_step`: it has been through every compaction.
        eids, evalid, in_step = [batch_ids] * len(extras), [n_valid] * len(extras), [True] * len(extras)

        def identity():
            # (a copy of a kept tensor: inside a captured call that is a copy node, where torch.eye would be a fill; the warm-up
            # run that precedes a capture makes the kept one)
            if (dev, n_batches) not in self._identity:
                self._identity[(dev, n_batches)] = torch.eye(4, 3, dtype=torch.float32, device=dev).reshape(1, 12).repeat(n_batches, 1)
            return self._identity[(dev, n_batches)].clone()

        def write_points(noise=None, step=0):
            nonlocal pts, table, last
            if table is not None or noise is not None:
                pts = aug_apply(pts, batch_ids, n_batches, table, False, noise, seed, seed_tensor, step, None, n_valid)
                last, table = (table if table is not None else last), None

        def write_extra(i):
            if etables[i] is not None:
                extras[i] = aug_apply(extras[i], eids[i], n_batches, etables[i], False, None, 0, None, 0, None, evalid[i])
                etables[i] = None

        def rows_of_the_points(i, aug):
            # (the reference indexes the extra with the points' mask: a tensor of another length raises there too)
            if not in_step[i]:
                raise ValueError(f"{type(aug).__name__}: extra tensor {i} was left out of an earlier removing step, its rows are "
                                 "no longer the points' rows and the points' mask does not apply to it")

        for step, aug in enumerate(self.pipeline_):
            flags = list(aug.apply_extra_tensors_) + [False] * len(extras)
            touched = [i for i in range(len(extras)) if flags[i]]
            if aug.kind_ in _AFFINE:
                counts, stats = aug_stats(pts, batch_ids, n_batches, table, n_valid) if aug.kind_ in _NEEDS_STATS else (None, None)
                consts = aug._consts()
                table = aug_affine_step(aug.kind_, consts, aug.prob_, draws[step], identity() if table is None else table, counts, stats)
                for i in touched:
                    if extras[i].dim() != 2 or extras[i].shape[1] != 3 or extras[i].shape[0] != eids[i].shape[0]:
                        raise ValueError(f"{type(aug).__name__}: extra tensor {i} must be [n_rows, 3] to take an affine step")
                    etables[i] = aug_affine_step(aug.kind_, consts, aug.prob_, draws[step], identity() if etables[i] is None else etables[i],
                                                 counts, stats)
            elif aug.kind_ == "noise":
                write_points((draws[step], aug.prob_, aug.stddev_, aug.clip_), step)
                for i in touched:   # the points' clipped noise times sigma once more: the same words, so the points' rows
                    rows_of_the_points(i, aug)
                    if extras[i].dim() != 2 or extras[i].shape[1] != 3:
                        raise ValueError(f"NoiseAug: extra tensor {i} must be [n_rows, 3], the shape of the points' noise")
                    extras[i] = aug_apply(extras[i], batch_ids, n_batches, etables[i], False,
                                          (draws[step], aug.prob_, aug.stddev_, aug.clip_, aug.stddev_), seed, seed_tensor, step, None, n_valid)
                    etables[i] = None
            elif aug.kind_ == "elastic":   # (the extra tensors stay as they are, whatever their flags)
                write_points()
                counts, stats = aug_stats(pts, batch_ids, n_batches, None, n_valid)
                gtab, word, ws = aug_elastic_plan(counts, stats, draws[step], aug.prob_, aug.granularity_, grid_capacity)
                grid = aug_elastic_grids(gtab, ws, grid_capacity, seed, seed_tensor, step)
                pts = aug_elastic_displace(pts, batch_ids, n_batches, stats, gtab, aug.magnitude_, grid, n_valid)
                overflow = word if overflow is None else torch.bitwise_or(overflow, word)
            else:
                write_points()
                stats = aug_stats(pts, batch_ids, n_batches, None, n_valid)[1] if aug.kind_ == "crop_box" else None
                mask = aug_keep_mask(aug.kind_, aug._consts(), aug.prob_, pts, batch_ids, n_batches, draws[step], stats, seed,
                                     seed_tensor, step, n_valid)
                for i in touched:
                    rows_of_the_points(i, aug)
                    write_extra(i)
                if aug.kind_ == "drop" and aug.keep_zeros_:
                    pts = aug_apply(pts, batch_ids, n_batches, None, False, None, 0, None, 0, mask, n_valid)
                    for i in touched:
                        if extras[i].dim() != 2 or extras[i].shape[1] != 3:
                            raise ValueError(f"DropAug(p_keep_zeros=True): extra tensor {i} must be [n_rows, 3]")
                        extras[i] = aug_apply(extras[i], batch_ids, n_batches, None, False, None, 0, None, 0, mask, n_valid)
                else:
                    sel, n_out, _, orig = aug_compact(mask, batch_ids, n_batches, n_valid, idx)
                    idx = sel if orig is None else orig
                    pts, batch_ids, n_valid = ops.rows_gather_padded(pts, sel), ops.rows_gather_padded(batch_ids, sel), n_out
                    for i in range(len(extras)):
                        if i in touched:
                            extras[i], cropped[i], eids[i], evalid[i] = ops.rows_gather_padded(extras[i], sel), True, batch_ids, n_valid
                        else:
                            in_step[i] = False
        write_points()
        for i in range(len(extras)):
            write_extra(i)
        return AugmentedBatch(pts, batch_ids, n_valid, idx, extras, last, cropped, evalid, overflow)

    def augment(self, p_tensor, p_extra_tensors=[]):
        """The reference's signature for ONE cloud: a batch of one, trimmed tensors back, ``(aug_tensor, params, extras)`` with
        an empty parameter list (the draws stay on the device).  When the pipeline removes points this reads the surviving
        count back (and the count of an extra tensor that was left out of a later removing step): the one host synchronisation
        of this module.  A pipeline that holds ``ElasticDistortionAug`` has one more: the cloud's box is read back once, in
        front of everything, to size the grid (``elastic_capacity``)."""
        if not isinstance(p_tensor, torch.Tensor) or not p_tensor.is_cuda:
            raise ValueError("augment: expected a GPU tensor (the HIP path has no CPU fallback)")
        pts = ops._as(p_tensor, torch.float32)
        ids = torch.zeros(pts.shape[0], dtype=torch.int32, device=pts.device)
        cap = None
        if any(a.kind_ == "elastic" for a in self.pipeline_) and pts.shape[0] > 0:
            cap = self.elastic_capacity((pts.amax(0) - pts.amin(0)).cpu().tolist())
        elif any(a.kind_ == "elastic" for a in self.pipeline_):
            cap = 0
        res = self.augment_batch(pts, ids, 1, [e.contiguous() for e in p_extra_tensors], grid_capacity=cap)
        if res.n_valid_ is None:
            return res.pts_, [], res.extra_tensors_
        counts = {}   # one read-back per distinct word: an extra tensor left out of a later crop keeps its own, longer count

        def rows(word):
            return counts.setdefault(id(word), int(word.item()))

        return res.pts_[:rows(res.n_valid_)], [], [e if w is None else e[:rows(w)] for e, w in zip(res.extra_tensors_, res.extra_n_valid_)]
