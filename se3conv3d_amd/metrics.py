"""``SemSegMetrics`` of the reference (point_cloud_lib/metrics/SemSegMetrics.py) with its counters on the device.

The reference's class takes numpy arrays: a training loop copies the ``[N, classes]`` logits to the host and synchronises on
every step to feed it.  This one carries the same surface and keeps, besides the host accumulators, a ``[3, classes]`` int64
device tensor ``tallies_`` (ground truth, predicted, hit) that the library's loss pass adds to (include/se3conv_seg_head.h):

  * ``update_metrics`` with numpy arrays is the reference's host arithmetic, on rows the caller has compacted;
  * ``update_metrics`` with device tensors runs the library pass into ``tallies_`` -- rows whose label is masked, out of range
    (``ignore_index``) or absent do not count, nothing is compacted, nothing is read back;
  * ``loss`` gives the training loss AND the counters in that one pass;
  * only the read-outs (``accum_*_`` and the six figures) synchronise.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops


class SemSegMetrics:

    def __init__(self, p_num_classes, p_mask_classes, device=None):
        self.num_classes_ = int(p_num_classes)
        self.mask_classes_ = tuple(int(c) for c in p_mask_classes)
        self.mask_ = np.array([i not in self.mask_classes_ for i in range(self.num_classes_)])
        self.tallies_: Optional[torch.Tensor] = None   # [3, classes] int64 on the device: ground truth, predicted, hit
        self.counted_: Optional[torch.Tensor] = None   # [classes] uint8 on the device: the classes that count
        self.reset()
        if device is not None:
            self._on(torch.device(device))

    def _on(self, device) -> None:
        if self.tallies_ is None:
            self.tallies_ = torch.zeros((3, self.num_classes_), dtype=torch.int64, device=device)
            self.counted_ = torch.from_numpy(self.mask_.astype(np.uint8)).to(device)
        elif self.tallies_.device != device:
            raise ValueError(f"SemSegMetrics: counters live on {self.tallies_.device}, got tensors on {device}")

    def reset(self):
        self.host_intersection_ = np.zeros(self.num_classes_)
        self.host_union_ = np.zeros(self.num_classes_)
        self.host_gt_ = np.zeros(self.num_classes_)
        if self.tallies_ is not None:
            self.tallies_.zero_()

    # ----------------------------------------------------------------------------------------------------- updates
    def update_metrics(self, p_predict_probs, p_labels, n_valid: Optional[torch.Tensor] = None):
        if isinstance(p_predict_probs, torch.Tensor) and p_predict_probs.is_cuda:
            with torch.no_grad():
                self.loss(p_predict_probs.detach(), p_labels, n_valid=n_valid)
            return
        if isinstance(p_predict_probs, torch.Tensor):
            p_predict_probs, p_labels = p_predict_probs.detach().numpy(), p_labels.numpy()
        pred = np.argmax(p_predict_probs, 1)
        mask_eq = pred == p_labels
        num_labels = np.bincount(p_labels, minlength=self.num_classes_).astype(np.float32)
        num_pred = np.bincount(pred, minlength=self.num_classes_).astype(np.float32)
        num_equal = np.bincount(p_labels[mask_eq], minlength=self.num_classes_).astype(np.float32)
        self.host_gt_ += num_labels
        self.host_union_ += num_labels + num_pred - num_equal
        self.host_intersection_ += num_equal

    def loss(self, logits, labels, label_smoothing: float = 0.0, n_valid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The mean smoothed cross-entropy over the rows that count (``ops.seg_loss``), whose counts are added to
        ``tallies_`` by the same pass.  No synchronisation; capturable."""
        self._on(logits.device)
        return ops.seg_loss(logits, labels, label_smoothing, self.counted_, n_valid, self.tallies_)

    # --------------------------------------------------------------------------------------------------- read-outs
    def _device_counts(self) -> np.ndarray:
        if self.tallies_ is None:
            return np.zeros((3, self.num_classes_))
        return self.tallies_.cpu().numpy().astype(np.float64)   # (the one synchronisation)

    @property
    def accum_gt_(self) -> np.ndarray:
        return self.host_gt_ + self._device_counts()[0]

    @property
    def accum_intersection_(self) -> np.ndarray:
        return self.host_intersection_ + self._device_counts()[2]

    @property
    def accum_union_(self) -> np.ndarray:
        gt, pred, hit = self._device_counts()
        return self.host_union_ + (gt + pred - hit)

    def per_class_acc(self):
        return self.accum_intersection_[self.mask_] / np.maximum(self.accum_gt_[self.mask_], 1) * 100.0

    def per_class_iou(self):
        return self.accum_intersection_[self.mask_] / np.maximum(self.accum_union_[self.mask_], 1) * 100.0

    def class_mean_acc(self):
        return np.mean(self.accum_intersection_[self.mask_] / np.maximum(self.accum_gt_[self.mask_], 1)) * 100.0

    def class_mean_iou(self):
        return np.mean(self.accum_intersection_[self.mask_] / np.maximum(self.accum_union_[self.mask_], 1)) * 100.0

    def mean_acc(self):
        return np.sum(self.accum_intersection_[self.mask_]) / np.maximum(np.sum(self.accum_gt_[self.mask_]), 1) * 100.0

    def mean_iou(self):
        return np.sum(self.accum_intersection_[self.mask_]) / np.maximum(np.sum(self.accum_union_[self.mask_]), 1) * 100.0
