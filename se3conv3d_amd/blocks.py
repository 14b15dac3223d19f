"""Block-level glue of the reference's networks around the convolution (scope row f-3): drop path with frame-aware
batch ids, the residual connection with its learned gain, the point-cloud batch norm and the ResNetFormer block, with
the reference's attribute names so that a reference ``state_dict`` loads key for key.  On GPU tensors the row-wise
passes run as the library's fused kernels (csrc/glue.hip through ops.BatchNormTrain / SkipDropPath / BiasGelu): training
batch norm in 3 launches each way, skip + layer scale + drop-path gate in one, bias + GELU behind a bias-free GEMM in
one, the linear layers' weight gradients on the library's row-split TN GEMM (timings per block:
profiles/r03_block_glue_timing.txt); the forward and input-gradient C x C products stay BLAS GEMMs.
``FUSED = False`` (or SE3_BLOCKS_FUSED=0) keeps the plain torch formulation (the A/B of tools/time_block.py).

  DropPathPC      layers/DropPathPC.py:30-46      one keep / drop decision per batch element, scaled by 1 / keep_prob
  SkipConnection  layers/SkipConnection.py        drop_path(x * gamma_) + y, gamma_ initialised to 1e-6
  BatchNormPC     layers/BatchNormPC.py:22-32     BatchNorm1d(momentum=0.2) on the feature rows (the cloud is unused)
  GroupNormPC     layers/GroupNormPC.py:13-57     per batch element and group of channels (channel c: group c % G), eps 1e-8;
                                                  ops.GroupNorm (csrc/group_norm.hip), no statistics across elements or ranks
  ResNetFormer    layers/ResNetFormer.py:33-88    norm -> conv -> skip; norm -> linear (x2) -> GELU -> linear -> skip
  ResNetB         layers/ResNetB.py:33-84         norm -> linear (/2) -> conv -> GELU -> linear -> skip
  ResConvNeXt     layers/ResConvNeXt.py:33-83     conv -> norm -> linear (x2) -> GELU -> linear -> skip

Padded clouds.  A cloud built with ``p_n_valid`` alone is refused by every module here.  One built with
``p_padded_rows=True`` (pc.py) has feature tensors padded like its points, and the modules run the library's padded passes
(include/se3conv_padded_rows.h; the same ops.BatchNormTrain / SkipDropPath / Linear, handed the cloud's row-count word and
the frame count of the rows, ``_rows_of``): statistics, ``1/N`` and channel sums over the present rows alone -- bit for bit
those of the trimmed tensors --, no absent row read (an absent row's batch id never indexes the drop-path gate), zeros
written at the absent rows.  The invariant a network gets: every library pass leaves
zeros at absent rows, the stock torch ops in between (Linear, GELU) are row-wise and keep them finite; the caller's part is
finite level-0 input features and a loss that ignores absent rows (``pc.present_mask``), so that the gradient arriving
there is zero.  There is no torch fallback on such a cloud: a configuration that would need one (non-fp32 input,
``FUSED = False``, ``drop_prob >= 1``, training without running statistics) raises ``NotImplementedError``; eval-mode batch
norm stays the row-wise torch path.  Group norm has no eval form: on such a cloud it is the kernel in either mode.
"""
import os

import torch

from . import ops
from .layers import PreProcessModule
from .pc import padded_rows, refuse_unflagged

FUSED = os.environ.get("SE3_BLOCKS_FUSED", "1") != "0"


def _num_batches(p_pc) -> int:
    """Batch count as a host integer: the clouds of this package cache it (no device read-back per call, and none
    inside a graph capture); a foreign cloud object is asked once per call like the reference does."""
    return p_pc.num_batches() if hasattr(p_pc, "num_batches") else int(p_pc.batch_size_)


def _fused(t: torch.Tensor) -> bool:
    return FUSED and t.is_cuda and t.dim() == 2 and t.dtype == torch.float32


def _need_fused_on_padded_rows(who: str, t: torch.Tensor, ok: bool = True, limit: str = "") -> None:
    """The loud end of a flagged padded cloud (``p_padded_rows``): the torch formulations read every row of the buffers."""
    if not _fused(t):
        raise NotImplementedError(f"{who} on padded feature rows (p_padded_rows) runs the library's kernels only: [rows, C] "
                                  "float32 GPU tensors with blocks.FUSED on -- the torch formulation would read absent rows")
    if not ok:
        raise NotImplementedError(f"{who} on padded feature rows (p_padded_rows): {limit} is not implemented -- it would need "
                                  "the torch formulation, which reads absent rows")


def _rows_of(p_x, p_pc):
    """``(n_valid, n_frames, row batch ids)`` of a feature tensor on a cloud, as the row-wise ops take them.  An ordinary
    cloud: no word, and rows of a cloud with frames carry the batch id of their point (batch_ids_considering_frames_).  A
    flagged padded cloud: its word, and one row per (point, frame) or one per point."""
    if not padded_rows(p_pc):
        ids = getattr(p_pc, "batch_ids_considering_frames_", None)
        return None, 1, ids if ids is not None else getattr(p_pc, "batch_ids_", None)
    n = int(p_pc.pts_.shape[0])
    f = int(getattr(p_pc, "n_frames_", 1))
    if p_x.shape[0] == n * f and f > 1:
        return p_pc.n_valid_, f, p_pc.batch_ids_considering_frames_
    if p_x.shape[0] == n:
        return p_pc.n_valid_, 1, p_pc.batch_ids_
    raise ValueError(f"{p_x.shape[0]} feature rows on a padded cloud of {n} rows with {f} frame(s)")


class DropPathPC(torch.nn.Module):
    def __init__(self, p_drop_prob):
        super().__init__()
        self.drop_prob_ = p_drop_prob

    def forward(self, p_x, p_pc):
        refuse_unflagged(p_pc, "DropPathPC")
        if self.drop_prob_ == 0.0 or not self.training:
            return p_x
        padded = padded_rows(p_pc)
        if padded:
            _need_fused_on_padded_rows("DropPathPC", p_x, self.drop_prob_ < 1.0, "drop_prob >= 1")
        n_valid, frames, ids = _rows_of(p_x, p_pc)
        # one uniform draw per batch element, keep where keep + u >= 1
        keep = 1.0 - self.drop_prob_
        u = torch.rand((_num_batches(p_pc),), dtype=p_x.dtype, device=p_x.device)
        if padded:
            # through the skip kernel's gate path (x * 1 * gate + 0): an absent row's batch id never indexes the gate
            one = torch.ones((1, p_x.shape[1]), dtype=p_x.dtype, device=p_x.device)
            return ops.SkipDropPath.apply(p_x, torch.zeros_like(p_x), one, u, ids, keep, n_valid, frames)
        return p_x.div(keep) * torch.floor(keep + u).index_select(0, ids.to(torch.int64)).reshape(-1, 1)


class SkipConnection(torch.nn.Module):
    def __init__(self, p_drop_prob, p_num_features, p_init_gamma=1e-6):
        super().__init__()
        self.drop_path_ = DropPathPC(p_drop_prob)
        self.gamma_ = torch.nn.Parameter(torch.full((1, p_num_features), float(p_init_gamma)))

    def forward(self, p_x, p_y, p_pc):
        refuse_unflagged(p_pc, "SkipConnection")
        if padded_rows(p_pc):
            _need_fused_on_padded_rows("SkipConnection", p_x, not (self.training and self.drop_path_.drop_prob_ >= 1.0),
                                       "drop_prob >= 1")
            if p_x.shape != p_y.shape:
                raise NotImplementedError("SkipConnection on padded feature rows (p_padded_rows): x and y of different shapes "
                                          "would need the torch formulation, which reads absent rows")
        # drop_prob >= 1 (keep <= 0): the reference divides by zero (DropPathPC.py:45) -- the plain formulation reproduces
        # that instead of handing the kernel keep = 0, which it reads as "the gate is the factor itself"
        elif not _fused(p_x) or p_x.shape != p_y.shape or (self.training and self.drop_path_.drop_prob_ >= 1.0):
            return self.drop_path_(p_x * self.gamma_, p_pc) + p_y
        n_valid, frames, ids = _rows_of(p_x, p_pc)
        gate, keep = None, 0.0
        if self.drop_path_.drop_prob_ != 0.0 and self.training:
            keep = 1.0 - self.drop_path_.drop_prob_
            # the same draw as DropPathPC (one uniform per batch element); floor(keep + u) / keep is evaluated in the kernel
            gate = torch.rand((_num_batches(p_pc),), dtype=p_x.dtype, device=p_x.device)
        return ops.SkipDropPath.apply(p_x, p_y, self.gamma_, gate, ids if gate is not None else None, keep, n_valid, frames)


class NormLayerPC(torch.nn.Module):
    def __init__(self, p_num_features):
        super().__init__()
        self.num_feats_ = p_num_features


class BatchNormPC(NormLayerPC):
    def __init__(self, p_num_features):
        super().__init__(p_num_features)
        self.layer_ = torch.nn.BatchNorm1d(p_num_features, momentum=0.2)

    def forward(self, p_x, p_pc):
        refuse_unflagged(p_pc, "BatchNormPC (its statistics need the present-row count)")
        bn = self.layer_
        kernel_form = bn.training and bn.track_running_stats and bn.momentum is not None
        if padded_rows(p_pc) and (bn.training or not bn.track_running_stats):  # (batch statistics; eval mode is row-wise)
            _need_fused_on_padded_rows("BatchNormPC", p_x, kernel_form, "training without running statistics (or with momentum None)")
        elif not (_fused(p_x) and kernel_form):
            return bn(p_x)
        n_valid, frames, _ = _rows_of(p_x, p_pc)
        return ops.BatchNormTrain.apply(p_x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                        bn.num_batches_tracked, n_valid, frames)


class GroupNormPC(NormLayerPC):
    """The reference's group norm: the statistics of a batch element come from its own rows, one mean and one (biased)
    variance per group of channels, where the group of channel ``c`` is ``c % num_groups_`` -- the reference reshapes its rows
    to ``(-1, num_groups_)``, so a group's channels are strided.  Rows of a cloud with frames take their point's element (the
    reference never ran it with frames; the extension DropPathPC makes).  There is no running state and no eval form."""

    EPS = 1e-8  # layers/GroupNormPC.py:41

    def __init__(self, p_num_features, p_num_groups=8):
        super().__init__(p_num_features)
        if p_num_features % p_num_groups:
            raise ValueError(f"GroupNormPC: {p_num_features} features are not a multiple of {p_num_groups} groups")
        self.num_groups_ = p_num_groups
        self.gamma_ = torch.nn.Parameter(torch.ones(1, p_num_features))
        self.betas_ = torch.nn.Parameter(torch.zeros(1, p_num_features))

    def forward(self, p_x, p_pc):
        refuse_unflagged(p_pc, "GroupNormPC (its statistics need the present-row count)")
        n = int(p_pc.batch_ids_.shape[0])
        if p_x.shape[0] % max(n, 1) or (n == 0 and p_x.shape[0]):
            raise ValueError(f"GroupNormPC: {p_x.shape[0]} feature rows on a cloud of {n} points")
        frames = max(p_x.shape[0] // max(n, 1), 1)
        if padded_rows(p_pc):
            _need_fused_on_padded_rows("GroupNormPC", p_x)
        elif not _fused(p_x):
            return self._torch_form(p_x, p_pc.batch_ids_, _num_batches(p_pc), frames)
        return ops.GroupNorm.apply(p_x, self.gamma_, self.betas_, p_pc.batch_ids_, _num_batches(p_pc), self.num_groups_,
                                   self.EPS, getattr(p_pc, "n_valid_", None) if padded_rows(p_pc) else None, frames)

    def _torch_form(self, p_x, p_batch_ids, p_num_batches, p_frames):
        """layers/GroupNormPC.py:41-57 with index_add_ in place of scatter_mean: mean, then the mean of the squared
        differences, both per (element, group)."""
        groups = self.num_groups_
        ids = p_batch_ids.to(torch.int64).repeat_interleave(p_frames) if p_frames > 1 else p_batch_ids.to(torch.int64)
        x = p_x.reshape(p_x.shape[0], -1, groups)                       # [rows, C / G, G]: channel c = k * G + j
        size = torch.zeros(p_num_batches, dtype=p_x.dtype, device=p_x.device).index_add_(
            0, ids, torch.full((ids.shape[0],), float(x.shape[1]), dtype=p_x.dtype, device=p_x.device)).clamp_(min=1.0)

        def mean_of(v):
            return torch.zeros((p_num_batches, groups), dtype=v.dtype, device=v.device).index_add_(0, ids, v.sum(1)) / size[:, None]

        diff = x - mean_of(x).index_select(0, ids)[:, None, :]
        var = mean_of(diff * diff).index_select(0, ids)[:, None, :]
        return (diff / torch.sqrt(var + self.EPS)).reshape(p_x.shape) * self.gamma_ + self.betas_


class Block(PreProcessModule):
    def __init__(self, p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob):
        super().__init__()
        self.feat_input_size_ = p_in_features
        self.feat_output_size_ = p_out_features


class ResNetFormer(Block):
    """Same-level residual block: the convolution keeps the width, the point-wise MLP widens by 2 and maps to the
    output width; a linear skip appears only when the widths differ."""

    def __init__(self, p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob):
        super().__init__(p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob)
        c_in, c_out = self.feat_input_size_, self.feat_output_size_
        self.act_func_ = torch.nn.GELU()
        self.feat_scale_factor_ = 2
        self.spatial_conv_ = p_conv_fact.create_conv_layer(c_in, c_in)
        self.norm_1_ = p_norm_layer(c_in)
        self.norm_2_ = p_norm_layer(c_in)
        self.linear_1_ = torch.nn.Linear(c_in, c_in * self.feat_scale_factor_)
        self.linear_2_ = torch.nn.Linear(c_in * self.feat_scale_factor_, c_out)
        self.skip_path_1_ = SkipConnection(p_path_drop_prob, c_in)
        self.skip_path_2_ = SkipConnection(p_path_drop_prob, c_out)
        if c_in != c_out:
            self.skip_conv_ = torch.nn.Linear(c_in, c_out)

    def forward(self, p_pc_in, p_in_features, p_neighborhood):
        refuse_unflagged(p_pc_in, "ResNetFormer")
        padded = padded_rows(p_pc_in)
        n_valid = frames = None
        if padded:
            # the bias gradients of the linear layers are then summed by the library over the present rows (no memset node
            # in a captured step); on an ordinary cloud they stay torch's column sum
            _need_fused_on_padded_rows("ResNetFormer", p_in_features)
            n_valid, frames, _ = _rows_of(p_in_features, p_pc_in)
        x = self.spatial_conv_(p_pc_in=p_pc_in, p_pc_out=p_pc_in, p_in_features=self.norm_1_(p_in_features, p_pc_in),
                               p_neighborhood=p_neighborhood)
        x = self.skip_path_1_(x, p_in_features, p_pc_in)
        h = self.norm_2_(x, p_pc_in)
        if padded or _fused(h):
            # bias + GELU in one pass behind a bias-free GEMM; the linear layers' weight gradients on the row-split GEMM
            h = ops.BiasGelu.apply(ops.Linear.apply(h, self.linear_1_.weight, None), self.linear_1_.bias)
            y = ops.Linear.apply(h, self.linear_2_.weight, self.linear_2_.bias, n_valid, frames)
            skip = x
            if self.feat_input_size_ != self.feat_output_size_:
                skip = ops.Linear.apply(x, self.skip_conv_.weight, self.skip_conv_.bias, n_valid, frames)
        else:
            h = self.act_func_(self.linear_1_(h))
            y = self.linear_2_(h)
            skip = self.skip_conv_(x) if self.feat_input_size_ != self.feat_output_size_ else x
        return self.skip_path_2_(y, skip, p_pc_in)


class _OneNormBlock(Block):
    """What ResNetB and ResConvNeXt share: one norm, two linear layers, one skip connection with a linear skip where the widths
    differ, and the way their dense layers run -- ``ops.Linear`` on fused rows (the weight gradient on the library's row-split
    GEMM; on a flagged padded cloud the bias gradient over the present rows alone), ``torch.nn.Linear`` otherwise.  The
    linear skip reads the block's input itself: on a padded cloud that input is finite at absent rows (zeros, behind any
    library pass), the invariant of the module docstring."""

    def _rows(self, p_pc_in, p_in_features, p_who):
        """``(fused, n_valid, frames)`` of this call."""
        refuse_unflagged(p_pc_in, p_who)
        if padded_rows(p_pc_in):
            _need_fused_on_padded_rows(p_who, p_in_features)
            n_valid, frames, _ = _rows_of(p_in_features, p_pc_in)
            return True, n_valid, frames
        return _fused(p_in_features), None, None

    @staticmethod
    def _linear(p_layer, p_x, p_fused, p_n_valid, p_frames):
        if p_fused:
            return ops.Linear.apply(p_x, p_layer.weight, p_layer.bias, p_n_valid, p_frames)
        return p_layer(p_x)

    def _skip(self, p_in_features, p_fused, p_n_valid, p_frames):
        if self.feat_input_size_ != self.feat_output_size_:
            return self._linear(self.skip_conv_, p_in_features, p_fused, p_n_valid, p_frames)
        return p_in_features


class ResNetB(_OneNormBlock):
    """Bottleneck block: the norm, a linear layer to half the width, the convolution at that width, GELU, a linear layer to the
    output width, and the skip connection."""

    def __init__(self, p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob):
        super().__init__(p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob)
        c_in, c_out = self.feat_input_size_, self.feat_output_size_
        self.act_func_ = torch.nn.GELU()
        self.feat_scale_factor_ = 2
        self.spatial_conv_ = p_conv_fact.create_conv_layer(c_in // self.feat_scale_factor_, c_in // self.feat_scale_factor_)
        self.norm_ = p_norm_layer(c_in)
        self.linear_1_ = torch.nn.Linear(c_in, c_in // self.feat_scale_factor_)
        self.linear_2_ = torch.nn.Linear(c_in // self.feat_scale_factor_, c_out)
        self.skip_path_ = SkipConnection(p_path_drop_prob, c_out)
        if c_in != c_out:
            self.skip_conv_ = torch.nn.Linear(c_in, c_out)

    def forward(self, p_pc_in, p_in_features, p_neighborhood):
        fused, n_valid, frames = self._rows(p_pc_in, p_in_features, "ResNetB")
        x = self._linear(self.linear_1_, self.norm_(p_in_features, p_pc_in), fused, n_valid, frames)
        x = self.spatial_conv_(p_pc_in=p_pc_in, p_pc_out=p_pc_in, p_in_features=x, p_neighborhood=p_neighborhood)
        x = self._linear(self.linear_2_, self.act_func_(x), fused, n_valid, frames)   # (the GELU follows the convolution)
        return self.skip_path_(x, self._skip(p_in_features, fused, n_valid, frames), p_pc_in)


class ResConvNeXt(_OneNormBlock):
    """ConvNeXt-style block: the convolution first, then the norm and the point-wise MLP (twice the width, GELU, the output
    width), and the skip connection."""

    def __init__(self, p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob):
        super().__init__(p_in_features, p_out_features, p_conv_fact, p_norm_layer, p_path_drop_prob)
        c_in, c_out = self.feat_input_size_, self.feat_output_size_
        self.act_func_ = torch.nn.GELU()
        self.feat_scale_factor_ = 2
        self.spatial_conv_ = p_conv_fact.create_conv_layer(c_in, c_in)
        self.norm_ = p_norm_layer(c_in)
        self.linear_1_ = torch.nn.Linear(c_in, c_in * self.feat_scale_factor_)
        self.linear_2_ = torch.nn.Linear(c_in * self.feat_scale_factor_, c_out)
        self.skip_path_ = SkipConnection(p_path_drop_prob, c_out)
        if c_in != c_out:
            self.skip_conv_ = torch.nn.Linear(c_in, c_out)

    def forward(self, p_pc_in, p_in_features, p_neighborhood):
        fused, n_valid, frames = self._rows(p_pc_in, p_in_features, "ResConvNeXt")
        x = self.spatial_conv_(p_pc_in=p_pc_in, p_pc_out=p_pc_in, p_in_features=p_in_features, p_neighborhood=p_neighborhood)
        x = self.norm_(x, p_pc_in)
        if fused:
            # bias + GELU in one pass behind a bias-free GEMM, as in ResNetFormer
            x = ops.BiasGelu.apply(ops.Linear.apply(x, self.linear_1_.weight, None), self.linear_1_.bias)
        else:
            x = self.act_func_(self.linear_1_(x))
        x = self._linear(self.linear_2_, x, fused, n_valid, frames)
        return self.skip_path_(x, self._skip(p_in_features, fused, n_valid, frames), p_pc_in)
