"""se3conv3d_amd -- MI355X (gfx950) implementation of the PNEConvLayerRotEquiv hot path.

Layout mirrors the slice of ``point_cloud_lib`` that the path touches:

  se3conv3d_amd.layers   PNEConvLayerRotEquiv(+Factory), PNEConvLayer(+Factory), MultiHeadAttLayer(+Factory), LoRAttConvLayer(+Factory),
                         IConvLayer(+Factory), PreProcessModule
  se3conv3d_amd.blocks   ResNetFormer, ResNetB, ResConvNeXt, SkipConnection, DropPathPC, BatchNormPC, GroupNormPC (torch glue
                         around the conv)
  se3conv3d_amd.pc       Pointcloud(RotEquiv), BQNeighborhood, PointHierarchy(RotEquiv), frame sampling
  se3conv3d_amd.ops      FeatBasisProj, BallQuery, ComputeKeys, SE3ConvFunction, SegLoss, LinearPNE, KPPNE, PneEmbed, NeighConvMax,
                         BasisAttention, FusedBasisAttention (ctypes -> C ABI)
  se3conv3d_amd.metrics  SemSegMetrics: the reference's counters, kept on the device (include/se3conv_seg_head.h)
  se3conv3d_amd.augment  AugPipeline and the reference's augmentation classes on a whole batch (include/se3conv_augment.h)
  se3conv3d_amd.optim    AdamW with clipping, accumulation gate and schedule table in one capturable call, clip_grad_norm,
                         one_cycle_table (include/se3conv_optim.h)
  se3conv3d_amd.csrc     HIP kernels + the extern "C" boundary (include/se3conv.h)

Importing the package does not load the HIP library; the first op call does and raises if it has
not been built (``python -m se3conv3d_amd.build``).
"""
from . import augment, blocks, layers, metrics, ops, optim, pc  # noqa: F401
from .augment import AugmentedBatch, AugPipeline, Augmentation  # noqa: F401
from .blocks import BatchNormPC, DropPathPC, GroupNormPC, ResConvNeXt, ResNetB, ResNetFormer, SkipConnection  # noqa: F401
from .layers import (IConvLayer, IConvLayerFactory, LoRAttConvLayer, LoRAttConvLayerFactory, MultiHeadAttLayer,  # noqa: F401
                     MultiHeadAttLayerFactory, PNEConvLayer, PNEConvLayerFactory,
                     PNEConvLayerRotEquiv, PNEConvLayerRotEquivFactory, PreProcessModule, create_pts_icosphere)
from .metrics import SemSegMetrics  # noqa: F401
from .ops import (KPPNE, BallQuery, BasisAttention, ComputeKeys, FeatBasisProj, FusedBasisAttention, KNNQuery, LinearPNE, NeighConvMax, PneEmbed,  # noqa: F401
                  SE3ConvFunction, SegLoss, get_precision, seg_loss, set_precision)
from .optim import AdamW, ParamTables, clip_grad_norm, one_cycle_table  # noqa: F401
from .pc import (BQNeighborhood, KnnNeighborhood, Pointcloud, PointcloudRotEquiv, PointHierarchy,  # noqa: F401
                 PointHierarchyRotEquiv)

__version__ = "0.1.0"
