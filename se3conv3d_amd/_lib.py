"""ctypes binding of libse3conv_hip.so (C ABI declared in include/se3conv.h).

There is no CPU fallback: if the library is missing or a call fails the caller gets an exception.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", f"libse3conv_hip{os.environ.get('SE3_LIB_SUFFIX', '')}.so")  # suffix: variant builds, see build.py

SE3_OK = 0
ABI_VERSION = 6  # SE3_ABI_VERSION of include/se3conv.h these signatures were written against
PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16x3_t16": 2}
REL_ROT = {"6D": (0, 9), "matrix": (1, 12), "quaternion": (2, 7)}  # p_rel_rot -> (SE3_REL_ROT_*, descriptor dims)


class Se3Shape(C.Structure):
    """struct se3conv_shape (include/se3conv.h)."""

    _fields_ = [
        ("n_in", C.c_int64), ("n_out", C.c_int64), ("n_edges", C.c_int64),
        ("f_in", C.c_int32), ("f_out", C.c_int32), ("c_in", C.c_int32), ("c_out", C.c_int32),
        ("num_basis", C.c_int32), ("precision", C.c_int32),
    ]


class Se3Prepared(C.Structure):
    """struct se3conv_prepared (include/se3conv.h): operands kept by the caller across calls."""

    _fields_ = [("geom_in", C.c_void_p), ("geom_out", C.c_void_p), ("feat_words", C.c_void_p),
                ("geom_in_valid", C.c_int32), ("geom_out_valid", C.c_int32), ("feat_words_valid", C.c_int32)]


class Se3Level(C.Structure):
    """struct se3_level (include/se3conv_levels.h): one level of a ``se3_grid_levels`` chain."""

    _fields_ = [("cell_size", C.c_float), ("capacity", C.c_int64),
                ("cell_ids", C.c_void_p), ("sorted_ids", C.c_void_p), ("cell_ends", C.c_void_p),
                ("pts", C.c_void_p), ("batch_ids", C.c_void_p),
                ("u", C.c_void_p), ("ids", C.c_void_p), ("picked", C.c_void_p)]


class Se3LibraryError(RuntimeError):
    pass


_P = C.c_void_p
_I64 = C.c_int64
_I32 = C.c_int32
_SZ = C.c_size_t
_F = C.c_float
_SHP = C.POINTER(Se3Shape)

# name -> (restype, argtypes), one table per header of include/ (see TABLES below)
SIGNATURES = {
    "se3_abi_version": (C.c_int, []),
    "se3_error_string": (C.c_char_p, [C.c_int]),
    "se3conv_intermediate_bytes_per_element": (C.c_int, [_SHP, C.c_int]),
    "se3conv_intermediate_row_bytes": (C.c_int64, [_SHP, C.c_int]),
    "se3_compute_keys": (C.c_int, [_P, _P, _P, _P, _P, _I64, _P, _P]),
    "se3_batch_aabb": (C.c_int, [_P, _P, _I64, _I32, _P, _P, _P]),
    "se3_grid_subsample_workspace_bytes": (_SZ, [_I64, _I32]),
    "se3_grid_subsample": (C.c_int, [_P, _P, _I64, _I32, _F, _P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    "se3_segment_pool": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "se3_segment_unpool": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I32, _P, _P]),
    "se3_frame_pool": (C.c_int, [_P, _I64, _I32, _I32, _I32, _P, _P, _P]),
    "se3_frame_unpool": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _P, _P]),
    "se3_ball_query_grid": (C.c_int, [_P, _P, _I64, _I32, _F, _P, _P, _P, _P]),
    "se3_ball_query_grid_from_box": (C.c_int, [_P, _P, _I32, _F, _P, _P, _P]),
    "se3_ball_query_needs_grid": (C.c_int, [_I64]),
    "se3_ball_query_workspace_bytes": (_SZ, [_I64, _I64]),
    "se3_ball_query_count": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I64, _I64, _P, _SZ, _P, _P]),
    "se3_ball_query_store": (C.c_int, [_P, _P, _F, _I64, _I64, _P, _SZ, _P, _I64, _P, _P]),
    "se3_ball_query_bounded": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I64, _I64, _I32, _P, _SZ, _I64, _P, _P, _P, _P, _P]),
    "se3_ball_query_grid_bytes": (_SZ, [_I64]),
    "se3_ball_query_bounded_shared": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I64, _I64, _I32, _P, _SZ, _I32, _P, _SZ, _I64, _P,
                                                _P, _P, _P, _P]),
    "se3_csr_transpose_workspace_bytes": (_SZ, [_I64]),
    "se3_csr_transpose": (C.c_int, [_P, _I64, _I64, _P, _SZ, _P, _P, _P, _P]),
    "se3_csr_transpose_bounded": (C.c_int, [_P, _I64, _P, _I64, _P, _SZ, _P, _P, _P, _P]),
    "se3_rot_tensors": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _SHP, _P, _P, _P, _P]),
    "se3_rot_tensors_rel": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _SHP, _I32, _P, _P, _P, _P]),
    "se3_feat_basis_proj": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I32, _I32, _P, _P]),
    "se3_feat_basis_proj_grad": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I32, _I32, _P, _P, _P]),
    "se3conv_fwd_workspace_bytes": (_SZ, [_SHP, C.c_int]),
    "se3conv_fwd": (C.c_int, [_P] * 12 + [_SHP, _P, _P, _P, _SZ, _P]),
    "se3conv_bwd_workspace_bytes": (_SZ, [_SHP, C.c_int, C.c_int, C.c_int]),
    "se3conv_bwd_needs_t": (C.c_int, [_SHP, C.c_int]),
    "se3conv_bwd": (C.c_int, [_P] * 17 + [_SHP, _P, _P, _P, _P, _P, _SZ, _P]),
    "se3conv_fwd_prepared": (C.c_int, [_P] * 12 + [_SHP, _P, _P, _P, _SZ, _P, C.POINTER(Se3Prepared)]),
    "se3conv_bwd_prepared": (C.c_int, [_P] * 17 + [_SHP, _P, _P, _P, _P, _P, _SZ, _P, C.POINTER(Se3Prepared)]),
    "se3_knn_query": (C.c_int, [_P, _P, _I64, _I32, _P, _P]),
    "se3_knn_query_pair": (C.c_int, [_P, _P, _I64, _P, _P, _I64, _I32, _P, _P]),
    "se3_grid_pick": (C.c_int, [_P, _P, _P, _I64, _P, _P, _P]),
    "se3_rows_gather": (C.c_int, [_P, _P, _I64, _I64, _P, _P]),
    "se3_rows_scatter": (C.c_int, [_P, _P, _I64, _I64, _P, _P]),
    "se3_knn_query_grid_workspace_bytes": (C.c_size_t, [_I64]),
    "se3_knn_grid_params": (C.c_int, [_P, _I64, _P, _P, _I32, _I32, C.c_float, _P, _P, _P, _P]),
    "se3_knn_query_grid": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _P, _P, C.c_size_t, _P]),
    "se3_pca_frames": (C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P]),
    "se3_shuffle_frames": (C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P]),
    "se3_glue_workspace_bytes": (_SZ, [_I32]),
    "se3_bn_fwd": (C.c_int, [_P, _P, _P, _I64, _I32, _F, _F, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "se3_affine_act": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I32, _P, _P]),
    "se3_bn_bwd": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P, _SZ, _P]),
    "se3_skip_fwd": (C.c_int, [_P, _P, _P, _P, _F, _P, _I64, _I32, _P, _P]),
    "se3_skip_bwd": (C.c_int, [_P, _P, _P, _P, _F, _P, _I64, _I32, _P, _P, _P, _SZ, _P]),
    "se3_bias_gelu_bwd": (C.c_int, [_P, _P, _P, _I64, _I32, _P, _P, _P, _SZ, _P]),
    "se3_linear_wgrad_workspace_bytes": (_SZ, [_I64, _I32, _I32]),
    "se3_linear_wgrad": (C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _SZ, _P]),
    "se3_profile_enable": (C.c_int, [C.c_int]),
    "se3_profile_reset": (C.c_int, []),
    "se3_profile_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "se3_profile_tags": (C.c_int, [C.c_char_p, _SZ]),
}

# the capped ball query
CAPPED_SIGNATURES = {
    "se3_ball_query_capped_workspace_bytes": (_SZ, [_I64, _I64]),
    "se3_ball_query_capped": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I64, _I64, _I32, _P, _SZ, _I32, _P, _SZ, _I64, _P, _P, _P, _P,
                                        _P, _I32, C.c_uint32, _P, _P]),
}

# the chain of grid sub-sampling levels with device-side sizes
_LVL = C.POINTER(Se3Level)
LEVEL_SIGNATURES = {
    "se3_grid_levels_workspace_bytes": (_SZ, [_I64, _I32, _LVL, _I32]),
    "se3_grid_levels": (C.c_int, [_P, _P, _I64, _P, _I32, _LVL, _I32, _P, _P, _SZ, _P]),
}

# the host-only query of the kernel forms a call takes
FORMS_SIGNATURES = {
    "se3conv_forms": (C.c_int, [_SHP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _SZ]),
}

# the geometry builds on padded clouds -- row counts in device words
PADDED_SIGNATURES = {
    "se3_batch_aabb_padded": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _P, _P]),
    "se3_ball_query_padded_workspace_bytes": (_SZ, [_I64, _I64]),
    "se3_ball_query_padded": (C.c_int, [_P, _P, _P, _P, _P, _P, _F, _I64, _I64, _P, _P, _I32, _P, _SZ, _I32, _P, _SZ, _I64, _P,
                                        _P, _P, _P, _P]),
    "se3_knn_grid_params_padded": (C.c_int, [_P, _I64, _P, _P, _P, _I32, _I32, _F, _P, _P, _P, _P]),
    "se3_knn_query_padded_workspace_bytes": (_SZ, [_I64, _I32]),
    "se3_knn_query_padded": (C.c_int, [_P, _P, _I64, _P, _P, _P, _P, _I32, _P, _P, _SZ, _P]),
    "se3_pca_frames_padded": (C.c_int, [_P, _P, _I64, _P, _I32, _I32, _P, _P]),
}

# the row-wise passes of a network on padded clouds -- feature tensors padded like the points, the present-row count a device word
PADDED_ROWS_SIGNATURES = {
    "se3_bn_fwd_padded": (C.c_int, [_P, _P, _P, _I64, _I32, _P, _I32, _F, _F, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "se3_bn_bwd_padded": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I32, _P, _I32, _P, _P, _P, _P, _SZ, _P]),
    "se3_skip_fwd_padded": (C.c_int, [_P, _P, _P, _P, _F, _P, _I64, _I32, _P, _I32, _P, _P]),
    "se3_skip_bwd_padded": (C.c_int, [_P, _P, _P, _P, _F, _P, _I64, _I32, _P, _I32, _P, _P, _P, _SZ, _P]),
    "se3_channel_sums_padded": (C.c_int, [_P, _I64, _I32, _P, _I32, _P, _P, _SZ, _P]),
    "se3_frame_pool_padded": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _P, _P, _P]),
    "se3_frame_unpool_padded": (C.c_int, [_P, _P, _I64, _I32, _P, _I32, _I32, _P, _P]),
    "se3_segment_unpool_padded": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I32, _P, _P]),
    "se3_rows_gather_padded": (C.c_int, [_P, _P, _I64, _I64, _P, _P]),
    "se3_rows_unpick_padded": (C.c_int, [_P, _P, _P, _I64, _I64, _P, _P]),
}

# farthest-point sampling
FPS_SIGNATURES = {
    "se3_fps_workspace_bytes": (_SZ, [_I64, _I32]),
    "se3_fps": (C.c_int, [_P, _P, _I64, _P, _I32, _F, _P, _I64, _P, _P, _P, _P, _P, _SZ, _P]),
}
FPS_RESIDENT_MAX = 8192  # SE3_FPS_RESIDENT_MAX: the largest element the register-resident form of the sampling kernel takes

# header under include/ -> its table, in the order the headers were added.  The rule, for every entry: the table lists exactly
# the symbols its header declares, with the header's argument counts, and no name stands in two tables.  Headers after
# se3conv.h are additions inside ABI version 6: they extend the surface, the earlier headers and tables stay as they are.
TABLES = {
    "se3conv.h": SIGNATURES,
    "se3conv_capped.h": CAPPED_SIGNATURES,
    "se3conv_levels.h": LEVEL_SIGNATURES,
    "se3conv_forms.h": FORMS_SIGNATURES,
    "se3conv_padded.h": PADDED_SIGNATURES,
    "se3conv_padded_rows.h": PADDED_ROWS_SIGNATURES,
    "se3conv_fps.h": FPS_SIGNATURES,
}

# capacity-bounded k-NN neighbourhoods: the pair query between padded clouds and the edge list of an id table
KNN_EDGES_SIGNATURES = {
    "se3_knn_query_pair_padded": (C.c_int, [_P, _P, _I64, _P, _P, _P, _I64, _P, _I32, _P, _P]),
    "se3_knn_edges_workspace_bytes": (_SZ, [_I64]),
    "se3_knn_edges_bounded": (C.c_int, [_P, _I64, _P, _I32, _I64, _P, _P, _P, _P, _SZ, _P]),
}

# Why a second registry: TABLES is the surface as tests/test_abi_tables.py pins it (seven headers, their declaration counts,
# build.HEADERS), and that file is a yardstick that does not change.  Headers added after it stand here, under the same rule
# -- the table lists exactly what the header declares, no name in two tables -- and get the same checks from a test file of
# their own, which places the header into TABLES for the duration of a test (tests/test_knn_edges_abi.py).
ADDED_TABLES = {
    "se3conv_knn_edges.h": KNN_EDGES_SIGNATURES,
}

# global pooling: one row per batch element, on padded clouds too, in a fixed order of additions
GLOBAL_POOL_SIGNATURES = {
    "se3_global_pool_workspace_bytes": (_SZ, [_I64, _I32, _I32, _I32]),
    "se3_global_pool": (C.c_int, [_P, _P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _P, _SZ, _P]),
    "se3_global_unpool": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P]),
}
GLOBAL_POOL_CHUNK = 128  # SE3_GLOBAL_POOL_CHUNK: points per chunk of the sum / avg order

# the point-cloud group norm: statistics per (batch element, channel group) in the same kind of fixed order
GROUP_NORM_SIGNATURES = {
    "se3_group_norm_workspace_bytes": (_SZ, [_I64, _I32, _I32, _I32, _I32]),
    "se3_group_norm_fwd": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _P, _I32, _I32, _I32, _F, _P, _P, _P, _P, _SZ, _P]),
    "se3_group_norm_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _P, _SZ, _P]),
}
GROUP_NORM_CHUNK = 64  # SE3_GROUP_NORM_CHUNK: points per chunk of the order of additions

# the loss and metrics head: masked, smoothed cross-entropy and the per-class counters of SemSegMetrics in one pass
SEG_HEAD_SIGNATURES = {
    "se3_seg_head_workspace_bytes": (_SZ, [_I64, _I32]),
    "se3_seg_loss_fwd": (C.c_int, [_P, _P, _I32, _P, _I64, _P, _I32, _F, _P, _P, _P, _P, _P, _SZ, _P]),
    "se3_seg_loss_bwd": (C.c_int, [_P, _P, _I32, _P, _P, _P, _P, _I64, _P, _I32, _F, _P, _P]),
}
SEG_HEAD_CHUNK = 256         # SE3_SEG_HEAD_CHUNK: rows per chunk of the loss sum
SEG_HEAD_TILE_CLASSES = 56   # SE3_SEG_HEAD_TILE_CLASSES: the widest row the LDS-tile form of the kernels takes
SEG_HEAD_MAX_CLASSES = 1024

# point-neighbourhood embeddings (the five kernel-MLP activations, the three kernel-point correlations) and the max aggregation
PNE_SIGNATURES = {
    "se3_pne_embed_workspace_bytes": (_SZ, [_I64, _I32, _I32, _I32]),
    "se3_pne_embed_fwd": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _P, _I32, _F, _P, _P, _I32, _P, _P]),
    "se3_pne_embed_bwd": (C.c_int, [_P, _P, _P, _P, _I64, _P, _I32, _P, _I32, _F, _P, _P, _I32, _P, _P, _P, _SZ, _P]),
    "se3_neigh_max_fwd": (C.c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I32, _I32, _P, _P, _P]),
    "se3_neigh_max_bwd": (C.c_int, [_P] * 9 + [_I64, _I64, _I64, _I32, _I32, _P, _P, _P]),
}
PNE_CHUNK = 1024     # SE3_PNE_CHUNK: edges per chunk of the order of additions of se3_pne_embed_bwd
PNE_MAX_KPTS = 64    # SE3_PNE_MAX_KPTS
# enum se3_pne_kind
PNE_KINDS = {"mlp_linear": 0, "mlp_relu": 1, "mlp_gelu": 2, "mlp_sin": 3, "mlp_softmax": 4, "kp_gauss": 5, "kp_linear": 6, "kp_box": 7}

# the attention stage of MultiHeadAttLayer / LoRAttConvLayer: a softmax per point and head over the basis functions of [N, 2V, K]
BASIS_ATT_SIGNATURES = {
    "se3_basis_att_workspace_bytes": (_SZ, [_I64, _I32, _I32, _I32]),
    "se3_basis_att_fwd": (C.c_int, [_P, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _P, _P]),
    "se3_basis_att_bwd": (C.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _SZ, _P]),
}
BASIS_ATT_CHUNK = 256        # SE3_BASIS_ATT_CHUNK: points per chunk of the order of additions of dpe
BASIS_ATT_MAX_BASIS = 64     # SE3_BASIS_ATT_MAX_BASIS

# the same attention edge-wise, without the aggregate [N, 2V, K]: per-edge scalars in place of T and dT
ATT_FUSED_SIGNATURES = {
    "se3_att_fused_workspace_bytes": (_SZ, [_I64, _I64, _I32, _I32, _I32]),
    "se3_att_fused_fwd": (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I32, _I32, _I32, _P, _P, _P]),
    "se3_att_fused_bwd": (C.c_int, [_P] * 10 + [_I64, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _SZ, _P]),
}
ATT_FUSED_CHUNK = 256        # SE3_ATT_FUSED_CHUNK: points per chunk of the order of additions of dpe
ATT_FUSED_SLAB = 64          # SE3_ATT_FUSED_SLAB: edges of a sample a wavefront holds at a time

# the augmentation pipeline on a batch: statistics per element, the affine table, apply + noise, keep masks, compaction
_U32 = C.c_uint32
_D = C.POINTER(C.c_double)   # host: the constants of a step
AUGMENT_SIGNATURES = {
    "se3_aug_stats_workspace_bytes": (_SZ, [_I64, _I32]),
    "se3_aug_stats": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _P, _P, _P, _SZ, _P]),
    "se3_aug_affine_step": (C.c_int, [_I32, _D, _F, _P, _P, _P, _I32, _P, _P]),
    "se3_aug_apply": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _I32, _P, _F, _F, _F, _F, _U32, _P, _U32, _P, _P, _P]),
    "se3_aug_keep_mask": (C.c_int, [_I32, _D, _F, _P, _P, _I64, _P, _I32, _P, _P, _U32, _P, _U32, _P, _P]),
    "se3_aug_compact_workspace_bytes": (_SZ, [_I64]),
    "se3_aug_compact": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _P, _P, _P, _P, _P, _SZ, _P]),
}
AUG_CHUNK = 256      # SE3_AUG_CHUNK: rows per chunk of the order of additions of se3_aug_stats
AUG_DRAWS = 8        # SE3_AUG_DRAWS: uniform numbers per (step, element); column 0 is the gate
AUG_CONSTS = 12      # SE3_AUG_CONSTS
# enum se3_aug_kind
AUG_KINDS = {"rot_axis": 0, "rot_3d": 1, "center": 2, "linear": 3, "mirror": 4, "translation": 5, "stdnorm": 6,
             "drop": 16, "crop_box": 17, "crop_pts": 18}

# ElasticDistortionAug on a batch: grid dims and offsets per (element, octave), blurred hashed noise grids, the look-up per row
ELASTIC_SIGNATURES = {
    "se3_elastic_workspace_bytes": (_SZ, [_I32, _I32]),
    "se3_elastic_plan": (C.c_int, [_P, _P, _P, _F, _D, _I32, _I32, _I64, _P, _P, _P, _SZ, _P]),
    "se3_elastic_grids": (C.c_int, [_P, _I32, _I32, _I64, _U32, _P, _U32, _P, _P, _P, _SZ, _P]),
    "se3_elastic_displace": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _P, _I32, _D, _P, _P, _P]),
}
ELASTIC_MAX_OCTAVES = 4            # SE3_ELASTIC_MAX_OCTAVES
ELASTIC_TILE = 8                   # SE3_ELASTIC_TILE: edge of the blur kernel's output tile
ELASTIC_MAX_QUOTIENT = 1 << 20     # SE3_ELASTIC_MAX_QUOTIENT: extent / granularity from which a box counts as not finite

# the optimizer step: gradient norm in a fixed order, clip coefficient, AdamW, schedule table and accumulation gate in device words
class Se3OptimTensor(C.Structure):
    """struct se3_optim_tensor (include/se3conv_optim.h): one row of the tensor table."""

    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("numel", C.c_int64), ("state_offset", C.c_int64)]


class Se3OptimChunk(C.Structure):
    """struct se3_optim_chunk (include/se3conv_optim.h): chunk `index` of tensor `tensor`."""

    _fields_ = [("tensor", C.c_int32), ("index", C.c_int32)]


_DBL = C.c_double
_I64P = C.POINTER(C.c_int64)  # host
OPTIM_SIGNATURES = {
    "se3_optim_plan": (C.c_int, [_I64P, _I32, C.POINTER(Se3OptimTensor), C.POINTER(Se3OptimChunk), _I64, _I64P, _I64P]),
    "se3_optim_workspace_bytes": (_SZ, [_I64]),
    "se3_optim_grad_norm": (C.c_int, [_P, _I32, _P, _I64, _P, _P, _SZ, _P]),
    "se3_optim_adamw_step": (C.c_int, [_P, _I32, _P, _I64, _P, _P, _P, _P, _P, _P, _I64, _DBL, _DBL, _DBL, _F, _I32, _I32, _I32,
                                       _P, _SZ, _P]),
}
OPTIM_CHUNK = 1024        # SE3_OPTIM_CHUNK: elements per chunk of the order of additions of the gradient norm
OPTIM_STATE_WORDS = 5     # SE3_OPTIM_STATE_WORDS: it, t, b1p, b2p, skipped (8 bytes each)
OPTIM_READOUT_WORDS = 4   # SE3_OPTIM_READOUT_WORDS: grad_norm, clip_coef, lr, stepped (4 bytes each)

# The third registry, and meant to be the last: tests/test_knn_edges_abi.py pins ADDED_TABLES to its one header the way
# tests/test_abi_tables.py pins TABLES to seven, so a header after those stands here, under the same rule and with the same
# checks from a test file of its own.  Such a test asserts that its header is IN this registry, never what the registry
# equals: the next header is one more line here and one more test file.  One of them did pin a position all the same:
# tests/test_pne_abi.py holds "se3conv_pne.h" to the END of this registry, and test files do not change, so a header added
# after it (se3conv_basis_att.h was the first) goes in FRONT of that line; the order here means nothing else.
EXTENSION_TABLES = {
    "se3conv_global_pool.h": GLOBAL_POOL_SIGNATURES,
    "se3conv_group_norm.h": GROUP_NORM_SIGNATURES,
    "se3conv_seg_head.h": SEG_HEAD_SIGNATURES,
    "se3conv_basis_att.h": BASIS_ATT_SIGNATURES,
    "se3conv_augment.h": AUGMENT_SIGNATURES,
    "se3conv_optim.h": OPTIM_SIGNATURES,
    "se3conv_att_fused.h": ATT_FUSED_SIGNATURES,
    "se3conv_elastic.h": ELASTIC_SIGNATURES,
    "se3conv_pne.h": PNE_SIGNATURES,
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises Se3LibraryError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Se3LibraryError(
            f"{LIB_PATH} not found: build it with `python -m se3conv3d_amd.build` "
            "(there is deliberately no CPU fallback for the HIP path)")
    lib = C.CDLL(LIB_PATH)
    lib.se3_abi_version.restype = C.c_int
    if lib.se3_abi_version() != ABI_VERSION:  # (checked before the symbols: an older library lacks some of them)
        raise Se3LibraryError(f"{LIB_PATH} has ABI version {lib.se3_abi_version()}, this binding expects {ABI_VERSION}: "
                              "rebuild it (`python -m se3conv3d_amd.build`)")
    for name, (res, args) in [item for tables in (TABLES, ADDED_TABLES, EXTENSION_TABLES) for table in tables.values() for item in table.items()]:
        try:
            fn = getattr(lib, name)
        except AttributeError:  # same ABI number, older build of it (entry points are added within a version): say so
            raise Se3LibraryError(f"{LIB_PATH} does not export {name}: it was built from older sources -- rebuild it "
                                  "(`python -m se3conv3d_amd.build`)") from None
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != SE3_OK:
        msg = load().se3_error_string(code).decode()
        raise Se3LibraryError(f"{what} failed with code {code}: {msg}")


def forms(shape: Se3Shape, backward: bool, want_feat: bool = True, want_params: bool = True, have_t: bool = False,
          cu_count: int = 256) -> list:
    """The "stage:form" lines of se3conv_forms (include/se3conv_forms.h): which kernel form every launch of a forward call
    (`have_t`: it keeps T) or of a backward call with that request would take.  Host only."""
    buf = C.create_string_buffer(4096)
    check(load().se3conv_forms(C.byref(shape), int(backward), int(want_feat), int(want_params), int(have_t), cu_count, buf,
                               len(buf)), "se3conv_forms")
    return buf.value.decode().split()
