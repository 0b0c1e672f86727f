"""ctypes binding of libspx_hip.so (include/spx_hip.h).

The HIP extension is the only compute path of this package: loading fails
loudly when the shared library is missing, and every operator raises when its
tensors are not on an AMD GPU.  There is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libspx_hip.so")
SPX_MAX_PANELS = 64
ABI_VERSION = 17


class SpxError(RuntimeError):
    """A libspx_hip.so entry point returned a non-zero status."""


class SpxPlan(C.Structure):
    _fields_ = [
        ("num_prototypes", C.c_int32),
        ("num_classes", C.c_int32),
        ("num_scales", C.c_int32),
        ("channels_per_scale", C.c_int32),
        ("kc", C.c_int32),
        ("npb", C.c_int32),
        ("ncb", C.c_int32),
        ("npanels", C.c_int32),
        ("panel_ch0", C.c_int32 * SPX_MAX_PANELS),
        ("panel_p0", C.c_int32 * SPX_MAX_PANELS),
        ("panel_np", C.c_int32 * SPX_MAX_PANELS),
    ]


class SpxCe(C.Structure):
    """spx_ce of include/spx_hip.h: the cross-entropy attachment of spx_dist_fwd_ce / spx_dist_bwd_ce."""

    _fields_ = [
        ("labels", C.c_void_p),
        ("lse", C.c_void_p),
        ("pred", C.c_void_p),
        ("partials", C.c_void_p),
        ("logits", C.c_void_p),
        ("coef", C.c_void_p),
        ("d_logits_out", C.c_void_p),
    ]


SPX_CE_MAX_SEGMENTS = 16


class SpxCeSegments(C.Structure):
    """spx_ce_segments of include/spx_hip.h: the row ranges of the segmented cross entropy (copied into the kernel arguments)."""

    _fields_ = [
        ("S", C.c_int32),
        ("off", C.c_int64 * (SPX_CE_MAX_SEGMENTS + 1)),
    ]


class SpxReg(C.Structure):
    """spx_reg of include/spx_hip.h: the weight-side regularisers' inputs (spx_reg_fwd / spx_reg_bwd)."""

    _fields_ = [
        ("wd", C.c_void_p),
        ("U", C.c_int32),
        ("P", C.c_int32),
        ("row_block", C.c_void_p),
        ("row_local", C.c_void_p),
        ("col_block", C.c_void_p),
        ("col_local", C.c_void_p),
        ("flat_col", C.c_void_p),
        ("block_info", C.c_void_p),
        ("spans", C.c_void_p),
        ("nblocks", C.c_int32),
        ("G", C.c_int32),
        ("S", C.c_int32),
        ("nspans", C.c_int32),
        ("head", C.c_void_p),
        ("ident", C.c_void_p),
        ("K", C.c_int32),
        ("Uh", C.c_int32),
        ("epsilon", C.c_float),
        ("weights", C.c_float * 4),
        ("terms", C.c_int32),
    ]


class SpxActLoss(C.Structure):
    """spx_actloss of include/spx_hip.h: the activation losses' inputs (spx_actloss_*)."""

    _fields_ = [
        ("vals", C.c_void_p),
        ("labels", C.c_void_p),
        ("slot_scale", C.c_void_p),
        ("B", C.c_int32),
        ("J", C.c_int32),
        ("HW", C.c_int32),
        ("W", C.c_int32),
        ("K", C.c_int32),
        ("mode", C.c_int32),
        ("terms", C.c_int32),
        ("norm_type", C.c_int32),
        ("epsilon", C.c_float),
        ("weights", C.c_float * 3),
    ]


SPX_BATCH_MAX_GRIDS = 4


class SpxBatchSample(C.Structure):
    """spx_batch_sample of include/spx_hip.h: one sample's descriptor of spx_batch_prepare (80 bytes, in device memory)."""

    _fields_ = [
        ("image", C.c_void_p),
        ("label", C.c_void_p),
        ("image_row_stride", C.c_int64),
        ("label_row_stride", C.c_int64),
        ("image_pixel_stride", C.c_int32),
        ("label_dtype", C.c_int32),
        ("h", C.c_int32),
        ("w", C.c_int32),
        ("hs", C.c_int32),
        ("ws", C.c_int32),
        ("y0", C.c_int32),
        ("x0", C.c_int32),
        ("flip", C.c_int32),
        ("row_tab", C.c_int32),
        ("col_tab", C.c_int32),
        ("reserved", C.c_int32),
    ]


class SpxBatch(C.Structure):
    """spx_batch of include/spx_hip.h: the batch-wide arguments of spx_batch_prepare / spx_resize_labels."""

    _fields_ = [
        ("samples", C.c_void_p),
        ("index", C.c_void_p),
        ("id_map", C.c_void_p),
        ("labels_in", C.c_void_p),
        ("image_out", C.c_void_p),
        ("window_labels", C.c_void_p),
        ("latent", C.c_void_p * SPX_BATCH_MAX_GRIDS),
        ("latent0", C.c_void_p * SPX_BATCH_MAX_GRIDS),
        ("n_index", C.c_int32),
        ("L", C.c_int32),
        ("labels_dtype", C.c_int32),
        ("B", C.c_int32),
        ("Hc", C.c_int32),
        ("Wc", C.c_int32),
        ("G", C.c_int32),
        ("grid_h", C.c_int32 * SPX_BATCH_MAX_GRIDS),
        ("grid_w", C.c_int32 * SPX_BATCH_MAX_GRIDS),
        ("grid_rt", C.c_int32 * SPX_BATCH_MAX_GRIDS),
        ("grid_ct", C.c_int32 * SPX_BATCH_MAX_GRIDS),
        ("normalize", C.c_int32),
        ("round_u8", C.c_int32),
        ("out_u8", C.c_int32),
        ("mean", C.c_float * 3),
        ("std", C.c_float * 3),
    ]


SPX_MSC_MAX_MAPS = 8


class SpxMscMap(C.Structure):
    """spx_msc_map of include/spx_hip.h: one map of spx_msc_max_fwd / spx_msc_max_bwd (strides in elements)."""

    _fields_ = [
        ("data", C.c_void_p),
        ("batch_stride", C.c_int64),
        ("channel_stride", C.c_int64),
        ("h", C.c_int32),
        ("w", C.c_int32),
    ]


class SpxMsc(C.Structure):
    """spx_msc of include/spx_hip.h: the arguments of spx_msc_max_fwd / spx_msc_max_bwd."""

    _fields_ = [
        ("maps", SpxMscMap * SPX_MSC_MAX_MAPS),
        ("grads", C.c_void_p * SPX_MSC_MAX_MAPS),
        ("out", C.c_void_p),
        ("index", C.c_void_p),
        ("g", C.c_void_p),
        ("K", C.c_int32),
        ("B", C.c_int32),
        ("C", C.c_int32),
        ("in_dtype", C.c_int32),
        ("out_dtype", C.c_int32),
        ("g_dtype", C.c_int32),
        ("activation", C.c_int32),
        ("reserved", C.c_int32),
    ]


_PP = C.POINTER(SpxPlan)
_PM = C.POINTER(SpxMsc)
_PB = C.POINTER(SpxBatch)
_PCE = C.POINTER(SpxCe)
_PR = C.POINTER(SpxReg)
_PA = C.POINTER(SpxActLoss)
_PS = C.POINTER(SpxCeSegments)
_V = C.c_void_p
_I = C.c_int32
_F = C.c_float
_PL = C.POINTER(C.c_int64)

# name -> (restype, argtypes); must list every symbol include/spx_hip.h declares
SIGNATURES = {
    "spx_version": (C.c_int, []),
    "spx_last_error": (C.c_char_p, []),
    "spx_make_plan": (C.c_int, [_I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _PP]),
    "spx_packed_bank_bytes": (C.c_size_t, [_PP]),
    "spx_packed_bankT_bytes": (C.c_size_t, [_PP]),
    "spx_packed_p2_bytes": (C.c_size_t, [_PP]),
    "spx_packed_head_bytes": (C.c_size_t, [_PP]),
    "spx_packed_headT_bytes": (C.c_size_t, [_PP]),
    "spx_pack_bank": (C.c_int, [_PP, _V, _V, _V, _V, _V]),
    "spx_pack_head": (C.c_int, [_PP, _V, _V, _V, _V]),
    "spx_pack_all": (C.c_int, [_PP, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V]),
    "spx_dist_fwd": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _V, _F, _I, _V]),
    "spx_dist_bwd": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _F, _I, _V]),
    "spx_dist_fwd_cls": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _I, _V, _V, _V, _F, _I, _V]),
    "spx_dist_bwd_cls": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _F, _I, _V]),
    "spx_group_dense": (C.c_int, [_V, _V, _I, _V, _V, _V, _V, _I, _I, _V, _V]),
    "spx_group_dense_bwd": (C.c_int, [_V, _V, _V, C.c_int64, _I, _V, _V]),
    "spx_simplex_project": (C.c_int, [_V, _V, _V, _I, _F, _V]),
    "spx_packed_tail_bytes": (C.c_size_t, [_PP]),
    "spx_pack_group_tail": (C.c_int, [_PP, _V, _I, _V, _V, _V]),
    "spx_pack_headT_units": (C.c_int, [_PP, _V, _V, _V]),
    "spx_dist_fwd_group": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _I, _V, _V, _V, _V, _F, _I, _V]),
    "spx_dist_bwd_group": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _F, _I, _V]),
    "spx_bwd_scratch_bytes": (C.c_size_t, [_PP, _I, _I]),
    "spx_bwd_head_scratch_bytes": (C.c_size_t, [_PP, _I, _I]),
    "spx_bwd_dx_scratch_bytes": (C.c_size_t, [_PP, _I, _I, _I]),
    "spx_bank_bwd_workspace_bytes": (C.c_size_t, [_PP, _I, _I]),
    "spx_bank_bwd": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _V, _V, _V]),
    "spx_push_argmin": (C.c_int, [_V, _V, _V, _I, _I, _I, _I, _I, _F, _V, _V, _V, _V]),
    "spx_dist_push_min": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _I, _I, _V, _F, _V, _V, _V, _V]),
    "spx_argmin_images": (C.c_int, [_V, _I, _I, _V, _V]),
    "spx_kld_segment_max": (C.c_int, [_V, _V, _I, _I, _I, _I, _I, _V, _V, _V, _V]),
    "spx_kld_segment_sumexp": (C.c_int, [_V, _V, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_kld_segment_lse": (C.c_int, [_V, _V, _I, _V, _V, _I, _V, _V]),
    "spx_kld_gram_loss": (C.c_int, [_V, _V, _V, _V, _I, _I, _I, _V, _V, _V, _V, _V]),
    "spx_kld_pair_sums": (C.c_int, [_V, _V, _I, _I, _I, _I, _I, _V, _V, _V, _V]),
    "spx_kld_backward": (C.c_int, [_V, _V, _I, _I, _I, _I, _V, _V, _V, _V, _V, _V]),
    "spx_upsample_argext": (C.c_int, [_V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_fwd_split_groups": (C.c_int32, [_PP, _I, _I]),
    "spx_fwd_split_workspace_bytes": (C.c_size_t, [_PP, _I, _I]),
    "spx_dist_fwd_ws": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V, _V, _F, _I, _V]),
    "spx_group_tail_workspace_bytes": (C.c_size_t, [_PP, _I, _I]),
    "spx_dist_fwd_group_ws": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _I, _V, _V, _V, _V, _PCE, _V, _F, _I, _V]),
    "spx_dist_bwd_group_ce": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _I, _V, _V, _V, _PCE, _V, _V, _V, _V, _V, _V, _F, _I, _V]),
    "spx_exp": (C.c_int, [_V, _V, C.c_int64, _V]),
    "spx_exp_bwd": (C.c_int, [_V, _V, _V, C.c_int64, _V]),
    "spx_pixel_outer_workspace_bytes": (C.c_size_t, [C.c_int64, _I, _I]),
    "spx_pixel_outer": (C.c_int, [_V, _V, C.c_int64, _I, _I, _V, _V, _V]),
    "spx_rows_gemm_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "spx_rows_gemm": (C.c_int, [_V, C.c_int64, C.c_int64, _V, C.c_int64, C.c_int64, _V, C.c_int64, _I, _I, _I, _I, _V, C.c_int64, _V, _V]),
    "spx_ce_partials": (C.c_size_t, [_I, _I]),
    "spx_ce_partials_flat": (C.c_size_t, [C.c_int64]),
    "spx_ce_finish": (C.c_int, [_V, C.c_int64, _V, _V, _V]),
    "spx_shift_labels": (C.c_int, [_V, _I, C.c_int64, _V, _V]),
    "spx_dist_fwd_ce": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _I, _V, _V, _V, _V, _PCE, _F, _I, _V]),
    "spx_dist_bwd_ce": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _V, _V, _V, _I, _V, _V, _V, _PCE, _V, _V, _V, _V, _F, _I, _V]),
    "spx_ce_fwd": (C.c_int, [_V, _V, C.c_int64, _I, _V, _V, _V, _V]),
    "spx_ce_bwd": (C.c_int, [_V, _V, _V, _V, C.c_int64, _I, _V, _V]),
    "spx_ce_seg_partials": (C.c_size_t, [_PS]),
    "spx_ce_seg_fwd": (C.c_int, [_V, _V, _PS, _I, _V, _V, _V, _V]),
    "spx_ce_seg_finish": (C.c_int, [_V, _PS, _V, _V, _V, _V, _V, _V]),
    "spx_ce_seg_bwd": (C.c_int, [_V, _V, _V, _PS, _V, _V, _V, _I, _V, _V]),
    "spx_eval_accumulate": (C.c_int, [_V, _PL, _V, _PL, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_eval_topk": (C.c_int, [_V, _PL, _V, _PL, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_eval_check_classes": (C.c_int, [C.POINTER(_I), _I, _I]),
    "spx_prune_argmin": (C.c_int, [_V, _V, _I, _I, _I, _I, _V, _V]),
    "spx_dist_prune_min": (C.c_int, [_PP, _V, _I, _I, _I, _V, _V, _V, _I, _V, _V, _V]),
    "spx_prune_footprint": (C.c_int, [_V, _I, _I, _I, _I, _I, _I, _V, _V, _V, _V, _V]),
    "spx_prune_merge": (C.c_int, [_V, _V, _V, _I, _I, _I, C.c_int64, _I, _V, _V, _V, _V, _V, _V]),
    "spx_reg_workspace_bytes": (C.c_size_t, [_PR]),
    "spx_reg_fwd": (C.c_int, [_PR, _V, _V, _V, _V]),
    "spx_reg_bwd": (C.c_int, [_PR, _V, _V, _V, _V, _V]),
    "spx_actloss_workspace_bytes": (C.c_size_t, [_PA]),
    "spx_actloss_segment_max": (C.c_int, [_PA, _V, _V]),
    "spx_actloss_segment_sums": (C.c_int, [_PA, _V, _V]),
    "spx_actloss_finish": (C.c_int, [_PA, _V, _V, _V, _V]),
    "spx_actloss_backward": (C.c_int, [_PA, _V, _V, _V, _V, _V]),
    "spx_overlap_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "spx_overlap_thresholds": (C.c_int, [_V, _PL, _I, _I, _I, _I, _I, _I, C.c_int64, _F, _V, _V, _V]),
    "spx_overlap_accumulate": (C.c_int, [_V, _PL, _V, _V, _I, _V, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V, _V, _V]),
    "spx_push_boxes": (C.c_int, [_V, _PL, _V, _I, _V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_push_boxes_rows": (C.c_int, [_V, _PL, _V, _I, _V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_masked_workspace_bytes": (C.c_size_t, [_I]),
    "spx_masked_thresholds": (C.c_int, [_V, _PL, _V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, C.c_double, _V, _V, _V]),
    "spx_patch_majority": (C.c_int, [_V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V]),
    "spx_nearest_protos": (C.c_int, [_V, _V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_explain_range": (C.c_int, [_V, _PL, _V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V]),
    "spx_explain_heat": (C.c_int, [_V, _PL, _V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V, _V]),
    "spx_explain_dominant": (C.c_int, [_V, _PL, _V, _I, _V, _V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V]),
    "spx_predict_accumulate": (C.c_int, [_V, _PL, _V, _I, _V, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_failure_table": (C.c_int, [_V, _I, _I, C.c_double, _V, _V, _V, _V]),
    "spx_paired_range": (C.c_int, [_V, _PL, _V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V]),
    "spx_paired_heat": (C.c_int, [_V, _PL, _V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V, _V]),
    "spx_push_merge": (C.c_int, [_V, _V, _V, _I, _I, _I, _I, _I, _I, _V, C.c_int64, _V, _V, _V, _V, _V]),
    "spx_scale_agg_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "spx_scale_agg_fwd": (C.c_int, [_V, _I, C.c_int64, _V, _I, _V, _V, _I, _I, _I, _I, _I, _F, _V]),
    "spx_scale_agg_bwd": (C.c_int, [_V, _I, C.c_int64, _V, _I, _V, _V, _V, _V, _V, _V, _I, _I, _I, _I, _I, _F, _V]),
    "spx_part_components_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "spx_part_components": (C.c_int, [_V, _I, _V, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_part_thresholds_workspace_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "spx_part_thresholds": (C.c_int, [_V, _PL, _V, _I, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, C.c_double, _I, _V, _V, _V]),
    "spx_part_presence": (C.c_int, [_V, _PL, _V, _I, _V, _I, _V, _V, _V, _V, _V, _I, _I, _I, _I, _I, _I, _I, _I, _I, _V, _V, _V]),
    "spx_part_fold_consistency": (C.c_int, [_V, _V, _V, _I, _I, _I, _I, _I, _V, _V]),
    "spx_part_fold_stability": (C.c_int, [_V, _V, _V, _V, _I, _I, _I, _I, _I, _V, _V]),
    "spx_batch_prepare": (C.c_int, [_PB, _V]),
    "spx_resize_labels": (C.c_int, [_PB, _V]),
    "spx_msc_max_fwd": (C.c_int, [_PM, _V]),
    "spx_msc_max_bwd": (C.c_int, [_PM, _V]),
    "spx_msc_pack_fwd": (C.c_int, [_PM, _I, _V]),
    "spx_msc_pack_bwd": (C.c_int, [_PM, _I, _V]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libspx_hip.so (built by scaleprotoseg_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SpxError(
            f"{LIB_PATH} is missing: build it with `python -m scaleprotoseg_amd.build` "
            "(hipcc --offload-arch=gfx950).  scaleprotoseg_amd has no CPU fallback."
        )
    # development A/B only (tools/ab_variants.sh): another build of the SAME library; never a different backend
    lib = C.CDLL(os.environ.get("SPX_LIB_OVERRIDE") or LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.spx_version() != ABI_VERSION:
        raise SpxError(f"libspx_hip.so ABI {lib.spx_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != 0:
        raise SpxError(load().spx_last_error().decode("utf-8", "replace"))


def require_gpu(t, what: str = "input") -> None:
    """Raise unless ``t`` (a tensor or a ``torch.device``) is on the GPU: the package's one statement of 'no CPU fallback'."""
    if not (t.type == "cuda" if isinstance(t, torch.device) else t.is_cuda):
        dev = t if isinstance(t, torch.device) else t.device
        raise SpxError(f"{what} is on {dev}: scaleprotoseg_amd runs on an AMD GPU only; there is no CPU fallback")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Raw device pointer of a dense GPU tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:            # (tested here first: ptr() runs a hundred times per step, the call is for the message)
        require_gpu(t)
    if not t.is_contiguous():
        raise SpxError("tensor must be contiguous")
    return t.data_ptr()


def stream_ptr() -> int:
    """hipStream_t of torch's current stream (the raw getter: ``torch.cuda.current_stream()`` builds a Stream object,
    ~20 us per call, which is visible at the launch-bound training shapes)."""
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is None:
        return torch.cuda.current_stream().cuda_stream
    return raw(torch.cuda.current_device())


def make_plan(P: int, K: int, S: int, Cs: int, scale_lo, scale_hi) -> SpxPlan:
    lib = load()
    plan = SpxPlan()
    lo = (C.c_int32 * S)(*[int(v) for v in scale_lo])
    hi = (C.c_int32 * S)(*[int(v) for v in scale_hi])
    check(lib.spx_make_plan(P, K, S, Cs, lo, hi, C.byref(plan)))
    return plan
