"""ctypes binding of libaodhip.so (the C ABI declared in include/aod_hip.h).

The product path has NO CPU fallback: importing this module without the built library, or
calling an op on a non-GPU tensor, raises.  Tensors are passed as raw device pointers; kernels
are enqueued on torch's current HIP stream."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AOD_HIP_LIB') or os.path.join(_HERE, 'lib', 'libaodhip.so')      # AOD_HIP_LIB: instrumented debug builds (tools/dbg)


class AodHipError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(f'{LIB_PATH} is missing: run `python -m aod_meh_hua_amd.build` (hipcc, gfx950). '
                      'There is no CPU fallback for the MEH/HUA hot path.')
lib = C.CDLL(LIB_PATH)


class ConvSeg(C.Structure):
    _fields_ = [('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('OH', C.c_int32), ('OW', C.c_int32),
                ('src_row0', C.c_int64), ('dst_row0', C.c_int64)]


class ConvDesc(C.Structure):
    _fields_ = [('C', C.c_int32), ('N', C.c_int32), ('R', C.c_int32), ('S', C.c_int32), ('stride', C.c_int32),
                ('pad', C.c_int32), ('dil', C.c_int32), ('transposed', C.c_int32), ('relu', C.c_int32),
                ('out_f32', C.c_int32), ('nseg', C.c_int32), ('x3', C.c_int32), ('seg', ConvSeg * 8)]


class ConvPlan(C.Structure):
    """aod_conv_plan_t: the kernel a conv launch runs on (aod_conv2d_plan); kind 1 PW_STREAM, 2 SPLIT_K, 3 X3P, 4 IGEMM"""
    _fields_ = [(n, C.c_int32) for n in ('kind', 'bm', 'bn', 'nt', 'ops', 'stages', 'x3', 'grouped', 'ksplit', 'taps', 'wide', 'pre', 'lat', 'grid')]


class WgradPlan(C.Structure):
    """aod_wgrad_plan_t: the kernel and the splits a weight-gradient launch runs on (aod_conv2d_wgrad_plan_ex)"""
    _fields_ = ([(n, C.c_int32) for n in ('form', 'wide', 'waves', 'tile', 'x3', 'sparse', 'grouped', 'threads', 'lds_bytes', 'grid')]
                + [(n, C.c_int32 * 4) for n in ('tiles_n', 'tiles_k', 'splits', 'rows_per_split')])


WGRAD_ATOMIC, WGRAD_GROUPED = 1, 2
WGRAD_HAS_MAP = lambda g: 16 << g      # flag of aod_conv2d_wgrad_plan_ex: member g carries a row-activity map


P, I32, I64, F32, U64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64, C.c_size_t
_SIGS = {
    'aod_version': (C.c_int, []),
    'aod_conv_x3p_count': (C.c_int64, []),
    'aod_set_pointwise_mode': (C.c_int, [I32]),
    'aod_bottleneck64_fwd': (C.c_int, [P, I32, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck64x3_fwd': (C.c_int, [P, I32, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck64x3_ds_fwd': (C.c_int, [P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck64_ds_fwd': (C.c_int, [P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_halo_conv3x3_x3_applies': (C.c_int, [P]),
    'aod_halo_conv3x3_x3': (C.c_int, [P, P, P, P, P, P]),
    'aod_mfma_clock_probe': (C.c_int, [I32, I32, P, P, P]),
    'aod_bottleneck128x3_bwd': (C.c_int, [P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck128x3_fwd': (C.c_int, [P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck128_fwd': (C.c_int, [P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck_bwd': (C.c_int, [I32, P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_bottleneck256_fwd': (C.c_int, [P, I32, I32, I32, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_conv2d': (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P, P, P, P, P, P]),
    'aod_conv2d_ws_bytes': (SZ, [C.POINTER(ConvDesc)]),
    'aod_conv2d_ws': (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P, P, P, P, P, P, SZ, P]),
    'aod_conv2d_plan': (C.c_int, [C.POINTER(ConvDesc), I32, C.c_uint, C.POINTER(ConvPlan)]),
    'aod_conv2d_grouped': (C.c_int, [C.POINTER(ConvDesc), I32, P, P, P, P, P, P, P]),
    'aod_conv2d_ws_map': (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P, P, P, P, P, P, SZ, P, P, P]),
    'aod_conv2d_ws_map_order': (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P, P, P, P, P, P, SZ, P, P, P, P]),
    'aod_conv2d_x3p_item_order': (C.c_int, [I32, I32, I32, P, P, P, P]),
    'aod_conv2d_x3p_mapped_grid': (C.c_int, [I32, I32, I32]),
    'aod_conv_x3p_mapped_count': (C.c_int64, []),
    'aod_conv2d_grouped_map': (C.c_int, [C.POINTER(ConvDesc), I32, P, P, P, P, P, P, P, P, P]),
    'aod_fwd_row_maps': (C.c_int, [C.POINTER(ConvDesc), P, I32, I32, P, P]),
    'aod_conv2d_grouped_fwd_map': (C.c_int, [C.POINTER(ConvDesc), I32, P, P, P, P, P, P]),
    'aod_conv2d_grouped_deal': (C.c_int, [I32, I32, I32, P, P]),
    'aod_conv2d_grouped_map_order': (C.c_int, [C.POINTER(ConvDesc), I32, P, P, P, P, P, P, P, P, P, P]),
    'aod_conv2d_grouped_fwd_map_order': (C.c_int, [C.POINTER(ConvDesc), I32, P, P, P, P, P, P, P]),
    'aod_conv2d_tile_order': (C.c_int, [I32, I32, I32, P, P, P]),
    'aod_halo_conv3x3_applies': (C.c_int, [C.POINTER(ConvDesc)]),
    'aod_halo_conv3x3': (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P, P, P]),
    'aod_conv2d_wgrad': (C.c_int, [C.POINTER(ConvDesc), P, P, P, P, P]),
    'aod_conv2d_wgrad_splits': (C.c_int, [C.POINTER(ConvDesc)]),
    'aod_conv2d_wgrad_slabs': (C.c_int, [C.POINTER(ConvDesc), P, P, P, I32, I64, P, P]),
    'aod_conv2d_wgrad_slabs_map': (C.c_int, [C.POINTER(ConvDesc), P, P, P, I32, I64, P, P, P]),
    'aod_conv2d_wgrad_group_plan': (C.c_int, [P, I32, P]),
    'aod_conv2d_wgrad_grouped': (C.c_int, [P, I32, P, P, P, P, P, P, P]),
    'aod_conv2d_wgrad_plan': (C.c_int, [P, I32, P, P, P]),
    'aod_conv2d_wgrad_plan_ex': (C.c_int, [P, I32, C.c_uint, C.POINTER(WgradPlan)]),
    'aod_conv2d_wgrad_grouped_map': (C.c_int, [P, I32, P, P, P, P, P, P, P, P]),
    'aod_unpack_wgrad_slabs_grouped': (C.c_int, [I32, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    'aod_unpack_wgrad_slabs': (C.c_int, [P, I32, I64, P, I32, I32, I32, I32, I32, I32, P, P, P, P, P, P, P]),
    'aod_conv_row_table_bytes': (SZ, [C.POINTER(ConvDesc)]),
    'aod_conv_row_table': (C.c_int, [C.POINTER(ConvDesc), P, P]),
    'aod_pack_weight_fwd': (C.c_int, [P, P, I32, I32, I32, I32, I32, P]),
    'aod_param_prep': (C.c_int, [P, I32, I32, P]),
    'aod_param_prep_item_bytes': (C.c_int, []),
    'aod_pack_weight_dgrad': (C.c_int, [P, P, I32, I32, I32, I32, I32, P, P]),
    'aod_unpack_wgrad': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, I32, P, P, P, P, P, P, P]),
    'aod_nchw_f32_to_nhwc_bf16': (C.c_int, [P, P, I32, I32, I32, I32, I32, P]),
    'aod_nchw_f32_to_s2d_bf16': (C.c_int, [P, P, I32, I32, I32, I32, P]),
    'aod_stem_pool_fwd': (C.c_int, [P, P, P, P, P, I32, I32, I32, P]),
    'aod_set_deterministic': (C.c_int, [I32]),
    'aod_get_deterministic': (C.c_int, []),
    'aod_stem_pool_x3_fwd': (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, P]),
    'aod_maxpool3x3s2': (C.c_int, [P, P, I32, I32, I32, I32, P]),
    'aod_upsample2x_add': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, P]),
    'aod_upsample2x_add_bwd': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, P]),
    'aod_upsample2x_add_to': (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, P]),
    'aod_upsample2x_add_bwd_set': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, P]),
    'aod_act_bwd': (C.c_int, [P, P, P, P, P, P, P, P, P, P, I64, I32, I32, I32, P]),
    'aod_add_relu': (C.c_int, [P, P, P, I64, P]),
    'aod_pad_cast_colsum': (C.c_int, [P, P, P, P, I64, I32, I32, I32, P]),
    'aod_assign_ws_bytes': (SZ, [I32, I32]),
    'aod_max_iou_assign': (C.c_int, [P, P, I64, I32, P, P, P, I32, F32, F32, F32, I32, I32, P, P, P, P, P, P, P, P, P, I32, P, P]),
    'aod_loss_partials_len': (SZ, [I64]),
    'aod_edl_focal_l1_fwd': (C.c_int, [P, P, P, P, P, P, I64, I32, F32, F32, P, P, P, P]),
    'aod_edl_focal_l1_bwd': (C.c_int, [P, P, P, P, P, P, I64, I32, F32, F32, P, P, P, F32, I32, P, P, I32, I32, I32, I32, P]),
    'aod_edl_focal_elem': (C.c_int, [P, P, I64, I32, F32, F32, P, P, P]),
    'aod_meh_loss_fwd': (C.c_int, [P, P, P, I64, P, P, P]),
    'aod_meh_loss_bwd': (C.c_int, [P, P, P, I64, P, P, I32, I32, I32, P]),
    'aod_sigmoid_focal_l1_fwd': (C.c_int, [P, P, P, P, P, P, I64, I32, F32, F32, P, P, P, P]),
    'aod_sigmoid_focal_l1_bwd': (C.c_int, [P, P, P, P, P, P, I64, I32, F32, F32, P, P, P, F32, I32, P, P, I32, I32, I32, I32, P]),
    'aod_sigmoid_focal_elem': (C.c_int, [P, P, I64, I32, F32, F32, P, P, P]),
    'aod_sigmoid_focal_l1_levels_fwd': (C.c_int, [P, P, P, P, P, P, I32, P, I32, F32, F32, P, P, P, P, I32, P, P, P]),
    'aod_sigmoid_focal_l1_levels_bwd': (C.c_int, [P, P, P, P, P, P, I32, P, I32, F32, F32, P, P, P, P, P, I32, I32, I32, I32, P]),
    'aod_loss_levels_partials_len': (SZ, [I32, P]),
    'aod_edl_focal_l1_levels_fwd': (C.c_int, [P, P, P, P, P, P, I32, P, I32, F32, F32, P, P, P, P, I32, P, P, P]),
    'aod_edl_focal_l1_levels_bwd': (C.c_int, [P, P, P, P, P, P, I32, P, I32, F32, F32, P, P, P, P, P, I32, I32, I32, I32, P]),
    # (focal form, box form, box eps, box linear, means4, stds4, wh_ratio_clip) in front of the arguments of the entries above
    'aod_focal_box_fwd_ex': (C.c_int, [I32, I32, F32, I32, P, P, F32, P, P, P, P, P, P, I64, I32, F32, F32, P, P, P, P]),
    'aod_focal_box_bwd_ex': (C.c_int, [I32, I32, F32, I32, P, P, F32, P, P, P, P, P, P, I64, I32, F32, F32, P, P, P, F32, I32, P, P, I32, I32, I32, I32, P]),
    'aod_focal_box_levels_fwd_ex': (C.c_int, [I32, I32, F32, I32, P, P, F32, P, P, P, P, P, P, I32, P, I32, F32, F32, P, P, P, P, I32, P, P, P]),
    'aod_focal_box_levels_bwd_ex': (C.c_int, [I32, I32, F32, I32, P, P, F32, P, P, P, P, P, P, I32, P, I32, F32, F32, P, P, P, P, P, I32, I32, I32, I32, P]),
    'aod_meh_loss_levels_fwd': (C.c_int, [P, P, P, I32, P, P, P, P]),
    'aod_meh_loss_levels_bwd': (C.c_int, [P, P, P, I32, P, P, P, I32, I32, I32, P]),
    'aod_meh_loss_fwd_ex': (C.c_int, [P, P, P, I64, I32, P, P, P]),
    'aod_meh_loss_bwd_ex': (C.c_int, [P, P, P, I64, I32, P, P, I32, I32, I32, P]),
    'aod_meh_loss_levels_fwd_ex': (C.c_int, [P, P, P, I32, P, I32, P, P, P]),
    'aod_meh_loss_levels_bwd_ex': (C.c_int, [P, P, P, I32, P, I32, P, P, I32, I32, I32, P]),
    'aod_softmax_rowmax': (C.c_int, [P, I32, I64, I32, F32, P, P, I32, P]),
    'aod_topk_stable': (C.c_int, [P, I32, I64, I32, P, I64, P]),
    'aod_pre_nms_levels': (C.c_int, [I32, P, P, P, P, P, P, I32, I32, F32, I32, I32, P, P, P, P, F32, P, P, P, P, P, P, P, I64, P]),
    'aod_gather_decode': (C.c_int, [P, P, P, P, P, I32, I64, I32, I32, I64, P, P, P, P, F32, P, P, P, P, I64, I64, I64, I32, P]),
    'aod_nms_ws_bytes': (SZ, [I32, I32, I32]),
    'aod_multiclass_nms': (C.c_int, [P, P, I32, I32, I32, F32, F32, I32, P, P, P, P, P, P]),
    'aod_eval_match': (C.c_int, [P, P, P, P, P, P, P, I32, I32, I32, P, I32, P, P]),
    'aod_coco_match': (C.c_int, [P, P, P, P, P, P, P, P, I32, I32, I32, P, I32, P, I32, P, P]),
    'aod_hua_ws_bytes': (SZ, [I32, I32]),
    'aod_hua_score': (C.c_int, [P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, F32, F32, F32, I32, U64, P, I32, I32, I32, P, P, I32, P, P, P]),
    'aod_hua_score_ex': (C.c_int, [P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, F32, F32, F32, I32, U64, P, I32, I32, I32, P, P, I32, P,
                                   I32, P, P, P, P]),
    'aod_hua_score_ex2': (C.c_int, [P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, F32, F32, F32, I32, U64, P, I32, I32, I32, P, P, I32, P,
                                    I32, I32, P, P, P, P]),
    'aod_maxpool_fwd': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P]),
    'aod_maxpool_bwd': (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P]),
    'aod_l2norm_fwd': (C.c_int, [P, P, P, I64, I32, F32, P]),
    'aod_l2norm_bwd': (C.c_int, [P, P, P, P, P, I64, I32, F32, P]),
    'aod_ssd_loss_fwd': (C.c_int, [P, P, P, P, P, P, I32, I32, I32, I32, I32, F32, P, P, P, P]),
    'aod_ssd_loss_bwd': (C.c_int, [P, P, P, P, P, P, P, P, I32, I32, I32, I32, F32, P, P, P, P, P, P]),
    'aod_synth_normal_images': (C.c_int, [P, I32, I64, U64, P, P]),
    'aod_image_xform': (C.c_int, [P, P, I32, I32, I32, P, P]),
    'aod_x3_split': (C.c_int, [P, P, I64, I32, P]),
    'aod_x3_merge': (C.c_int, [P, P, I64, I32, P]),
    'aod_x3_add': (C.c_int, [P, P, P, I64, P]),
    'aod_x3_nchw_f32_to_s2d': (C.c_int, [P, P, I32, I32, I32, I32, P]),
    'aod_x3_maxpool3x3s2': (C.c_int, [P, P, I32, I32, I32, I32, P]),
    'aod_x3_upsample2x_add_to': (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, P]),
    'aod_x3_upsample2x_add_bwd_set': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, P]),
    'aod_x3_act_bwd': (C.c_int, [P, P, P, P, I64, I32, I32, P]),
    'aod_x3_pad_cast_colsum': (C.c_int, [P, P, P, P, I64, I32, P]),
    'aod_x3_pad_cast_colsum_map': (C.c_int, [P, P, P, P, I64, I32, P, P]),
    'aod_x3_nchw_f32_to_nhwc': (C.c_int, [P, P, I32, I32, I32, I32, P]),
    'aod_x3_maxpool_fwd': (C.c_int, [P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P]),
    'aod_x3_maxpool_bwd': (C.c_int, [P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P]),
    'aod_x3_l2norm_fwd': (C.c_int, [P, P, P, I64, I32, F32, P]),
    'aod_x3_l2norm_bwd': (C.c_int, [P, P, P, P, P, I64, I32, F32, P]),
    'aod_sgd_multi': (C.c_int, [P, P, P, P, I32, F32, P, F32, F32, I32, F32, P]),
    'aod_sgd_multi_clipped': (C.c_int, [P, P, P, P, I32, F32, P, F32, F32, I32, F32, P, P]),
    'aod_grad_norm_multi': (C.c_int, [P, P, I32, F32, F32, I32, P, I64, P, P]),
    'aod_ensemble_mi_partials_len': (SZ, [I32, P, I32]),
    'aod_ensemble_mi': (C.c_int, [P, I32, I32, P, I32, I32, P, P, I64, P]),
    'aod_dropout2d_masks': (C.c_int, [P, P, I32, P, I32, I32, F32, U64, C.c_uint32, P]),
    'aod_dropout2d_apply': (C.c_int, [P, P, I64, I32, I32, I32, I32, P]),
    'aod_dropout2d_apply_multi': (C.c_int, [P, P, I64, I32, I32, P, P, P, I32, I32, P]),
    'aod_pool_descriptor': (C.c_int, [P, I32, P, P, I32, I32, I32, P, I64, P]),
    'aod_kcenter_chunk': (C.c_int, []),
    'aod_kcenter_ws_len': (SZ, [I64]),
    'aod_kcenter_greedy': (C.c_int, [P, I64, I32, P, I64, I64, P, P, P, P, P]),
    'aod_kcenter_greedy_ex': (C.c_int, [P, I64, I32, P, I64, I64, P, P, P, P, P, I32]),
    'aod_cdal_chunk': (C.c_int, []),
    'aod_cdal_ws_len': (SZ, [I32, P, I32, I32]),
    'aod_cdal_descriptor': (C.c_int, [P, I32, P, I32, I32, F32, P, I64, P, I64, P]),
    'aod_det_uncertainty': (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P]),
    'aod_det_uncertainty_ex': (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P]),
    'aod_object_descriptors': (C.c_int, [P, I32, P, P, I32, I32, I32, P, I32, P, P, P, P, I32, I32, F32, P, P, P, P, P, P]),
    'aod_ccms_max_images': (C.c_int, []),
    'aod_ccms_distance': (C.c_int, [P, P, P, P, I32, I32, I32, P, P]),
    'aod_kcenter_greedy_matrix': (C.c_int, [P, I64, P, I64, I64, P, P, P, P, P]),
    'aod_object_measure': (C.c_int, [P, P, P, P, I32, I32, I32, F32, P, P]),
    'aod_enms_prototypes': (C.c_int, [P, P, P, P, P, I32, I32, I32, F32, P, P, P, P, P, P, P, P]),
    'aod_divproto_chunk': (C.c_int, []),
    'aod_divproto_ws_len': (SZ, [I64, I32, I64]),
    'aod_divproto_select': (C.c_int, [P, I64, I64, P, P, P, P, I32, I32, I32, I64, F32, F32, I32, I64, I64, I32, I32, P, P, P, P]),
    'aod_object_posterior': (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, F32, P, P]),
    'aod_badge_embedding': (C.c_int, [P, P, P, P, I32, I32, I32, I32, I32, P, I64, P]),
    'aod_kmeanspp_block': (C.c_int, []),
    'aod_kmeanspp_ws_len': (SZ, [I64]),
    'aod_kmeanspp_seed': (C.c_int, [P, I64, I32, P, I64, I64, P, P, P, P, P, P, P]),
    'aod_loc_stability_max_levels': (C.c_int, []),
    'aod_pixel_noise': (C.c_int, [P, P, I32, I32, I32, I32, P, P, F32, I32, U64, P, P]),
    'aod_loc_stability': (C.c_int, [P, P, P, I32, I32, I32, F32, I32, I32, P, P, P]),
    'aod_class_difficulty_ws_len': (SZ, [I64, I32]),
    'aod_class_difficulty_accum': (C.c_int, [P, P, P, P, P, I64, I32, I32, P, P, F32, F32, P, P, P]),
    'aod_class_difficulty_update': (C.c_int, [P, P, I32, F32, P]),
    'aod_det_uncertainty_w': (C.c_int, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, F32, P, P, P, P, P, P]),
    'aod_consistency_max_views': (C.c_int, []),
    'aod_flip_images': (C.c_int, [P, P, I32, I32, I32, I32, P, I32, P]),
    'aod_det_posterior': (C.c_int, [P, P, P, I32, I32, I32, I32, P, P, P]),
    'aod_det_consistency': (C.c_int, [P, P, P, P, I32, P, P, I32, I32, I32, I32, I32, I32, F32, I32, P, P, P, P, P, P]),
}
for _n, (_r, _a) in _SIGS.items():
    if hasattr(lib, _n):
        getattr(lib, _n).restype = _r
        getattr(lib, _n).argtypes = _a
lib.aod_last_error.restype = C.c_char_p


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses CPU tensors: no CPU path exists."""
    if t is None:
        return None
    if not t.is_cuda:
        raise AodHipError('aod_meh_hua_amd ops need tensors on the MI355X (cuda:N); got a CPU tensor. There is no CPU fallback.')
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, name='aod'):
    if rc != 0:
        raise AodHipError(f'{name} failed ({rc}): {lib.aod_last_error().decode()}')


def call(name, *args):
    check(getattr(lib, name)(*args), name)
