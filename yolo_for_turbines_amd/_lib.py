"""ctypes binding of ``libyolo_mi355x.so`` (declared in ``include/yolo_mi355x.h``).

There is no CPU fallback: if the HIP library has not been built (``__graft_entry__.build()``
or ``make -C yolo_for_turbines_amd/csrc``) every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YOLO_MI355X_LIB") or os.path.join(_HERE, "libyolo_mi355x.so")

F32, F16, BF16 = 0, 1, 2
ACT_NONE, ACT_LEAKY, ACT_MISH = 0, 1, 2
OUT_NHWC, OUT_UPSAMPLE2X, OUT_HEAD = 0, 1, 2
FLAG_RESIDUAL, FLAG_NANCHECK, FLAG_FILTERS_READY, FLAG_SPLIT_BF16, FLAG_SPLIT_WEIGHTS_READY = 1, 2, 4, 8, 16
FLAG_SPLIT_K = 32
FLAG_FILTERS_APPENDED = 64
FLAG_WINO_SPLIT_BF16 = 128
FLAG_FILTER_PLANES = 256
WGRAD_KERNEL_F32, WGRAD_KERNEL_PATCH, WGRAD_KERNEL_DMA, WGRAD_KERNEL_STEM = 0, 1, 2, 3      # YOLO_WGRAD_KERNEL_* of the header
LOSS_BOX_KINDS = {"mse": 0, "giou": 1, "diou": 2, "ciou": 3}          # YOLO_LOSS_BOX_* / YOLO_LOSS_OBJ_* of the header
LOSS_OBJ_KINDS = {"mse": 0, "bce": 1}


class PackItem(C.Structure):
    """`yolo_pack_item` (include/yolo_mi355x.h)."""
    _fields_ = [("w_oihw", C.c_void_p), ("w_packed", C.c_void_p), ("cout", C.c_int), ("cin", C.c_int), ("ksize", C.c_int),
                ("reserved", C.c_int)]


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n", "h", "w", "cin", "cout", "ksize", "stride", "x_ld", "x_off", "y_ld", "y_off", "r_ld", "r_off",
        "act", "out_mode", "dtype", "flags", "tile")]


class ConvOp(C.Structure):
    _fields_ = [("d", ConvDesc)] + [(n, C.c_uint64) for n in ("x", "w_packed", "scale", "shift", "residual", "y",
                                                              "workspace", "workspace_bytes")]


class LossOpts(C.Structure):
    """`yolo_loss_opts` (include/yolo_mi355x.h): the terms of yolo_loss_fwd_opts / yolo_loss_bwd_opts."""
    _fields_ = [("box_kind", C.c_int), ("obj_kind", C.c_int), ("focal_gamma", C.c_float), ("label_smoothing", C.c_float),
                ("lambda_box", C.c_float), ("lambda_obj", C.c_float), ("lambda_noobj", C.c_float), ("lambda_class", C.c_float)]


class ClipState(C.Structure):
    """`yolo_clip_state` (include/yolo_mi355x.h): four 32-bit words in device memory; the host writes max_norm only."""
    _fields_ = [("max_norm", C.c_float), ("total_norm", C.c_float), ("coef", C.c_float), ("norm_type", C.c_int32)]


class TrackParams(C.Structure):
    """`yolo_track_params` (include/yolo_mi355x.h): the thresholds and switches of yolo_track_update, 64 bytes."""
    _fields_ = [("high_threshold", C.c_double), ("low_threshold", C.c_double), ("new_threshold", C.c_double), ("match_iou", C.c_double * 3),
                ("max_age", C.c_int32), ("center", C.c_int32), ("class_agnostic", C.c_int32), ("reserved", C.c_int32)]


class DrawParams(C.Structure):
    """`YoloDrawParams` (include/yolo_mi355x.h): the style of yolo_draw_boxes, 32 bytes."""
    _fields_ = [(n, C.c_int32) for n in ("thickness", "font_scale", "line_alpha", "fill_alpha", "labels", "scores", "color_by_id", "reserved")]


class FrameRow(C.Structure):
    """`yolo_frame_row` (include/yolo_mi355x.h): where one frame lies in the pool, 24 bytes."""
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("pitch", C.c_int32), ("reserved", C.c_int32)]


FRAME_FORMATS = {"rgb": 0, "bgr": 1, "nv12": 2}                        # YOLO_FRAMES_* / YOLO_CSC_* of the header
CSC_KINDS = {"bt601": 0, "bt601-full": 1, "bt709": 2, "bt709-full": 3}

NORM_KINDS = {2.0: 0, float("inf"): 1}                                 # YOLO_NORM_L2 / YOLO_NORM_INF of the header

CALL_MAX_ARGS = 24


class Call(C.Structure):
    """`yolo_call` (include/yolo_mi355x.h): one recorded launch of a train-step table."""
    _fields_ = [("fn", C.c_int32), ("reserved", C.c_int32), ("a", C.c_uint64 * CALL_MAX_ARGS)]


class Reloc(C.Structure):
    """`yolo_reloc`: a[arg] of calls[call] = slots[slot] + offset at run time."""
    _fields_ = [("call", C.c_int32), ("arg", C.c_int32), ("slot", C.c_int32), ("reserved", C.c_int32), ("offset", C.c_int64)]


# YOLO_FN_* of the header, by exported name
FN_IDS = {name: i + 1 for i, name in enumerate((
    "yolo_fill_zero", "yolo_copy_d2d", "yolo_nchw_to_nhwc", "yolo_stem_fwd", "yolo_conv_fwd", "yolo_bn_stats", "yolo_bn_act_fwd",
    "yolo_bn_act_bwd", "yolo_upsample2x_bwd", "yolo_conv_wgrad", "yolo_pack_weights_dgrad", "yolo_pack_weights_batch",
    "yolo_conv_dgrad_s2", "yolo_head_grad_to_nhwc", "yolo_conv_fwd_stats", "yolo_bn_stats_from_partials",
    "yolo_conv_dgrad_bstats", "yolo_bn_act_bwd_rows", "yolo_conv_fwd_ws", "yolo_head_grad_to_nhwc_hw"))}


class YoloLibError(RuntimeError):
    pass


_SIGS = {
    "yolo_last_error": (C.c_char_p, []),
    "yolo_version": (C.c_int, []),
    "yolo_switches_describe": (C.c_int, [C.c_char_p, C.c_size_t]),
    "yolo_packed_weight_elems": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "yolo_packed_weight_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "yolo_pack_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_unpack_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_bn_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                               C.c_int, C.c_void_p]),
    "yolo_nchw_to_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p]),
    "yolo_nhwc_to_nchw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p]),
    "yolo_fill_zero": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_copy_d2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_run_calls": (C.c_int, [C.POINTER(Call), C.c_int, C.POINTER(Reloc), C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_void_p]),
    "yolo_train_fwd_batch": (C.c_int, [C.POINTER(Call), C.c_int, C.POINTER(Reloc), C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_void_p]),
    "yolo_train_bwd_batch": (C.c_int, [C.POINTER(Call), C.c_int, C.POINTER(Reloc), C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_void_p]),
    "yolo_sgd_chunk_elems": (C.c_int, []),
    "yolo_sgd_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_sgd_check_finite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_ema_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_clip_norm_partials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_clip_finalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_clip_scale_grads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_adam_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_adam_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_stem_supported": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "yolo_stem_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_stem_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_conv_fwd": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_conv_fwd_batch": (C.c_int, [C.POINTER(ConvOp), C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_conv_workspace_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "yolo_conv_fwd_ws": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "yolo_conv_pick_tile": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_split3_eligible": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_split3_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_splitk_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_splitk_eligible": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_splitk_slices": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_split3_weight_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "yolo_split3_weights": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_conv_num_tiles": (C.c_int, []),
    "yolo_wino4_filter_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "yolo_wino4_filters": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_wino4_appended_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "yolo_wino4_appended_wanted": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_wino4_blocks": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "yolo_conv_patch_plan": (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.POINTER(C.c_int32)]),
    "yolo_conv_wino4_split_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_conv_wino4_split_eligible": (C.c_int, [C.POINTER(ConvDesc)]),
    "yolo_wino4_filter_plane_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "yolo_wino4_filter_planes": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_bn_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_bn_stats": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                C.c_size_t, C.c_void_p]),
    "yolo_conv_stats_rows": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),
    "yolo_conv_fwd_stats": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_bn_stats_from_partials": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_bn_act_fwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p]),
    "yolo_bn_act_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_conv_bstats_rows": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),
    "yolo_conv_dgrad_bstats": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_bn_act_bwd_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_upsample2x_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p]),
    "yolo_wgrad_workspace_bytes": (C.c_size_t, [C.c_int] * 8),
    "yolo_conv_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_wgrad_plan": (C.c_int, [C.c_int] * 12 + [C.POINTER(C.c_int32)]),
    "yolo_debug_tr_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_packed_dgrad_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "yolo_pack_weights_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_pack_weights_dgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_conv_dgrad_s2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_head_grad_to_nhwc": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p]),
    "yolo_head_grad_to_nhwc_hw": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_void_p]),
    "yolo_letterbox": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "yolo_letterbox_canvas": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "yolo_letterbox_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.c_void_p]),
    "yolo_augment_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "yolo_augment_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int,
                                     C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    "yolo_augment_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int,
                                      C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "yolo_build_targets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "yolo_build_targets_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_map_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_eval_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "yolo_eval_detections": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                       C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "yolo_accuracy_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                       C.c_void_p]),
    "yolo_accuracy_counts_hw": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_void_p, C.c_void_p]),
    "yolo_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_loss_workspace_bytes_hw": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "yolo_loss_fwd_hw": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_loss_bwd_hw": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_loss_fwd_opts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(LossOpts), C.c_void_p]),
    "yolo_loss_bwd_opts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LossOpts), C.c_void_p]),
    "yolo_loss_fwd": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_loss_bwd": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_decode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_decode3": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                               C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_decode3_ex": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int,
                                  C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_decode_hw": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_decode3_hw": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int,
                                  C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_decode3_hw_at": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_nms_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_sort_u64_workspace_bytes": (C.c_size_t, [C.c_int]),
    "yolo_sort_u64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_fuse_onchip_clusters": (C.c_int, []),
    "yolo_fuse_chunk_candidates": (C.c_int, []),
    "yolo_fuse_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_fuse_boxes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_soft_nms_onchip_rows": (C.c_int, []),
    "yolo_soft_nms_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_soft_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_track_state_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_track_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "yolo_track_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_track_update": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TrackParams),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_draw_tile": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "yolo_draw_chunk": (C.c_int, []),
    "yolo_draw_text_capacity": (C.c_int, []),
    "yolo_draw_font": (None, [C.c_char_p]),
    "yolo_draw_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_draw_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(DrawParams), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                  C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_frames_tile": (None, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "yolo_frames_csc_constants": (C.c_int, [C.c_int, C.POINTER(C.c_int32)]),
    "yolo_frames_letterbox": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "yolo_frames_to_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_boxes_to_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_tta_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_boxes_unflip": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_tile_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "yolo_tile_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_tile_collect_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_tile_collect": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_tile_level_hw": (C.c_int, [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "yolo_tile_gather_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "yolo_tile_collect_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                       C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_crop_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_crop_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    # the augmentation extras (extras.py): the four calls above with the (b, 24) extras table behind the augmentation table
    "yolo_augment_boxes_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int,
                                        C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_augment_images_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int,
                                         C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "yolo_crop_boxes_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p]),
    "yolo_crop_images_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_anchor_kmeans_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "yolo_anchor_kmeans": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_anchor_fitness_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "yolo_anchor_fitness": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
}

EXPORTS = tuple(_SIGS)
_lib = None


def lib():
    """The loaded library; raises YoloLibError when it is missing (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise YoloLibError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C yolo_for_turbines_amd/csrc`. This package has no CPU fallback.")
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:                                  # pragma: no cover
            raise YoloLibError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().yolo_last_error()
        raise YoloLibError(f"{what or 'libyolo_mi355x'} failed ({rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device pointer of a torch tensor (or 0 for None)."""
    return 0 if t is None else t.data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream
