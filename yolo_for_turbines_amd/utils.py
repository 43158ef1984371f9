"""Drop-in mirror of the reference's post-processing functions
(`/root/reference/code/utils.py:22-191`) on top of the HIP kernels.

Two levels:
  * list-returning wrappers with the reference's names and signatures (``cells_to_boxes``,
    ``non_max_suppression``, ``calc_iou``, ``iou_aligned``) so ``demo.predict`` /
    ``get_eval_boxes`` keep working unchanged (they pay the reference's ``.tolist()`` cost);
  * device-resident entries (``decode_boxes``, ``nms_indices``, ``detect``) that keep every
    intermediate in HBM and return tensors — this is the path that is benchmarked.
"""
# Re-exports only: the code lives in one module per stage (the module map in DESIGN.md).
from .boxes import STRIDES, calc_iou, cells_to_boxes, decode_boxes, detect, detect_images, iou_aligned, nms_indices, non_max_suppression, scaled_anchors, AnchorFitness, AnchorResult, anchor_draws, anchor_fitness, anchors_layout, kmeans_anchors
from .data import AUG_NPARAM, augment_batch, augment_params, build_targets, letterbox, train_batch, unletterbox_boxes
# the reference's two plotting functions (draw.py): attributes of this module that its __all__, pinned to the names of before, leaves out
from .draw import plot_image_with_boxes, plot_original
from .fuse import detect_tta, fuse_boxes, tta_boxes, tta_views
from .metrics import EVAL_MAX_THRESHOLDS, EvalMatches, EvalResult, accuracy_counts, calc_mAP, check_model_accuracy, eval_boxes, evaluate_detections, evaluate_model, get_eval_boxes
from .model import load_checkpoint, save_checkpoint
from .tiles import detect_tiled, tile_grid, tile_pyramid

__all__ = ["iou_aligned", "calc_iou", "cells_to_boxes", "non_max_suppression", "decode_boxes", "nms_indices",
           "detect", "detect_tiled", "fuse_boxes", "tta_views", "tta_boxes", "detect_tta", "tile_grid", "tile_pyramid", "build_targets", "calc_mAP", "evaluate_detections", "evaluate_model", "accuracy_counts", "check_model_accuracy", "eval_boxes", "get_eval_boxes", "letterbox", "unletterbox_boxes",
           "augment_params", "augment_batch", "train_batch",
           "save_checkpoint", "load_checkpoint", "scaled_anchors", "anchor_draws", "kmeans_anchors", "anchor_fitness", "anchors_layout"]
