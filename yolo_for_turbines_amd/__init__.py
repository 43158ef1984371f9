"""yolo_for_turbines_amd — MI355X-native YOLOv3 hot path (forward, box decode, NMS) behind the
call surface of GabeTsai/YOLO-For-Turbines (`code/model.py`, `code/utils.py`).

The on-disk directory is also reachable as ``yolo-for-turbines_amd`` (symlink; a hyphen is not a
legal Python identifier). Everything computes in ``libyolo_mi355x.so`` (hand-written gfx950 HIP);
there is no CPU fallback.
"""
from .graph import GraphedTrainStep
from .loss import FusedYOLOLoss, YOLOLoss
from .optim import SGD, Adam, AdamW, clip_grad_norm_
from .amp import GradScaler
from .ema import ModelEMA
from .model import CNNBlock, ResidualBlock, ScalePredictionBlock, YOLOv3, layer_config
from .utils import (save_checkpoint, load_checkpoint, accuracy_counts, build_targets, calc_iou, calc_mAP, evaluate_detections, evaluate_model, check_model_accuracy, eval_boxes, get_eval_boxes, letterbox, unletterbox_boxes, augment_params, augment_batch, train_batch, scaled_anchors, anchor_draws, kmeans_anchors, anchor_fitness, anchors_layout, cells_to_boxes, decode_boxes, detect, detect_images, detect_tiled, tile_grid, tile_pyramid, iou_aligned, nms_indices,
                    fuse_boxes, tta_views, tta_boxes, detect_tta,
                    non_max_suppression)
from .track import Tracker, TrackResult, track_images
# Soft-NMS and the NMS options: attributes of the package (yt.soft_nms, yt.NMSOptions) that are deliberately in neither __all__ -
# utils.py and its name list mirror the reference's utils module and stay as they are; the new names live in boxes.py.
from .boxes import NMSOptions, soft_nms
# ... and so is drawing (draw.py): yt.draw_boxes, yt.draw_tracks and the reference's plot_original / plot_image_with_boxes
from .draw import draw_boxes, draw_tracks, plot_image_with_boxes, plot_original
# ... and the frame front end (frames.py): yt.preprocess_frames, yt.FrameStager, yt.frames_to_rgb, yt.boxes_to_frames, yt.detect_frames
from .frames import FrameStager, boxes_to_frames, detect_frames, frames_to_rgb, preprocess_frames
# ... and training on tiles (crops.py): yt.CropPool, yt.crop_params, yt.crop_batch, yt.train_crops
from .crops import CropPool, crop_batch, crop_params, train_crops
# ... and the augmentation extras (extras.py): yt.extra_params, the table behind extra= of augment_batch and CropPool.batch
from .extras import EXTRA_NPARAM, extra_params

__all__ = ["YOLOLoss", "FusedYOLOLoss", "GraphedTrainStep", "SGD", "Adam", "AdamW", "clip_grad_norm_", "GradScaler", "ModelEMA", "CNNBlock", "ResidualBlock", "ScalePredictionBlock", "YOLOv3", "layer_config", "calc_iou",
           "cells_to_boxes", "decode_boxes", "detect", "detect_images", "detect_tiled", "fuse_boxes", "tta_views", "tta_boxes", "detect_tta", "tile_grid", "tile_pyramid", "iou_aligned", "nms_indices", "non_max_suppression", "build_targets", "calc_mAP", "evaluate_detections", "evaluate_model", "accuracy_counts", "check_model_accuracy", "eval_boxes", "get_eval_boxes", "letterbox", "unletterbox_boxes", "augment_params",
           "augment_batch", "train_batch", "scaled_anchors", "anchor_draws", "kmeans_anchors", "anchor_fitness", "anchors_layout",
           "Tracker", "TrackResult", "track_images"]
