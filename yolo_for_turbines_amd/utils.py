"""Drop-in mirror of the reference's post-processing functions
(`/root/reference/code/utils.py:22-191`) on top of the HIP kernels.

Two levels:
  * list-returning wrappers with the reference's names and signatures (``cells_to_boxes``,
    ``non_max_suppression``, ``calc_iou``, ``iou_aligned``) so ``demo.predict`` /
    ``get_eval_boxes`` keep working unchanged (they pay the reference's ``.tolist()`` cost);
  * device-resident entries (``decode_boxes``, ``nms_indices``, ``detect``) that keep every
    intermediate in HBM and return tensors — this is the path that is benchmarked.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import torch

from . import _lib as L

__all__ = ["iou_aligned", "calc_iou", "cells_to_boxes", "non_max_suppression", "decode_boxes", "nms_indices",
           "detect", "detect_tiled", "fuse_boxes", "tta_views", "tta_boxes", "detect_tta", "tile_grid", "tile_pyramid", "build_targets", "calc_mAP", "evaluate_detections", "evaluate_model", "accuracy_counts", "check_model_accuracy", "eval_boxes", "get_eval_boxes", "letterbox", "unletterbox_boxes",
           "augment_params", "augment_batch", "train_batch",
           "save_checkpoint", "load_checkpoint", "scaled_anchors", "anchor_draws", "kmeans_anchors", "anchor_fitness", "anchors_layout"]


# -------------------------------------------------------------------------------- IoU
def iou_aligned(box1, box2):
    """Width/height IoU of centre-aligned boxes (utils.py:22-36). Elementwise torch ops; not on
    the accelerated path (used by the dataset's anchor matching)."""
    inter = torch.min(box1[..., 0], box2[..., 0]) * torch.min(box1[..., 1], box2[..., 1])
    return inter / (box1[..., 0] * box1[..., 1] + box2[..., 0] * box2[..., 1] - inter)


def calc_iou(boxes1, boxes2, box_format="center"):
    """IoU of cxcywh ("center") or x1y1wh (anything else) boxes, +1e-6 in the denominator
    (utils.py:38-84). Elementwise torch ops on whatever device the inputs live on: it is the
    objectness-loss helper (loss.py:64); inside NMS the same arithmetic runs in the HIP kernel."""
    if boxes1.dim() == 1:
        boxes1 = boxes1.unsqueeze(0)
    if boxes2.dim() == 1:
        boxes2 = boxes2.unsqueeze(0)
    if box_format == "center":
        x1, y1 = boxes1[..., 0] - boxes1[..., 2] / 2, boxes1[..., 1] - boxes1[..., 3] / 2
        x2, y2 = boxes2[..., 0] - boxes2[..., 2] / 2, boxes2[..., 1] - boxes2[..., 3] / 2
    else:
        x1, y1, x2, y2 = boxes1[..., 0], boxes1[..., 1], boxes2[..., 0], boxes2[..., 1]
    w1, h1, w2, h2 = boxes1[..., 2], boxes1[..., 3], boxes2[..., 2], boxes2[..., 3]
    iw = torch.clamp(torch.min(x1 + w1, x2 + w2) - torch.max(x1, x2), min=0)
    ih = torch.clamp(torch.min(y1 + h1, y2 + h2) - torch.max(y1, y2), min=0)
    inter = iw * ih
    return inter / (w1 * h1 + w2 * h2 - inter + 1e-6)


# ------------------------------------------------------------------------------ anchors
STRIDES = (32, 16, 8)


def scaled_anchors(anchors, H, W=None):
    """Anchors in grid cells for an H x W input, (3, 3, 2) fp32: ``anchors[k] * (L / stride_k)`` with L = max(H, W) - an
    H x W canvas behaves like the square canvas of side L with its padding cropped away. For H == W this is
    the reference's ``torch.tensor(config.ANCHORS) * S`` (train.py:195-197) bit for bit."""
    W = H if W is None else W
    L_ = max(int(H), int(W))
    if L_ % 32:
        raise ValueError(f"H and W must be multiples of 32, got {H} x {W}")
    grids = torch.tensor([L_ // s for s in STRIDES]).view(3, 1, 1)
    return torch.as_tensor(anchors, dtype=torch.float32).reshape(3, 3, 2) * grids


def _grid_hw(grid_size):
    """None | g | (gh, gw) -> None | (gh, gw)."""
    if grid_size is None:
        return None
    if isinstance(grid_size, (tuple, list)):
        gh, gw = grid_size
        return int(gh), int(gw)
    return int(grid_size), int(grid_size)


# ------------------------------------------------------------------------------ anchors of a dataset
AnchorResult = collections.namedtuple("AnchorResult", "anchors centroids fitness iterations converged picks best")
AnchorFitness = collections.namedtuple("AnchorFitness", "mean_iou recall counts labels")
ANCHOR_MAX_K, ANCHOR_MAX_RESTARTS = 16, 64


def anchor_draws(restarts, k, generator=None):
    """The random draws of :func:`kmeans_anchors` as a (restarts, k) float64 table in [0, 1): row r seeds restart r (k-means++, one
    draw per seed). The same generator state gives the same table, as for :func:`augment_params`."""
    return torch.rand((int(restarts), int(k)), generator=generator, dtype=torch.float64)


def anchors_layout(centroids):
    """k (w, h) pairs -> the ``config.ANCHORS`` layout: sorted ascending by fp32 area ``w * h`` (stable: equal areas keep their input
    order), then, for k % 3 == 0, cut into three groups of k / 3 with the group of the largest anchors (the coarsest grid) first
    and areas ascending inside each group, shape (3, k / 3, 2); any other k stays (k, 2), ascending. Pure tensor code, any device."""
    c = torch.as_tensor(centroids, dtype=torch.float32).reshape(-1, 2)
    s = c[torch.sort(c[:, 0] * c[:, 1], stable=True).indices]
    k = s.shape[0]
    return s.reshape(3, k // 3, 2).flip(0).contiguous() if k and k % 3 == 0 else s


def _anchor_wh(boxes, image_size):
    """(N, 2) wh | (N, >= 4) [x, y, w, h, ...] | per-image lists of [x, y, w, h, ...] rows (None / empty entries allowed) -> the valid
    sizes as a contiguous (M, 2) fp32 tensor on the input's device: rows whose w or h is NaN, <= 0 or > 1 are dropped, the rest is
    multiplied in fp32 by (W / L, H / L), L = max(H, W), when ``image_size = (H, W)`` is given (the factors of build_targets)."""
    first = next((b for b in boxes if b is not None and len(b)), None) if isinstance(boxes, (list, tuple)) else None
    if isinstance(boxes, (list, tuple)) and (any(b is None for b in boxes) or (first is not None and torch.as_tensor(first).dim() >= 2)):
        per =[torch.as_tensor(b, dtype=torch.float32) for b in boxes if b is not None and len(b)]
        per = [b.reshape(-1, b.shape[-1]) for b in per]
        t = torch.cat(per) if per else torch.zeros((0, 4), dtype=torch.float32)
    else:
        t = torch.as_tensor(boxes, dtype=torch.float32)
        if t.numel() == 0:
            t = t.reshape(0, 2)
    if t.dim() != 2 or not (t.shape[1] == 2 or t.shape[1] >= 4):
        raise ValueError(f"boxes must be (N, 2) sizes or (N, >= 4) [x, y, w, h, ...] rows, got {tuple(t.shape)}")
    wh = t if t.shape[1] == 2 else t[:, 2:4]
    w, h = wh[:, 0], wh[:, 1]
    wh = wh[(w > 0) & (w <= 1) & (h > 0) & (h <= 1)]
    if image_size is not None:
        H, W = _grid_hw(image_size)
        L_ = max(H, W)
        wh = wh * torch.tensor([W / L_, H / L_], dtype=torch.float32, device=wh.device)
    return wh.contiguous()


def kmeans_anchors(boxes, k=9, restarts=8, max_iter=300, image_size=None, generator=None, draws=None, device=None):
    """The anchors of a dataset: k-means under the distance 1 - IoU(w, h) with k-means++ seeding, ``restarts`` seedings side by side
    on the device, the best one kept (``yolo_anchor_kmeans``; the arithmetic is stated in include/yolo_mi355x.h). The IoU is the one
    :func:`build_targets` ranks the anchors of a box by.

    ``boxes``: an (N, 2) array of normalised (w, h), an (N, >= 4) array of ``[x, y, w, h, ...]`` rows, or the per-image list that
    :func:`train_batch` takes. Rows whose w or h is NaN, <= 0 or > 1 are dropped; fewer than ``k`` left is a ``ValueError``.
    ``image_size=(H, W)``: the sizes are first multiplied in fp32 by (W / L, H / L), L = max(H, W), as :func:`build_targets` does on
    that canvas, so the anchors come out L-normalised and go straight into ``scaled_anchors(anchors, H, W)``. ``draws``: the
    (restarts, k) table of :func:`anchor_draws` (drawn from ``generator`` when omitted). 1 <= k <= 16, 1 <= restarts <= 64.

    Returns an ``AnchorResult`` of CPU tensors, read back in one copy (the only host synchronisation, apart from the row filter
    when ``boxes`` is itself a device tensor): ``anchors`` - the centroids of the best restart in the ``config.ANCHORS`` layout
    (:func:`anchors_layout`); ``centroids`` (R, k, 2) fp32 in seed order; ``fitness`` (R,) fp64, the mean over the boxes of the best
    IoU; ``iterations`` / ``converged`` (R,) int32 (``max_iter`` Lloyd steps are enqueued, a converged restart leaves them at
    once); ``picks`` (R, k) int32, the rows (of the filtered boxes) taken as seeds; ``best``, the restart with the highest
    fitness, ties to the lowest index."""
    k, R, max_iter = int(k), int(restarts), int(max_iter)
    if not (1 <= k <= ANCHOR_MAX_K and 1 <= R <= ANCHOR_MAX_RESTARTS and max_iter >= 1):
        raise ValueError(f"need 1 <= k <= {ANCHOR_MAX_K}, 1 <= restarts <= {ANCHOR_MAX_RESTARTS}, max_iter >= 1; got {k}, {R}, {max_iter}")
    wh = _anchor_wh(boxes, image_size)
    n = int(wh.shape[0])
    if n < k:
        raise ValueError(f"{n} valid boxes (0 < w, h <= 1) are fewer than k = {k}")
    if draws is None:
        draws = anchor_draws(R, k, generator)
    draws = torch.as_tensor(draws, dtype=torch.float64)
    if tuple(draws.shape) != (R, k) or not bool(((draws >= 0) & (draws < 1)).all()):
        raise ValueError(f"draws must be a ({R}, {k}) table of numbers in [0, 1)")
    dev = torch.device(device) if device is not None else (wh.device if wh.is_cuda else torch.device("cuda"))
    if dev.type != "cuda":
        raise RuntimeError("kmeans_anchors runs on MI355X only (no CPU fallback)")
    lib = L.lib()
    with torch.cuda.device(dev):
        wh, dd = wh.to(dev), draws.to(dev).contiguous()
        # one buffer for every result, 8-byte sections: fitness f64 [R] | centroids f32 [R k 2] | iterations, converged i32 [R] each | picks i32 [R k]
        out = torch.empty(16 * R + 12 * R * k, dtype=torch.uint8, device=dev)
        fit, cen, itc, pk = out[:8 * R], out[8 * R:8 * R + 8 * R * k], out[8 * R + 8 * R * k:16 * R + 8 * R * k], out[16 * R + 8 * R * k:]
        ws = torch.empty(int(lib.yolo_anchor_kmeans_workspace_bytes(n, k, R)), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_anchor_kmeans(wh.data_ptr(), n, k, R, dd.data_ptr(), max_iter, cen.data_ptr(), fit.data_ptr(), itc.data_ptr(),
                                       itc.data_ptr() + 4 * R, pk.data_ptr(), ws.data_ptr(), ws.numel(), L.current_stream()),
                "yolo_anchor_kmeans")
        host = out.cpu()                                            # the one read-back
    fitness = host[:8 * R].view(torch.float64).clone()
    centroids = host[8 * R:8 * R + 8 * R * k].view(torch.float32).reshape(R, k, 2).clone()
    ic = host[8 * R + 8 * R * k:16 * R + 8 * R * k].view(torch.int32).clone()
    picks = host[16 * R + 8 * R * k:16 * R + 12 * R * k].view(torch.int32).reshape(R, k).clone()
    fl = fitness.tolist()
    best = max(range(R), key=lambda r: (fl[r], -r))
    return AnchorResult(anchors_layout(centroids[best]), centroids, fitness, ic[:R], ic[R:], picks, best)


def anchor_fitness(boxes, anchors, iou_threshold=0.5, image_size=None):
    """How well any anchors fit a set of boxes (``yolo_anchor_fitness``), for instance the COCO anchors on the tiles of a new dataset.
    ``boxes`` and ``image_size`` as for :func:`kmeans_anchors` (same filter, same factors); ``anchors``: up to 16 (w, h) pairs in
    any shape, normalised as the boxes are after ``image_size``. Returns an ``AnchorFitness``: ``mean_iou``, the mean over the
    boxes of the best IoU (the fitness of :func:`kmeans_anchors`), ``recall``, the share of boxes whose best IoU is
    ``> iou_threshold`` (both Python floats), ``counts`` (k,) int32, the boxes every anchor wins (the first maximum), and ``labels``
    (N,) int32, the winning anchor per valid box, in the flattened order of ``anchors``; CPU tensors, one read-back."""
    wh = _anchor_wh(boxes, image_size)
    n = int(wh.shape[0])
    if n < 1:
        raise ValueError("no valid box (0 < w, h <= 1)")
    anc = torch.as_tensor(anchors, dtype=torch.float32).reshape(-1, 2)
    k = int(anc.shape[0])
    if not 1 <= k <= ANCHOR_MAX_K:
        raise ValueError(f"need 1 <= k <= {ANCHOR_MAX_K} anchors, got {k}")
    dev = wh.device if wh.is_cuda else torch.device("cuda")
    lib = L.lib()
    with torch.cuda.device(dev):
        wh, anc = wh.to(dev), anc.to(dev).contiguous()
        out = torch.empty(16 + 4 * k + 4 * n, dtype=torch.uint8, device=dev)          # mean, recall f64 | counts i32 [k] | labels i32 [n]
        ws = torch.empty(int(lib.yolo_anchor_fitness_workspace_bytes(n, k)), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_anchor_fitness(wh.data_ptr(), n, anc.data_ptr(), k, float(iou_threshold), out.data_ptr(), out.data_ptr() + 16,
                                        out.data_ptr() + 16 + 4 * k, ws.data_ptr(), ws.numel(), L.current_stream()), "yolo_anchor_fitness")
        host = out.cpu()
    mr = host[:16].view(torch.float64).tolist()
    ints = host[16:].view(torch.int32).clone()
    return AnchorFitness(mr[0], mr[1], ints[:k], ints[k:])


# ------------------------------------------------------------------------------ decode
def decode_boxes(predictions, anchors, grid_size=None, is_pred=True, out=None, box_offset=0, mutate=True):
    """Device decode of one scale: (B,3,gh,gw,5+nc) -> (B, 3*gh*gw, 6) fp32 tensor
    [cx,cy,w,h,obj,cls] normalised to [0,1]; mutates ``predictions[...,0:4]`` in place when
    ``is_pred`` exactly like the reference (utils.py:106-110) unless ``mutate=False``. ``out`` / ``box_offset`` let
    several scales share one (B, N_total, 6) buffer. ``grid_size``: None (taken from the tensor), g or (gh, gw); x and w
    are normalised by gw, y and h by gh."""
    if not predictions.is_cuda:
        raise RuntimeError("decode_boxes runs on MI355X only (no CPU fallback)")
    if predictions.dtype in (torch.float16, torch.bfloat16):
        # heads handed out under autocast: decode an fp32 copy and write the in-place side effect (utils.py:106-110) back
        p32 = predictions.float()
        res = decode_boxes(p32, anchors, grid_size, is_pred, out, box_offset, mutate)
        if is_pred and mutate:
            predictions[..., 0:4] = p32[..., 0:4].to(predictions.dtype)
        return res
    if predictions.dtype != torch.float32:
        raise NotImplementedError("decode_boxes: floating-point predictions only")
    B, A, gh, gw, D = predictions.shape
    if A != 3 or (grid_size is not None and _grid_hw(grid_size) != (gh, gw)):
        raise ValueError(f"bad prediction shape {tuple(predictions.shape)} for grid {grid_size}")
    n = 3 * gh * gw
    if out is None:
        out = torch.empty((B, n, 6), dtype=torch.float32, device=predictions.device)
        box_offset = 0
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape[0] != B or out.shape[2] != 6:
        raise ValueError("out must be a contiguous (B, N, 6) fp32 tensor")
    anc = torch.as_tensor(anchors, dtype=torch.float32, device=predictions.device).reshape(3, 2).contiguous() \
        if is_pred else None
    strides = (C.c_int64 * 5)(*predictions.stride())
    with torch.cuda.device(predictions.device):
        L.check(L.lib().yolo_decode_hw(predictions.data_ptr(), strides, L.ptr(anc), B, gh, gw, D - 5,
                                       (1 if mutate else 2) if is_pred else 0, out.data_ptr(), out.shape[1], int(box_offset),
                                       L.current_stream()), "yolo_decode")
    return out


def cells_to_boxes(predictions, anchors, grid_size, is_pred=True):
    """Reference signature (utils.py:86-148): returns ``list[B][3*gh*gw][6]``; ``grid_size`` is g or (gh, gw)."""
    return decode_boxes(predictions, anchors, grid_size, is_pred).tolist()


# --------------------------------------------------------------------------------- NMS
_ws_cache = {}


def _workspace(nbytes, device):
    key = device.index
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws_cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def nms_indices(boxes, iou_threshold, obj_threshold, box_format="corners"):
    """Batched device NMS. ``boxes``: (B, N, 6) or (N, 6) fp32 CUDA tensor of
    [x,y,w,h,obj,cls]. Returns (keep_idx (B,N) int32, keep_count (B,) int32): for image b the
    first keep_count[b] entries index its input rows in the reference's output order."""
    if not boxes.is_cuda:
        raise RuntimeError("nms_indices runs on MI355X only (no CPU fallback)")
    single = boxes.dim() == 2
    if single:
        boxes = boxes.unsqueeze(0)
    if boxes.dim() != 3 or boxes.shape[-1] != 6:
        raise ValueError("boxes must be (B, N, 6)")
    boxes = boxes.float().contiguous()
    B, N, _ = boxes.shape
    keep = torch.empty((B, max(N, 1)), dtype=torch.int32, device=boxes.device)
    count = torch.empty((B,), dtype=torch.int32, device=boxes.device)
    lib = L.lib()
    with torch.cuda.device(boxes.device):
        nbytes = lib.yolo_nms_workspace_bytes(B, N)
        ws = _workspace(max(nbytes, 256), boxes.device)
        L.check(lib.yolo_nms(boxes.data_ptr(), B, N, float(iou_threshold), float(obj_threshold),
                             int(box_format == "center"), keep.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                             L.current_stream()), "yolo_nms")
    if single:
        return keep[0], count[0]
    return keep, count


def non_max_suppression(boxes, iou_threshold, obj_threshold, box_format="corners"):
    """Reference signature (utils.py:150-191): list of [x,y,w,h,obj,cls] lists in, kept boxes
    out (objectness-descending). The list is shipped to the GPU, suppressed there, and the kept
    rows are returned as Python lists of the same fp32 values the reference would produce."""
    if len(boxes) == 0:
        return []
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 6).to(dev)
    keep, count = nms_indices(t, iou_threshold, obj_threshold, box_format)
    k = int(count.item())
    return t[keep[:k].long()].tolist() if k else []


def detect(predictions, scaled_anchors, iou_threshold=0.45, obj_threshold=0.5, box_format="center", mutate=False):
    """Fused post-processing of a forward pass (the sequence of demo.py:44-55 /
    utils.py:300-321, all images at once, nothing leaves HBM):
    decode three scales into one (B, N, 6) buffer in the reference's concatenation order
    (scale 0, 1, 2), then per-image NMS. Returns (boxes (B,N,6), keep_idx (B,N), keep_count (B,)).
    ``mutate=True`` also performs the in-place sigmoid / exp write-back ``cells_to_boxes`` does to the prediction tensors
    (utils.py:106-110); the reference's callers of this sequence never read them again, so the default leaves them alone."""
    B = predictions[0].shape[0]
    n_per = [3 * p.shape[2] * p.shape[3] for p in predictions]
    total = sum(n_per)
    dev = predictions[0].device
    boxes = torch.empty((B, total, 6), dtype=torch.float32, device=dev)
    if len(predictions) == 3 and all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 5 for p in predictions) \
            and len({p.shape[4] for p in predictions}) == 1:
        with torch.cuda.device(dev):                      # the three scales in one launch
            anc = [torch.as_tensor(a, dtype=torch.float32).reshape(3, 2).to(dev).contiguous() for a in scaled_anchors]
            pp = (C.c_void_p * 3)(*[p.data_ptr() for p in predictions])
            st = (C.c_int64 * 15)(*[v for p in predictions for v in p.stride()])
            ap = (C.c_void_p * 3)(*[a.data_ptr() for a in anc])
            gg = (C.c_int * 6)(*[v for p in predictions for v in (p.shape[2], p.shape[3])])      # (gh, gw) per scale
            L.check(L.lib().yolo_decode3_hw(pp, st, ap, gg, B, predictions[0].shape[4] - 5, int(bool(mutate)), boxes.data_ptr(), total,
                                            L.current_stream()), "yolo_decode3")
    else:
        off = 0
        for p, a, n in zip(predictions, scaled_anchors, n_per):
            decode_boxes(p, a, (p.shape[2], p.shape[3]), True, out=boxes, box_offset=off, mutate=mutate)
            off += n
    keep, count = nms_indices(boxes, iou_threshold, obj_threshold, box_format)
    return boxes, keep, count


def detect_images(model, x, scaled_anchors, iou_threshold=0.45, obj_threshold=0.5, box_format="center"):
    """``detect(model(x), ...)`` with ONE host synchronisation instead of two back to back: the forward's NaN guards
    (model.py:175,183-184) are read after decode and NMS have been enqueued, so the GPU does not sit idle between the
    forward and the post-processing while the host wakes up and launches them (~0.1-0.25 ms per batch). Same results, same
    exceptions (``AssertionError`` for a NaN input, ``ValueError("Nan in layer")``), raised before anything is returned."""
    eng = model._engine
    eng._defer_nan, eng._pending_flag = True, None
    try:
        with torch.no_grad():
            preds = model(x)
        flag = eng._pending_flag
    finally:
        eng._defer_nan, eng._pending_flag = False, None
    out = detect(preds, scaled_anchors, iou_threshold, obj_threshold, box_format)
    if flag is not None:
        eng.raise_on_nan(flag)
    return out


# ------------------------------------------------------------------------------ tiled detection
def _tile_hw(tile):
    th, tw = _grid_hw(tile)
    if th <= 0 or tw <= 0 or th % 32 or tw % 32:
        raise ValueError(f"tile sides must be positive multiples of 32, got {th} x {tw}")
    return th, tw


def _overlap_px(overlap, th, tw):
    """fraction | pixels | (per axis) -> (oh, ow) pixels: an int is a pixel count, anything else a fraction of the tile side."""
    oh, ow = overlap if isinstance(overlap, (tuple, list)) else (overlap, overlap)

    def px(o, t):
        return int(o) if isinstance(o, int) and not isinstance(o, bool) else int(round(float(o) * t))
    oh, ow = px(oh, th), px(ow, tw)
    if not (0 <= oh < th and 0 <= ow < tw):
        raise ValueError(f"overlap must satisfy 0 <= overlap < tile, got {oh} of {th}, {ow} of {tw} pixels")
    return oh, ow


def _tile_origins(h, w, th, tw, oh, ow):
    """yolo_tile_grid: the flat [y0, x0, y0, x0, ...] list of one image's tiles in row-major order."""
    lib = L.lib()
    n = lib.yolo_tile_grid(h, w, th, tw, oh, ow, None, 0)
    L.check(min(n, 0), "yolo_tile_grid")
    buf = (C.c_int32 * (2 * n))()
    L.check(min(lib.yolo_tile_grid(h, w, th, tw, oh, ow, buf, n), 0), "yolo_tile_grid")
    return list(buf)


def tile_grid(h, w, tile=416, overlap=0.2):
    """Origins of the overlapping tiles an h x w image is cut into, an int32 (T, 2) tensor of [y0, x0] rows in row-major tile
    order (``yolo_tile_grid``). ``tile``: t or (th, tw), any size. ``overlap``: a fraction of the tile side (``int(round(overlap *
    t))`` pixels per axis), or pixels when given as int(s); a pair is (rows, columns). Per axis the stride is t - overlap; an axis
    that is no longer than the tile has one tile at 0 (zero-padded), otherwise the last tile is flush with the edge."""
    th, tw = _grid_hw(tile)
    oh, ow = _overlap_px(overlap, th, tw)
    return torch.tensor(_tile_origins(int(h), int(w), th, tw, oh, ow), dtype=torch.int32).reshape(-1, 2)


def _scales(scales):
    """A non-empty sequence of distinct finite floats in (0, 8] -> list of float."""
    try:
        if isinstance(scales, (str, bytes)) or any(isinstance(v, (bool, str, bytes)) for v in scales):
            raise TypeError
        out = [float(v) for v in scales]
    except (TypeError, ValueError):
        raise ValueError(f"scales must be a non-empty sequence of numbers, got {scales!r}") from None
    if not out or not all(math.isfinite(v) and 0.0 < v <= 8.0 for v in out):
        raise ValueError(f"scales must be a non-empty sequence of finite numbers in (0, 8], got {scales!r}")
    if len(set(out)) != len(out):
        raise ValueError(f"scales must not repeat a level, got {scales!r}")
    return out


def _level_hw(h, w, scale):
    """yolo_tile_level_hw: (max(1, rint(h scale)), max(1, rint(w scale))), half to even."""
    lh, lw = C.c_int(), C.c_int()
    L.check(L.lib().yolo_tile_level_hw(int(h), int(w), float(scale), C.byref(lh), C.byref(lw)), "yolo_tile_level_hw")
    return lh.value, lw.value


def tile_pyramid(h, w, tile=416, overlap=0.2, scales=(1.0,)):
    """The levels :func:`detect_tiled` cuts an h x w image into: a list with one ``((lh, lw), origins)`` entry per scale, in the
    order given. ``(lh, lw)`` is the size of the image resized by that scale (``yolo_tile_level_hw``: ``max(1, rint(h * scale))``,
    half to even; scale 1.0 is the image itself) and ``origins`` is ``tile_grid(lh, lw, tile, overlap)``, in pixels of the level.
    ``scales``: distinct finite numbers in (0, 8]."""
    out = []
    for sc in _scales(scales):
        lh, lw = _level_hw(h, w, sc)
        out.append(((lh, lw), tile_grid(lh, lw, tile, overlap)))
    return out


def detect_tiled(model, images, scaled_anchors, tile=416, overlap=0.2, iou_threshold=0.45, obj_threshold=0.5, box_format="center",
                 batch=32, max_candidates=65536, scales=(1.0,), edge_margin=None):
    """Detection on frames that are larger than the network input: every frame is cut into overlapping tiles
    (:func:`tile_grid`), the tiles of all frames run through ``model(x)`` in chunks of ``batch``, the decoded boxes
    above ``obj_threshold`` are mapped back to their frame and compacted on the device (``yolo_tile_collect``), and one
    per-class NMS per frame merges the duplicates along the seams. ``images``: one uint8 (H, W, 3) tensor / array or a list of
    them (any sizes; on the host or already on the device). ``scaled_anchors``: for the TILE size, as for
    :func:`detect_images` (``scaled_anchors(anchors, th, tw)``), whatever the level.

    ``scales``: the pyramid (:func:`tile_pyramid`), distinct finite numbers in (0, 8]. Every frame is tiled once per scale, on
    the frame resized by it (``max(1, rint(side * scale))`` per side, half to even; the library's one uint8 INTER_LINEAR, sampled
    by the gather, no resized frame is stored; a scale below 0.5 skips source pixels as :func:`letterbox` does), so an object
    that no native tile sees whole is seen whole by a coarser level; the levels meet in the one NMS. The default ``(1.0,)`` is
    native resolution only. A level that is no larger than the tile is a single zero-padded tile: with tile 416 a 5472 x 3648
    frame is one at scale 416 / 5472 = 0.076 or below, and ``(1.0, 0.5, 0.25)`` ends at 1368 x 912, 4 x 3 tiles (187 + 48 + 12 tiles per frame).
    ``edge_margin``: ``None`` (off) or pixels of the tile, >= 0. On, a box that reaches within ``edge_margin`` of a side of its
    tile is dropped before the NMS when that side is interior, i.e. not on the level's border (``yolo_tile_collect_ex``): it is
    the truncated copy of an object that a neighbouring tile or a coarser level reports whole, and its IoU with the whole box
    is too low for the NMS to remove it. An object is lost if every tile of every level cuts it, so use it with an overlap
    larger than the objects of the finest level or with a coarser level.

    Returns ``(boxes (F, max_candidates, 6), keep (F, max_candidates) int32, count (F,) int32, candidates (F,) int32)``:
    ``boxes[f, :candidates[f]]`` are frame f's candidates ``[cx, cy, w, h, obj, cls]`` normalised to that frame, in (level, tile,
    row) order with the levels in the order of ``scales`` (the order :func:`nms_indices` breaks score ties by), zero rows behind
    them; ``keep`` / ``count`` index them as from :func:`nms_indices`. ``max_candidates`` counts a frame's candidates over all its
    levels. The tiles are in (frame, level, tile) order and a chunk runs across levels and frames. Everything is stream-ordered
    with ONE host synchronisation, which reads ``candidates`` and the forwards' NaN flags together; the forward's exceptions are
    raised as by :func:`detect_images`, and a frame with more than ``max_candidates`` candidates raises ``ValueError``.
    A last chunk shorter than ``batch`` runs at its own size (a second plan of the model, at most two per call).
    ``fuse_boxes(boxes, ..., class_agnostic=...)`` on the returned candidates is the fusing (weighted box fusion instead of the
    NMS's one winner per object) and the class-agnostic merge.
    Not built: area-filtered downscaling; merging the two halves of a box across a seam."""
    th, tw = _tile_hw(tile)
    oh, ow = _overlap_px(overlap, th, tw)
    if not float(obj_threshold) >= 0:
        raise ValueError(f"obj_threshold must be >= 0 (the zero rows behind the candidates must not pass it), got {obj_threshold}")
    batch, cap = int(batch), int(max_candidates)
    if batch < 1 or cap < 1:
        raise ValueError(f"batch and max_candidates must be >= 1, got {batch} and {cap}")
    scales = _scales(scales)
    if edge_margin is not None:
        try:
            margin = float(edge_margin)
        except (TypeError, ValueError):
            margin = math.nan
        if isinstance(edge_margin, bool) or not (math.isfinite(margin) and margin >= 0):
            raise ValueError(f"edge_margin must be None or a finite number >= 0 (pixels of the tile), got {edge_margin!r}")
    plain = scales == [1.0] and edge_margin is None             # today's launches: yolo_tile_gather, yolo_tile_collect
    if isinstance(images, torch.Tensor) and images.dim() == 3 or not isinstance(images, (list, tuple)):
        images = [images]
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
            raise ValueError("images must be uint8 (H, W, 3)")
        ts.append(t)
    if not ts:
        raise ValueError("detect_tiled needs at least one image")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("detect_tiled runs on MI355X only (no CPU fallback)")
    F = len(ts)
    lib = L.lib()
    # host tables: per tile [y0, x0] (gather) and {image, y0, x0, level} (collect), per image [H, W], per level [H, W].
    # A level is one (frame, scale) pair, numbered f * len(scales) + k; runs[r] = (first tile, frame, level H, level W).
    origins, tiles, runs, lev = [], [], [], []
    for f, t in enumerate(ts):
        for sc in scales:
            lh, lw = _level_hw(t.shape[0], t.shape[1], sc)
            o = _tile_origins(lh, lw, th, tw, oh, ow)
            runs.append((len(origins) // 2, f, lh, lw))
            origins += o
            for k in range(0, len(o), 2):
                tiles += [f, o[k], o[k + 1], 0 if plain else len(lev) // 2]   # yolo_tile_collect's spare field stays 0
            lev += [lh, lw]
    T = len(origins) // 2
    runs.append((T, F, 0, 0))
    hw = [int(v) for t in ts for v in t.shape[:2]]
    if plain:
        lev = []
    host = _pinned(6 * T + 2 * F + len(lev), torch.int32)
    host.copy_(torch.tensor(origins + tiles + hw + lev, dtype=torch.int32))
    anc = [torch.as_tensor(a, dtype=torch.float32).reshape(3, 2) for a in scaled_anchors]
    if any(a.device != dev for a in anc):
        anc_host = _pinned(18, torch.float32)
        anc_host.copy_(torch.cat([a.cpu().reshape(-1) for a in anc]))
    chunks = [(s, min(batch, T - s)) for s in range(0, T, batch)]
    eng = model._engine
    with torch.cuda.device(dev):
        stream = L.current_stream()
        tab = host.to(dev, non_blocking=True)
        d_origins, d_tiles, d_hw, d_lev = tab[:2 * T], tab[2 * T:6 * T], tab[6 * T:6 * T + 2 * F], tab[6 * T + 2 * F:]
        if any(a.device != dev for a in anc):
            anc = list(anc_host.to(dev, non_blocking=True).reshape(3, 3, 2))
        anc = [a.contiguous() for a in anc]
        frames = []
        for t in ts:
            if t.device.type != "cuda":
                staged = _pinned(t.numel(), torch.uint8)
                staged.copy_(t.reshape(-1))
                t = staged.to(dev, non_blocking=True)
            frames.append(t.to(dev).contiguous())
        cand = torch.empty((F, cap, 6), dtype=torch.float32, device=dev)
        tail = torch.empty(F + len(chunks), dtype=torch.int32, device=dev)       # candidates per image | NaN flag per chunk
        L.check(lib.yolo_fill_zero(cand.data_ptr(), cand.numel() * 4, stream), "yolo_fill_zero")
        L.check(lib.yolo_fill_zero(tail.data_ptr(), tail.numel() * 4, stream), "yolo_fill_zero")
        x = torch.empty((min(batch, T), 3, th, tw), dtype=torch.float32, device=dev)
        boxes = ws = None
        eng._defer_nan, eng._pending_flag = True, None
        try:
            for c, (s, n) in enumerate(chunks):
                r = max(k for k in range(len(runs) - 1) if runs[k][0] <= s)
                while runs[r][0] < s + n:                           # one gather per (frame, level) that has tiles in this chunk
                    a, b = max(runs[r][0], s), min(runs[r + 1][0], s + n)
                    f, lh, lw = runs[r][1:]
                    if b > a and (lh, lw) == (hw[2 * f], hw[2 * f + 1]):
                        L.check(lib.yolo_tile_gather(frames[f].data_ptr(), hw[2 * f], hw[2 * f + 1], d_origins.data_ptr() + 8 * a, b - a,
                                                     th, tw, x.data_ptr() + 4 * (a - s) * 3 * th * tw, stream), "yolo_tile_gather")
                    elif b > a:
                        L.check(lib.yolo_tile_gather_scaled(frames[f].data_ptr(), hw[2 * f], hw[2 * f + 1], lh, lw,
                                                            d_origins.data_ptr() + 8 * a, b - a, th, tw,
                                                            x.data_ptr() + 4 * (a - s) * 3 * th * tw, stream), "yolo_tile_gather_scaled")
                    r += 1
                eng._pending_flag = None
                with torch.no_grad():
                    preds = model(x[:n])
                if eng._pending_flag is not None:
                    L.check(lib.yolo_copy_d2d(tail.data_ptr() + 4 * (F + c), eng._pending_flag.data_ptr(), 4, stream), "nan flag copy")
                preds = [p if p.dtype == torch.float32 else p.float() for p in preds]
                n_per = sum(3 * p.shape[2] * p.shape[3] for p in preds)
                if boxes is None:
                    boxes = torch.empty((x.shape[0], n_per, 6), dtype=torch.float32, device=dev)
                    ws = _workspace(max(int(lib.yolo_tile_collect_workspace_bytes(x.shape[0], n_per)), 256), dev)
                pp = (C.c_void_p * 3)(*[p.data_ptr() for p in preds])
                st = (C.c_int64 * 15)(*[v for p in preds for v in p.stride()])
                ap = (C.c_void_p * 3)(*[a.data_ptr() for a in anc])
                gg = (C.c_int * 6)(*[v for p in preds for v in (p.shape[2], p.shape[3])])
                L.check(lib.yolo_decode3_hw(pp, st, ap, gg, n, preds[0].shape[4] - 5, 0, boxes.data_ptr(), n_per, stream), "yolo_decode3")
                if plain:
                    L.check(lib.yolo_tile_collect(boxes.data_ptr(), n, n_per, d_tiles.data_ptr() + 16 * s, d_hw.data_ptr(), F, th, tw,
                                                  float(obj_threshold), cand.data_ptr(), cap, tail.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  stream), "yolo_tile_collect")
                else:
                    L.check(lib.yolo_tile_collect_ex(boxes.data_ptr(), n, n_per, d_tiles.data_ptr() + 16 * s, d_lev.data_ptr(),
                                                     len(lev) // 2, F, th, tw, float(obj_threshold),
                                                     -1.0 if edge_margin is None else margin, cand.data_ptr(), cap,
                                                     tail.data_ptr(), ws.data_ptr(), ws.numel(), stream), "yolo_tile_collect_ex")
        finally:
            eng._defer_nan, eng._pending_flag = False, None
        for t in frames:
            t.record_stream(torch.cuda.current_stream())
        keep, count = nms_indices(cand, iou_threshold, obj_threshold, box_format)
        tail_host = tail.tolist()                                   # the one host synchronisation
    flag = 0
    for v in tail_host[F:]:
        flag |= v
    eng._raise_flag(flag)
    for f in range(F):
        if tail_host[f] > cap:
            raise ValueError(f"image {f} has {tail_host[f]} candidates above obj_threshold {obj_threshold}, max_candidates is {cap}")
    return cand, keep, count, tail[:F]


# ------------------------------------------------------------------------------ box fusion and test-time augmentation
_CONF_TYPES = {"avg": 0, "max": 1}
_FLIPS = {"none": (0, 0), "lr": (1, 0), "ud": (0, 1), "lrud": (1, 1)}


def fuse_boxes(boxes, iou_threshold=0.55, obj_threshold=0.0, box_format="center", n_views=0, conf_type="avg", class_agnostic=False,
               return_assign=False):
    """Weighted box fusion on the device (``yolo_fuse_boxes``; the arithmetic is defined to the bit in DESIGN.md 7.20). ``boxes``:
    (B, N, 6) or (N, 6) fp32 CUDA tensor of [x, y, w, h, obj, cls] rows, e.g. the candidates of :func:`tta_boxes` or
    :func:`detect_tiled`. The rows above ``obj_threshold`` are walked in descending score; each joins the cluster of its class
    (of any class with ``class_agnostic``) whose fused box it overlaps most with IoU > ``iou_threshold``, or founds one; a
    cluster's box is the score-weighted mean of its members' corners. ``conf_type``: "avg" (mean member score) or "max" (the
    founder's); with ``n_views`` > 0 the score is scaled by ``min(members, n_views) / n_views``, so an object that only some views
    report ranks lower. Returns ``(fused (B, N, 6), count (B,) int32, members (B, N) int32)``: the first ``count[b]`` rows of
    image b are its clusters, best score first, zero rows behind them (so the result can go to :func:`nms_indices`,
    :func:`evaluate_detections` or another fusion); with ``return_assign`` also ``assign (B, N) int32``, the fused row every input
    row joined (-1: below the threshold). No host synchronisation."""
    if not isinstance(boxes, torch.Tensor):
        raise ValueError("boxes must be a tensor")
    single = boxes.dim() == 2
    if single:
        boxes = boxes.unsqueeze(0)
    if boxes.dim() != 3 or boxes.shape[-1] != 6 or boxes.shape[0] < 1 or not boxes.is_floating_point():
        raise ValueError("boxes must be a floating-point (B, N, 6) or (N, 6) tensor")
    iou_threshold, obj_threshold = float(iou_threshold), float(obj_threshold)
    if not 0.0 <= iou_threshold <= 1.0:
        raise ValueError(f"iou_threshold must be in [0, 1], got {iou_threshold}")
    if not obj_threshold >= 0:
        raise ValueError(f"obj_threshold must be >= 0 (zero rows behind a caller's boxes must not pass it), got {obj_threshold}")
    if box_format not in ("center", "corners"):
        raise ValueError(f"box_format must be 'center' or 'corners', got {box_format!r}")
    if conf_type not in _CONF_TYPES:
        raise ValueError(f"conf_type must be 'avg' or 'max', got {conf_type!r}")
    if isinstance(n_views, bool) or int(n_views) != n_views or n_views < 0:
        raise ValueError(f"n_views must be an integer >= 0, got {n_views!r}")
    if not boxes.is_cuda:
        raise RuntimeError("fuse_boxes runs on MI355X only (no CPU fallback)")
    boxes = boxes.float().contiguous()
    B, N, _ = boxes.shape
    dev = boxes.device
    lib = L.lib()
    with torch.cuda.device(dev):
        nbytes = lib.yolo_fuse_workspace_bytes(B, N)
        if nbytes == 0:
            raise ValueError(f"fuse_boxes takes at most 2,047 images of 163,456 boxes, got {B} x {N}")
        fused = torch.empty((B, N, 6), dtype=torch.float32, device=dev)
        members = torch.empty((B, N), dtype=torch.int32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        assign = torch.empty((B, N), dtype=torch.int32, device=dev) if return_assign else None
        ws = _workspace(max(nbytes, 256), dev)
        L.check(lib.yolo_fuse_boxes(boxes.data_ptr(), B, N, iou_threshold, obj_threshold, int(box_format == "center"),
                                    int(bool(class_agnostic)), int(n_views), _CONF_TYPES[conf_type], fused.data_ptr(), members.data_ptr(),
                                    count.data_ptr(), L.ptr(assign), ws.data_ptr(), ws.numel(), L.current_stream()), "yolo_fuse_boxes")
    out = (fused, count, members) + ((assign,) if return_assign else ())
    return tuple(t[0] for t in out) if single else out


def tta_views(h, w, flips=("none", "lr"), scales=(1.0,), max_sizes=None):
    """The views of test-time augmentation for an h x w input, host only: ``[(Hv, Wv, flip_lr, flip_ud)]``, scale-major then flip,
    in the order given. ``Hv = 32 * max(1, round(h * s / 32))`` (half to even), ``Wv`` likewise: the network takes multiples of 32.
    ``flips``: names out of "none", "lr", "ud", "lrud"; ``scales``: finite numbers in (0, 4]. Two views that come out equal raise
    ``ValueError``, and so do more distinct sizes than ``max_sizes`` (:func:`tta_boxes` passes the number of eval plans the model
    keeps, so that no view evicts another view's plan)."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f"h and w must be positive, got {h} x {w}")
    if isinstance(flips, (str, bytes)) or isinstance(scales, (str, bytes)):
        raise ValueError("flips and scales must be sequences")
    try:
        flips, scales = list(flips), list(scales)
    except TypeError:
        raise ValueError("flips and scales must be sequences") from None
    if not flips or any(not isinstance(f, str) or f not in _FLIPS for f in flips):
        raise ValueError(f"flips must be a non-empty sequence out of {tuple(_FLIPS)}, got {flips!r}")
    try:
        if any(isinstance(s, (bool, str, bytes)) for s in scales):
            raise TypeError
        scales = [float(s) for s in scales]
    except (TypeError, ValueError):
        raise ValueError(f"scales must be a non-empty sequence of numbers, got {scales!r}") from None
    if not scales or not all(math.isfinite(s) and 0.0 < s <= 4.0 for s in scales):
        raise ValueError(f"scales must be a non-empty sequence of finite numbers in (0, 4], got {scales!r}")
    views = []
    for s in scales:
        hv, wv = 32 * max(1, round(h * s / 32)), 32 * max(1, round(w * s / 32))
        for f in flips:
            v = (hv, wv) + _FLIPS[f]
            if v in views:
                raise ValueError(f"view {v} (scale {s}, flip {f!r}) repeats an earlier view")
            views.append(v)
    sizes = {v[:2] for v in views}
    if max_sizes is not None and len(sizes) > int(max_sizes):
        raise ValueError(f"{len(sizes)} distinct view sizes {sorted(sizes)}, but the model keeps {int(max_sizes)} eval plans")
    return views


def _tta_run(model, x, anchors, flips, scales, post=None):
    """tta_boxes; ``post(boxes)`` is enqueued before the one host synchronisation and its result returned with the boxes."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_floating_point():
        raise ValueError("x must be a floating-point (B, 3, H, W) tensor")
    B, Cc, H, W = x.shape
    eng = model._engine
    views = tta_views(H, W, flips, scales, max_sizes=eng.max_eval_plans)
    if not x.is_cuda:
        raise RuntimeError("tta_boxes runs on MI355X only (no CPU fallback)")
    dev = x.device
    lib = L.lib()
    anc_host = _pinned(18 * len(views), torch.float32)
    anc_host.copy_(torch.cat([scaled_anchors(anchors, hv, wv).reshape(-1) for hv, wv, _, _ in views]))
    n_view = [3 * ((hv // 32) * (wv // 32) + (hv // 16) * (wv // 16) + (hv // 8) * (wv // 8)) for hv, wv, _, _ in views]
    total = sum(n_view)
    with torch.cuda.device(dev):
        stream = L.current_stream()
        anc = anc_host.to(dev, non_blocking=True).reshape(len(views), 3, 3, 2)
        boxes = torch.empty((B, total, 6), dtype=torch.float32, device=dev)
        tail = torch.empty(len(views), dtype=torch.int32, device=dev)            # NaN flag per view
        L.check(lib.yolo_fill_zero(tail.data_ptr(), tail.numel() * 4, stream), "yolo_fill_zero")
        src = None
        eng._defer_nan, eng._pending_flag = True, None
        try:
            off = 0
            for v, (hv, wv, flr, fud) in enumerate(views):
                if (hv, wv, flr, fud) == (H, W, 0, 0):
                    xv = x                                                     # the frame itself: no copy
                else:
                    if src is None:
                        src = x.detach()
                        if src.dtype != torch.float32 or not src.is_contiguous():
                            src = src.float().contiguous()
                    xv = torch.empty((B, Cc, hv, wv), dtype=torch.float32, device=dev)
                    L.check(lib.yolo_tta_view(src.data_ptr(), B, Cc, H, W, xv.data_ptr(), hv, wv, flr, fud, stream), "yolo_tta_view")
                eng._pending_flag = None
                with torch.no_grad():
                    preds = model(xv)
                if eng._pending_flag is not None:
                    L.check(lib.yolo_copy_d2d(tail.data_ptr() + 4 * v, eng._pending_flag.data_ptr(), 4, stream), "nan flag copy")
                preds = [p if p.dtype == torch.float32 else p.float() for p in preds]
                if sum(3 * p.shape[2] * p.shape[3] for p in preds) != n_view[v]:
                    raise ValueError("tta_boxes needs the three heads at strides 32, 16 and 8")
                pp = (C.c_void_p * 3)(*[p.data_ptr() for p in preds])
                st = (C.c_int64 * 15)(*[s for p in preds for s in p.stride()])
                ap = (C.c_void_p * 3)(*[anc[v, k].data_ptr() for k in range(3)])
                gg = (C.c_int * 6)(*[s for p in preds for s in (p.shape[2], p.shape[3])])
                L.check(lib.yolo_decode3_hw_at(pp, st, ap, gg, B, preds[0].shape[4] - 5, 0, boxes.data_ptr(), total, off, stream),
                        "yolo_decode3")
                L.check(lib.yolo_boxes_unflip(boxes.data_ptr(), B, total, off, n_view[v], flr, fud, stream), "yolo_boxes_unflip")
                off += n_view[v]
        finally:
            eng._defer_nan, eng._pending_flag = False, None
        res = post(boxes, len(views)) if post is not None else None
        flags = tail.tolist()                                                  # the one host synchronisation
    flag = 0
    for f in flags:
        flag |= f
    eng._raise_flag(flag)
    return boxes, res


def tta_boxes(model, x, anchors, flips=("none", "lr"), scales=(1.0,)):
    """The decoded boxes of every view of ``x`` in one buffer, mapped back to the frame: ``(B, sum N_v, 6)`` fp32 rows
    [cx, cy, w, h, obj, cls], view v in its own row block in the order of :func:`tta_views`. ``x``: (B, 3, H, W) float on the
    device; ``anchors``: the NORMALISED (3, 3, 2) anchors - every view takes ``scaled_anchors(anchors, Hv, Wv)``. A view is made
    on the device (``yolo_tta_view``: mirrored copy, or bilinear resize with half-pixel centres), run through ``model``, decoded
    straight into its block without the write-back into the predictions, and unmirrored (``yolo_boxes_unflip``); the view
    (1.0, "none") is ``model(x)`` on ``x`` itself. 16-bit heads are cast as in :func:`detect_tiled`. One host synchronisation,
    which reads the forwards' NaN flags; the exceptions of :func:`detect_images` are raised before anything is returned.
    ``nms_indices(tta_boxes(...), ...)`` is NMS over all views; :func:`detect_tta` fuses them instead."""
    return _tta_run(model, x, anchors, flips, scales)[0]


def detect_tta(model, x, anchors, flips=("none", "lr"), scales=(1.0,), iou_threshold=0.55, obj_threshold=0.5, conf_type="avg",
               class_agnostic=False):
    """Test-time augmented detection: :func:`tta_boxes` followed by ``fuse_boxes(..., n_views=len(views))`` on its candidates,
    enqueued before the one host synchronisation. Returns ``(fused, count, members)`` as :func:`fuse_boxes` does. WBF averages:
    it needs several reports per object, which the views provide; on a single view it mostly rescales scores (use
    :func:`detect_images`)."""
    def post(boxes, n_views):
        return fuse_boxes(boxes, iou_threshold, obj_threshold, "center", n_views, conf_type, class_agnostic)
    return _tta_run(model, x, anchors, flips, scales, post)[1]


# ------------------------------------------------------------------------------ targets
def build_targets(boxes, anchors, image_size, counts=None, ignore_iou_threshold=0.5, device=None):
    """Batched device version of the target loop of ``YOLODataset.__getitem__`` (dataset.py:119-161).

    ``boxes``: per-image lists ``[[x, y, w, h, class], ...]`` (normalised, the dataset's order) or a padded
    ``(B, max_boxes, 5)`` tensor with ``counts`` (B). ``anchors``: the 3x3x2 normalised anchor table
    (``config.ANCHORS``). ``image_size``: S or (H, W) (multiples of 32; per-axis grids, see ``yolo_build_targets_hw``).
    Returns the tuple of three ``(B, 3, gh, gw, 6)`` fp32 tensors the loss consumes."""
    if isinstance(boxes, torch.Tensor):
        if counts is None:
            raise ValueError("a padded box tensor needs `counts`")
        bt = boxes.to(dtype=torch.float32)
        dev = bt.device if device is None else torch.device(device)
        ct = torch.as_tensor(counts, dtype=torch.int32)
    else:
        B = len(boxes)
        mb = max(1, max((len(b) for b in boxes), default=1))
        host = torch.zeros((B, mb, 5), dtype=torch.float32)
        ct = torch.tensor([len(b) for b in boxes], dtype=torch.int32)
        for i, bl in enumerate(boxes):
            if len(bl):
                host[i, :len(bl)] = torch.as_tensor(bl, dtype=torch.float32).reshape(-1, 5)
        bt = host
        dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("build_targets runs on MI355X only (no CPU fallback)")
    bt = bt.to(dev).contiguous()
    ct = ct.to(dev).contiguous()
    anc = torch.as_tensor(anchors, dtype=torch.float32).reshape(9, 2).to(dev).contiguous()
    B, mb = bt.shape[0], bt.shape[1]
    H, W = _grid_hw(image_size)
    with torch.cuda.device(dev):
        outs = [torch.empty((B, 3, H // s, W // s, 6), dtype=torch.float32, device=dev) for s in STRIDES]
        L.check(L.lib().yolo_build_targets_hw(bt.data_ptr(), ct.data_ptr(), mb, anc.data_ptr(), B, H, W, float(ignore_iou_threshold),
                                              outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), L.current_stream()),
                "yolo_build_targets")
    return tuple(outs)


def _stable_order(major, minor, descending_minor):
    """Indices that order rows by (``major`` ascending, ``minor`` ascending / descending, original position): what two stable
    Python list sorts produce (utils.py:206,232). ``major`` holds small non-negative integers (class ids), ``minor`` any
    floats. One sort of unique 64-bit keys  major (11 bits) | orderable(minor) (32) | index (20)  by ``yolo_sort_u64`` (the
    NMS ordering kernels); above 262,144 rows or 2,047 classes the same two stable sorts run through ``torch.sort``."""
    n = int(major.shape[0])
    if n == 0:
        return torch.empty(0, dtype=torch.long, device=major.device)
    if n > 262144 or n >= (1 << 20) or float(major.max()) > 2046:
        o = torch.sort(minor, descending=descending_minor, stable=True).indices
        return o[torch.sort(major[o], stable=True).indices]
    bits = (minor.float() + 0.0).contiguous().view(torch.int32).to(torch.int64) & 0xffffffff      # -0.0 -> +0.0: equal in Python
    u = torch.where(bits >= 0x80000000, bits ^ 0xffffffff, bits | 0x80000000)                     # ascending-orderable
    if descending_minor:
        u = 0xffffffff - u
    keys = (major.to(torch.int64) << 52) | (u << 20) | torch.arange(n, dtype=torch.int64, device=major.device)
    out = torch.empty_like(keys)
    with torch.cuda.device(major.device):
        ws = torch.empty(L.lib().yolo_sort_u64_workspace_bytes(n), dtype=torch.uint8, device=major.device)
        L.check(L.lib().yolo_sort_u64(keys.data_ptr(), out.data_ptr(), n, ws.data_ptr(), ws.numel(), L.current_stream()), "yolo_sort_u64")
    return out & 0xfffff


# ------------------------------------------------------------------------------ mAP
def calc_mAP(pred_boxes, true_boxes, iou_threshold=0.5, box_format="center", num_classes=20):
    """Drop-in for the reference's ``calc_mAP`` (utils.py:193-274): rows ``[image_id, cx, cy, w, h, obj, class]``
    (lists or tensors), returns the mean over the classes that have ground truth of the trapezoid area under the
    precision/recall curve, as a 0-dim CPU tensor. The two stable list sorts become one device sort each
    (``_stable_order``), the per-pair Python loop two kernels (sequential matching per class, AP integration)."""
    dev = torch.device("cuda")
    dets = torch.as_tensor(pred_boxes, dtype=torch.float32).reshape(-1, 7).to(dev)
    gts = torch.as_tensor(true_boxes, dtype=torch.float32).reshape(-1, 7).to(dev)
    nc = int(num_classes)

    def class_rows(t):                                     # `box[-1] == c` for c in range(num_classes)
        c = t[:, 6]
        ok = (c >= 0) & (c < nc) & (c == torch.floor(c))
        return t[ok]
    dets, gts = class_rows(dets), class_rows(gts)
    # detections: objectness descending, then class ascending — both stable, so ties keep list order (list.sort)
    dets = dets[_stable_order(dets[:, 6], dets[:, 5], descending_minor=True)].contiguous()
    # ground truths: image ascending, then class ascending (stable): per (class, image) the list order survives
    gts = gts[_stable_order(gts[:, 6], gts[:, 0], descending_minor=False)].contiguous()

    def offsets(t):
        cnt = torch.bincount(t[:, 6].long(), minlength=nc)[:nc]
        return torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(cnt, 0)]).to(torch.int32).contiguous()
    d_off, g_off = offsets(dets), offsets(gts)
    with torch.cuda.device(dev):
        assigned = torch.empty(max(1, gts.shape[0]), dtype=torch.int32, device=dev)
        tp = torch.zeros(max(1, dets.shape[0]), dtype=torch.float32, device=dev)
        ap = torch.empty(nc, dtype=torch.float32, device=dev)
        L.check(L.lib().yolo_map_match(dets.data_ptr(), d_off.data_ptr(), gts.data_ptr(), g_off.data_ptr(), nc, gts.shape[0],
                                       float(iou_threshold), 1 if box_format == "center" else 0, assigned.data_ptr(), tp.data_ptr(),
                                       ap.data_ptr(), L.current_stream()), "yolo_map_match")
    ap = ap.cpu()
    valid = ap >= 0
    if not bool(valid.any()):
        raise ZeroDivisionError("division by zero")        # the reference divides by len([]) here
    return ap[valid].sum() / int(valid.sum())


# ------------------------------------------------------------------------------ evaluation at several thresholds
EvalResult = collections.namedtuple("EvalResult", "ap has_gt map map_50_95 n_gt n_det n_det_at_conf tp_at_conf precision recall f1")
EvalMatches = collections.namedtuple("EvalMatches", "order tp best_iou best_gt")
EVAL_MAX_THRESHOLDS = 16


def evaluate_detections(pred_boxes, true_boxes, num_classes, iou_thresholds=None, conf_threshold=0.5, box_format="center",
                        return_matches=False):
    """The evaluation of a detector in one pass (``yolo_eval_detections``): :func:`calc_mAP` at every IoU threshold of
    ``iou_thresholds`` (default 0.50, 0.55 .. 0.95, i.e. mAP@[.5:.95]; 1 to 16 values in [0, 1), any order), the AP of every class,
    and precision / recall / F1 of every class at the objectness threshold ``conf_threshold`` (strict ``>``, as the object filter of
    :func:`non_max_suppression`). Rows ``[image_id, cx, cy, w, h, obj, class]`` as lists or tensors, as for :func:`calc_mAP`; rows
    whose class is not in ``range(num_classes)`` are dropped. One upload, one sort per list, one call, one read-back.

    Returns an ``EvalResult`` of CPU tensors, T thresholds x nc classes: ``ap`` (T, nc) fp32, NaN where the class has no ground
    truth; ``has_gt`` (nc,) bool; ``map`` (T,) fp32, ``map[t]`` bit-equal to ``calc_mAP(..., iou_thresholds[t], ...)``;
    ``map_50_95`` = ``map.mean()``; ``n_gt`` / ``n_det`` / ``n_det_at_conf`` (nc,) int64: ground truths, detections, detections
    above ``conf_threshold``; ``tp_at_conf`` (T, nc) int64, the true positives among the latter; ``precision`` = tp / n_det_at_conf
    (0 without such a detection), ``recall`` = tp / n_gt (NaN without ground truth), ``f1`` = 2 p r / (p + r) (0 when p + r = 0),
    (T, nc) fp64. No class with ground truth: ``ZeroDivisionError``, as :func:`calc_mAP`.

    ``return_matches=True`` returns ``(result, EvalMatches)`` with device tensors for precision / recall curves and threshold
    picking: ``order`` (D,) int64, the row of ``pred_boxes`` behind each kept detection in (class ascending, objectness descending,
    stable) order; ``tp`` (T, D) bool; ``best_iou`` (D,) fp32 and ``best_gt`` (D,) int64, the ground truth every detection is
    compared with (its first maximum IoU > 0 among the ground truths of its image and class) as a row of ``true_boxes``, -1 for none."""
    thr = [0.5 + 0.05 * i for i in range(10)] if iou_thresholds is None else [float(v) for v in iou_thresholds]
    T = len(thr)
    if not 1 <= T <= EVAL_MAX_THRESHOLDS or not all(0.0 <= v < 1.0 for v in thr):
        raise ValueError(f"iou_thresholds: 1 to {EVAL_MAX_THRESHOLDS} numbers in [0, 1), got {thr}")
    conf = float(conf_threshold)
    if math.isnan(conf):
        raise ValueError("conf_threshold must be a number")
    dev = torch.device("cuda")
    dets = torch.as_tensor(pred_boxes, dtype=torch.float32).reshape(-1, 7).to(dev)
    gts = torch.as_tensor(true_boxes, dtype=torch.float32).reshape(-1, 7).to(dev)
    nc = int(num_classes)

    def ordered(t, minor, descending):                     # calc_mAP's class filter and stable order; rows[i] = the input row of t[i]
        c = t[:, 6]
        rows = torch.nonzero((c >= 0) & (c < nc) & (c == torch.floor(c))).reshape(-1)
        t = t[rows]
        o = _stable_order(t[:, 6], t[:, minor], descending_minor=descending)
        return t[o].contiguous(), rows[o]
    dets, det_rows = ordered(dets, 5, True)
    gts, gt_rows = ordered(gts, 0, False)

    def offsets(t):
        cnt = torch.bincount(t[:, 6].long(), minlength=nc)[:nc]
        return torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(cnt, 0)]).to(torch.int32).contiguous()
    d_off, g_off = offsets(dets), offsets(gts)
    D, G = int(dets.shape[0]), int(gts.shape[0])
    lib = L.lib()
    with torch.cuda.device(dev):
        best_iou = torch.empty(D, dtype=torch.float32, device=dev)
        best_gt = torch.empty(D, dtype=torch.int32, device=dev)
        tp = torch.empty((T, D), dtype=torch.uint8, device=dev)
        out = torch.empty(2 * T * nc + nc, dtype=torch.int32, device=dev)         # ap f32 [T nc] | tp_at_conf [T nc] | n_det_at_conf [nc]
        ws = torch.empty(int(lib.yolo_eval_workspace_bytes(D, G, T)), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_eval_detections(dets.data_ptr(), d_off.data_ptr(), D, gts.data_ptr(), g_off.data_ptr(), G, nc, (C.c_float * T)(*thr), T,
                                         conf, 1 if box_format == "center" else 0, best_iou.data_ptr(), best_gt.data_ptr(), tp.data_ptr(),
                                         out.data_ptr(), out.data_ptr() + 4 * T * nc, out.data_ptr() + 8 * T * nc, ws.data_ptr(), ws.numel(),
                                         L.current_stream()), "yolo_eval_detections")
        host = torch.cat([out, d_off, g_off]).cpu()                                # the one read-back
    ap = host[:T * nc].view(torch.float32).reshape(T, nc).clone()
    tp_at_conf = host[T * nc:2 * T * nc].reshape(T, nc).to(torch.int64)
    n_det_at_conf = host[2 * T * nc:2 * T * nc + nc].to(torch.int64)
    offs = host[2 * T * nc + nc:].to(torch.int64)
    n_det, n_gt = offs[1:nc + 1] - offs[:nc], offs[nc + 2:] - offs[nc + 1:-1]
    has_gt = n_gt > 0
    if not bool(has_gt.any()):
        raise ZeroDivisionError("division by zero")        # as calc_mAP
    mp = torch.stack([ap[t][ap[t] >= 0].sum() / int((ap[t] >= 0).sum()) for t in range(T)])      # calc_mAP's fp32 host arithmetic
    ap[:, ~has_gt] = math.nan
    tpd, nd = tp_at_conf.double(), n_det_at_conf.double()
    precision = torch.where(nd > 0, tpd / nd.clamp(min=1), torch.zeros((), dtype=torch.float64)).expand(T, nc).clone()
    recall = torch.where(has_gt, tpd / n_gt.double().clamp(min=1), torch.full((), math.nan, dtype=torch.float64)).expand(T, nc).clone()
    pr = precision + recall
    f1 = torch.where(pr == 0, torch.zeros((), dtype=torch.float64), 2 * precision * recall / torch.where(pr == 0, torch.ones_like(pr), pr))
    res = EvalResult(ap, has_gt, mp, mp.mean(), n_gt, n_det, n_det_at_conf, tp_at_conf, precision, recall, f1)
    if not return_matches:
        return res
    bg = best_gt.long()
    bg = torch.where(bg >= 0, gt_rows[bg.clamp(min=0)], bg) if G else bg
    return res, EvalMatches(det_rows, tp.bool(), best_iou, bg)


def evaluate_model(loader, model, anchors, iou_threshold=0.45, obj_threshold=0.5, **kw):
    """:func:`eval_boxes` (forward, decode, NMS at ``iou_threshold`` / ``obj_threshold``) and :func:`evaluate_detections` of its two
    tensors, which never leave the device in between. ``kw`` goes to :func:`evaluate_detections`; ``num_classes`` defaults to
    ``model.num_classes``, ``box_format`` is shared by both."""
    kw = dict(kw)
    nc = kw.pop("num_classes", None)
    nc = model.num_classes if nc is None else nc
    pred, true = eval_boxes(loader, model, iou_threshold, anchors, obj_threshold, kw.get("box_format", "center"))
    return evaluate_detections(pred, true, nc, **kw)


# ------------------------------------------------------------------------------ accuracy
def accuracy_counts(predictions, targets, object_threshold, counts=None):
    """Accumulate the five counters of ``check_model_accuracy`` (utils.py:355-372) for one batch: ``predictions`` /
    ``targets`` are the three per-scale tensors; returns an int64 tensor [class correct, n_obj, obj correct,
    noobj correct, n_noobj] on the device (pass it back in as ``counts`` to keep accumulating)."""
    dev = predictions[0].device
    if dev.type != "cuda":
        raise RuntimeError("accuracy_counts runs on MI355X only (no CPU fallback)")
    if counts is None:
        counts = torch.zeros(5, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        for p, t in zip(predictions, targets):
            if p.dtype != torch.float32:
                raise ValueError("fp32 predictions expected")
            t = t.to(dev, torch.float32).contiguous()
            B, _, gh, gw, D = p.shape
            if tuple(t.shape[:4]) != (B, 3, gh, gw):
                raise ValueError(f"target shape {tuple(t.shape)} does not match predictions {tuple(p.shape)}")
            strides = (C.c_int64 * 5)(*p.stride())
            L.check(L.lib().yolo_accuracy_counts_hw(p.data_ptr(), strides, t.data_ptr(), B, gh, gw, D - 5, float(object_threshold),
                                                    counts.data_ptr(), L.current_stream()), "yolo_accuracy_counts")
    return counts


def check_model_accuracy(model, loader, object_threshold):
    """Drop-in for the reference's ``check_model_accuracy`` (utils.py:334-381): class / no-object / object accuracy over
    a loader; one fused counting kernel per scale instead of ~15 mask / gather / reduce launches, one host sync at the end."""
    was_training = model.training
    model.eval()
    counts = None
    dev = next(model.parameters()).device
    for x, target in loader:
        with torch.no_grad():
            out = model(x.to(dev))
        counts = accuracy_counts(out, list(target), object_threshold, counts)
    c = [0] * 5 if counts is None else [int(v) for v in counts.tolist()]
    ct = [torch.tensor(v) for v in c]                      # int64 / (int64 + 1e-16) -> fp32 division, as in the reference
    class_accuracy = ct[0] / (ct[1] + 1e-16)
    noobj_accuracy = ct[3] / (ct[4] + 1e-16)
    obj_accuracy = ct[2] / (ct[1] + 1e-16)
    print(f"Class accuracy is: {(class_accuracy) * 100:2f}%")
    print(f"No obj accuracy is: {(noobj_accuracy) * 100:2f}%")
    print(f"Obj accuracy is: {(obj_accuracy) * 100:2f}%")
    if was_training:
        model.train()
    return class_accuracy, noobj_accuracy, obj_accuracy


# ------------------------------------------------------------------------------ evaluation boxes
def eval_boxes(loader, model, iou_threshold, anchors, obj_threshold, box_format="center"):
    """Device-resident ``get_eval_boxes`` (utils.py:276-332): per batch one forward, one fused decode + batched NMS
    (:func:`detect`) and one decode of the last-scale targets; returns two tensors of rows
    ``[image_id, cx, cy, w, h, obj, class]`` — kept predictions in the reference's order (image by image,
    objectness-descending) and ground-truth boxes (cells of ``targets[2]`` with objectness > ``obj_threshold``).
    Feed them straight to :func:`calc_mAP`."""
    was_training = model.training
    model.eval()
    dev = next(model.parameters()).device
    preds_out, trues_out = [], []
    data_idx = 0
    for x, targets in loader:
        with torch.no_grad():
            predictions = model(x.to(dev))
        B = x.shape[0]
        # anchors in grid cells: * S / stride (utils.py:300-309); an H x W batch uses L = max(H, W) (see scaled_anchors)
        sa = [torch.as_tensor(anchors[i], dtype=torch.float32, device=dev).reshape(3, 2) * max(predictions[i].shape[2:4])
              for i in range(3)]
        boxes, keep, count = detect(predictions, sa, iou_threshold, obj_threshold, box_format)
        ghw = tuple(predictions[2].shape[2:4])
        true_boxes = decode_boxes(targets[2].to(dev, torch.float32).contiguous(), sa[2], ghw, is_pred=False)     # (B, 3 gh gw, 6)
        cnt = count.tolist()
        for b in range(B):
            kb = boxes[b, keep[b, :cnt[b]].long()]
            ids = torch.full((kb.shape[0], 1), float(data_idx + b), device=dev)
            preds_out.append(torch.cat([ids, kb], 1))
            tb = true_boxes[b][true_boxes[b][:, 4] > obj_threshold]
            trues_out.append(torch.cat([torch.full((tb.shape[0], 1), float(data_idx + b), device=dev), tb], 1))
        data_idx += B
    if was_training:
        model.train()
    empty = torch.zeros((0, 7), device=dev)
    return (torch.cat(preds_out) if preds_out else empty), (torch.cat(trues_out) if trues_out else empty)


def get_eval_boxes(loader, model, iou_threshold, anchors, obj_threshold, box_format="center", device=None):
    """Drop-in for the reference's ``get_eval_boxes`` (utils.py:276-332): same arguments, same two Python lists of
    ``[image_id, cx, cy, w, h, obj, class]`` rows. (``device`` is accepted for signature compatibility; the model's
    device is used.) It leaves the model in train mode like the reference (utils.py:331)."""
    p, t = eval_boxes(loader, model, iou_threshold, anchors, obj_threshold, box_format)
    model.train()
    return p.tolist(), t.tolist()


# ------------------------------------------------------------------------------ letterbox
def letterbox(images, image_size=416, device=None, rect=False):
    """``config.set_only_image_transforms`` (config.py:101-113) on the device: each uint8 (H, W, 3) image (tensor or
    array) is resized so that its longer side is ``image_size`` (bilinear), centred on a zero canvas, scaled to [0,1]
    and laid out CHW. Returns ``(batch (B,3,Hc,Wc) fp32, meta)`` with ``meta[i] = (orig_h, orig_w, new_h, new_w,
    pad_top, pad_left)`` for :func:`unletterbox_boxes`. Parity with cv2 is unpinned (see csrc/preprocess.hip).
    ``rect=False``: the canvas is ``image_size`` square. ``rect=True``: (Hc, Wc) are the smallest multiples of 32 that hold
    every resized image of the batch (``yolo_letterbox_canvas``); resize arithmetic and the centring rule are the square
    path's, so the resized pixels are the same bits as the interior of the square letterbox."""
    if isinstance(images, (torch.Tensor,)) and images.dim() == 3 or not isinstance(images, (list, tuple)):
        images = [images]
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("letterbox runs on MI355X only (no CPU fallback)")
    S = int(image_size)
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("images must be uint8 (H, W, 3)")
        ts.append(t)
    hw = (C.c_int32 * max(2 * len(ts), 2))(*[int(v) for t in ts for v in t.shape[:2]])
    canvas = (C.c_int32 * 2)()
    L.check(L.lib().yolo_letterbox_canvas(hw, len(ts), S, int(bool(rect)), canvas), "yolo_letterbox_canvas")
    Hc, Wc = int(canvas[0]), int(canvas[1])
    with torch.cuda.device(dev):
        out = torch.empty((len(ts), 3, Hc, Wc), dtype=torch.float32, device=dev)
        meta = []
        for i, t in enumerate(ts):
            t = t.to(dev).contiguous()
            nhw, pad = (C.c_int * 2)(), (C.c_int * 2)()
            L.check(L.lib().yolo_letterbox_hw(t.data_ptr(), t.shape[0], t.shape[1], S, Hc, Wc, out[i].data_ptr(), nhw, pad,
                                              L.current_stream()), "yolo_letterbox")
            t.record_stream(torch.cuda.current_stream())
            meta.append((int(t.shape[0]), int(t.shape[1]), nhw[0], nhw[1], pad[0], pad[1]))
    return out, meta


def unletterbox_boxes(boxes, original_hw, resized_hw, meta=None):
    """Box mapping of ``plot_original`` (utils.py:475-501): normalised letterboxed ``[cx, cy, w, h, obj, cls]`` rows ->
    coordinates normalised to the ORIGINAL image. Same arithmetic (incl. its ``int(o * scale)`` size and ``// 2`` padding).
    ``resized_hw`` is the canvas (H, W). The reference's formula re-derives the resize from the canvas, which is only exact
    for a square canvas: on a rectangular one the short side can hold padding of its own (another image of the batch set the
    canvas, or the resized side was rounded up to 32), and ``min(r_w / o_w, r_h / o_h)`` then picks the wrong axis or is
    off by a rounding. ``meta`` (the tuple :func:`letterbox` returned for this image) uses the letterbox's own resized size
    and padding instead."""
    r_h, r_w = resized_hw
    if meta is not None:
        _, _, new_height, new_width, pad_height, pad_width = meta
    else:
        o_h, o_w = original_hw
        scale = min(r_w / o_w, r_h / o_h)
        new_width, new_height = int(o_w * scale), int(o_h * scale)
        pad_width, pad_height = (r_w - new_width) // 2, (r_h - new_height) // 2
    return [[(b[0] * r_w - pad_width) / new_width, (b[1] * r_h - pad_height) / new_height, (b[2] * r_w) / new_width,
             (b[3] * r_h) / new_height, b[4], b[5]] for b in boxes]


# ------------------------------------------------------------------------------ training augmentation
AUG_NPARAM = 29                       # YOLO_AUG_NPARAM: [do_hsv, hue, sat, val, do_ssr, scale, dx, dy, do_flip, (mx_k, my_k) k < 10]


def augment_params(n, generator=None, mosaic=False):
    """The random draws of ``config.set_train_transforms`` for ``n`` images as an (n, 29) float64 table: each transform
    on with p = 0.5; ``hue ~ U(-2, 2)``, ``sat ~ U(-50, 50)``, ``val ~ U(-40, 40)`` (HueSaturationValue(2, 50, 40)),
    ``scale ~ U(1, 1.5)``, ``dx, dy ~ U(-0.0625, 0.0625)`` (ShiftScaleRotate(scale_limit=(0, 0.5), rotate_limit=0)), and
    with ``mosaic`` the 10 cutout draws ``(x, y) ~ U(0.2, 0.3)`` of ``mosaic_augmentation``. The same generator state
    gives the same table (the draws are taken in one call whether or not ``mosaic`` is set)."""
    u = torch.rand((int(n), AUG_NPARAM), generator=generator, dtype=torch.float64)
    p = torch.zeros((int(n), AUG_NPARAM), dtype=torch.float64)
    for col in (0, 4, 8):
        p[:, col] = (u[:, col] < 0.5).to(torch.float64)
    p[:, 1] = -2.0 + 4.0 * u[:, 1]
    p[:, 2] = -50.0 + 100.0 * u[:, 2]
    p[:, 3] = -40.0 + 80.0 * u[:, 3]
    p[:, 5] = 1.0 + 0.5 * u[:, 5]
    p[:, 6] = -0.0625 + 0.125 * u[:, 6]
    p[:, 7] = -0.0625 + 0.125 * u[:, 7]
    if mosaic:
        p[:, 9:] = 0.2 + 0.1 * u[:, 9:]
    return p


def _resized_hw(h, w, size):
    scale = size / float(max(h, w))
    nh, nw = (int(round(h * scale)), int(round(w * scale))) if scale != 1.0 else (h, w)   # round(): half to even
    return max(nh, 1), max(nw, 1)


def _pinned(n, dtype):
    return torch.empty(n, dtype=dtype, pin_memory=True)


def augment_batch(images, boxes, image_size=416, params=None, generator=None, mosaic=None, device=None):
    """``YOLODataset.apply_augmentations`` (dataset.py:75-111) for a whole batch on the device, with no host synchronisation.

    ``images``: list of uint8 (H, W, 3) tensors or arrays (CPU: staged with one pinned copy; or already on the device).
    ``boxes``: one entry per image, ``[[x, y, w, h, class], ...]`` (normalised, the dataset's order) or ``None`` for an image
    without a label file (letterbox only, count 0; dataset.py:162-165). ``image_size``: S or (H, W) (multiples of 32).
    ``mosaic``: ``None`` (output image b is the standard transform of ``images[b]``) or a (B, 4) index array into ``images``:
    row b is ``mosaic_augmentation`` of the four images followed by ``set_train_transforms(mosaic=True)``; a row
    ``[i, -1, -1, -1]`` is the standard transform of image i. ``params``: the (B, 29) table of :func:`augment_params`
    (drawn from ``generator`` when omitted). Returns ``(x (B, 3, H, W) fp32, boxes (B, M, 5) fp32, counts (B,) int32)``, all
    on the device: the padded box table is the input of :func:`build_targets`. Parity with cv2 / albumentations is unpinned
    (see csrc/augment.hip)."""
    x, out_boxes, counts, launch = _augment_prepare(images, boxes, image_size, params, generator, mosaic, device)
    launch()
    return x, out_boxes, counts


def _augment_prepare(images, boxes, image_size, params, generator, mosaic, device):
    """augment_batch up to the launches: validated tables uploaded, outputs allocated; ``launch()`` enqueues the kernels
    (tools/augment_bench.py times it alone)."""
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("augment_batch runs on MI355X only (no CPU fallback)")
    H, W = _grid_hw(image_size)
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("images must be uint8 (H, W, 3)")
        ts.append(t)
    n = len(ts)
    if n == 0 or len(boxes) != n:
        raise ValueError("augment_batch needs at least one image and one box entry (or None) per image")
    if mosaic is None:
        src = [[i, -1, -1, -1] for i in range(n)]
    else:
        src = [[int(v) for v in row] for row in (mosaic.tolist() if hasattr(mosaic, "tolist") else mosaic)]
        if any(len(r) != 4 for r in src):
            raise ValueError("mosaic must be a (B, 4) index array")
        S = max(H, W)
        for r in src:
            if r[1] < 0:
                continue
            if H != W:
                raise ValueError(f"mosaic needs a square image_size (got {H}x{W}): rectangular mosaic is not built")
            if any(not 0 <= k < n for k in r):
                raise ValueError(f"mosaic row {r} indexes outside the {n} images")
            sizes = {_resized_hw(int(ts[k].shape[0]), int(ts[k].shape[1]), S) for k in r}
            if len(sizes) != 1:
                raise ValueError(f"mosaic row {r}: the four images resize to different sizes {sorted(sizes)} (the reference "
                                 "needs them equal)")
    B = len(src)
    if params is None:
        params = augment_params(B, generator, mosaic=mosaic is not None)
    params = torch.as_tensor(params)
    if tuple(params.shape) != (B, AUG_NPARAM):
        raise ValueError(f"params must be ({B}, {AUG_NPARAM})")
    # host tables: box rows per pool image (None -> -1), the pool layout, the source slots
    nbox = [-1 if b is None else len(b) for b in boxes]
    max_in = max([1] + nbox)
    max_out = max(1, max(sum(max(nbox[k], 0) for k in r if k >= 0) for r in src))
    hw_l = [int(v) for t in ts for v in t.shape[:2]]
    src_l = [k for r in src for k in r]
    # one pinned staging buffer for every small table: float64 params + boxes, then int64 offsets, then int32 hw / src / nbox
    n_f = (0 if params.device.type == "cuda" else B * AUG_NPARAM) + n * max_in * 5
    n_i = n + (2 * n + 4 * B + n + 1) // 2
    host = _pinned(n_f + n_i, torch.float64)
    hf = host[:n_f]
    off_p = 0
    if params.device.type != "cuda":
        hf[:B * AUG_NPARAM] = params.to(torch.float64).reshape(-1)
        off_p = B * AUG_NPARAM
    bx = hf[off_p:].view(n, max_in, 5)
    bx.zero_()
    for i, bl in enumerate(boxes):
        if bl is not None and len(bl):
            bx[i, :len(bl)] = torch.as_tensor(bl, dtype=torch.float64).reshape(-1, 5)
    hi = host[n_f:].view(torch.int64)
    cpu = [i for i, t in enumerate(ts) if t.device.type != "cuda"]
    offs, o = [0] * n, 0
    for i in cpu + [i for i in range(n) if i not in cpu]:
        offs[i] = o
        o += ts[i].numel()
    hi[:n] = torch.tensor(offs, dtype=torch.int64)
    h32 = hi[n:].view(torch.int32)
    h32[:2 * n] = torch.tensor(hw_l, dtype=torch.int32)
    h32[2 * n:2 * n + 4 * B] = torch.tensor(src_l, dtype=torch.int32)
    h32[2 * n + 4 * B:3 * n + 4 * B] = torch.tensor(nbox, dtype=torch.int32)
    n_cpu_bytes = sum(ts[i].numel() for i in cpu)
    if n_cpu_bytes:
        pool_host = _pinned(n_cpu_bytes, torch.uint8)
        for i in cpu:
            pool_host[offs[i]:offs[i] + ts[i].numel()] = ts[i].reshape(-1)
    with torch.cuda.device(dev):
        dtab = host.to(dev, non_blocking=True)
        pool = torch.empty(max(o, 1), dtype=torch.uint8, device=dev)
        if n_cpu_bytes:
            pool[:n_cpu_bytes].copy_(pool_host, non_blocking=True)
        for i in range(n):
            if i not in cpu:
                pool[offs[i]:offs[i] + ts[i].numel()].copy_(ts[i].to(dev).reshape(-1))
                ts[i].record_stream(torch.cuda.current_stream())
        dp = params.to(dev, torch.float64).contiguous() if params.device.type == "cuda" else dtab[:B * AUG_NPARAM]
        dbox = dtab[off_p:n_f]
        di = dtab[n_f:].view(torch.int64)
        d32 = di[n:].view(torch.int32)
        dhw, dsrc, dnbox = d32[:2 * n], d32[2 * n:2 * n + 4 * B], d32[2 * n + 4 * B:3 * n + 4 * B]
        x = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        out_boxes = torch.empty((B, max_out, 5), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        sel = torch.empty((B,), dtype=torch.int32, device=dev)
        staging = torch.empty(int(L.lib().yolo_augment_workspace_bytes(B, H, W)), dtype=torch.uint8, device=dev)
        hw_c = (C.c_int32 * (2 * n))(*hw_l)
        src_c = (C.c_int32 * (4 * B))(*src_l)

    def launch():
        with torch.cuda.device(dev):
            stream = L.current_stream()
        L.check(L.lib().yolo_augment_boxes(dbox.data_ptr(), dnbox.data_ptr(), max_in, dhw.data_ptr(), dsrc.data_ptr(), hw_c, n, src_c,
                                           dp.data_ptr(), B, H, W, out_boxes.data_ptr(), counts.data_ptr(), max_out, sel.data_ptr(),
                                           stream), "yolo_augment_boxes")
        L.check(L.lib().yolo_augment_images(pool.data_ptr(), di.data_ptr(), dhw.data_ptr(), dsrc.data_ptr(), hw_c, n, src_c,
                                            dp.data_ptr(), sel.data_ptr(), B, H, W, staging.data_ptr(), x.data_ptr(), stream),
                "yolo_augment_images")
    return x, out_boxes, counts, launch


def train_batch(images, boxes, anchors, image_size=416, **kw):
    """:func:`augment_batch` followed by :func:`build_targets` on its padded device table: the ``(x, targets)`` a training
    step (``GraphedTrainStep`` / ``YOLOLoss``) consumes, with no host synchronisation. ``kw`` goes to :func:`augment_batch`."""
    x, bt, ct = augment_batch(images, boxes, image_size=image_size, **kw)
    anc = torch.as_tensor(anchors, dtype=torch.float32).reshape(9, 2)
    if anc.device != x.device:
        pinned = _pinned(18, torch.float32)
        pinned.copy_(anc.reshape(-1))
        anc = pinned.to(x.device, non_blocking=True).reshape(9, 2)
    return x, build_targets(bt, anc, image_size, counts=ct, device=x.device)


# ------------------------------------------------------------------------ checkpoints
def save_checkpoint(model, optimizer, filename="YOLOv3TurbineCheckpoint.pth.tar", ema=None):
    """`utils.py:383-396`: ``{"state_dict": model.state_dict(), "optimizer": optimizer.state_dict()}`` through ``torch.save``.
    The model's 438 ``state_dict`` entries and its parameter order are the reference's, so a file written here loads with
    the reference's ``load_checkpoint`` and the other way round (pinned by ``tests/golden/checkpoint.npz``).
    ``ema`` (a ``ModelEMA``): the file gains one key, ``"ema"`` (``ema.state_dict()``); without it the file is the reference's."""
    checkpoint = {"state_dict": model.state_dict(), "optimizer": optimizer.state_dict()}
    if ema is not None:
        checkpoint["ema"] = ema.state_dict()
    torch.save(checkpoint, filename)


def load_checkpoint(model, optimizer, lr, filename="", model_folder=None, map_location=None, ema=None):
    """`utils.py:398-416`: restore model and optimizer, then force every param group's ``lr``. The reference prefixes
    ``config.MODEL_FOLDER`` and maps to ``config.DEVICE``; there is no global config here, so both are arguments
    (``model_folder=None``: ``filename`` is the path; ``map_location=None``: the model's own device). ``ema``: restored from the
    file's ``"ema"`` entry; a file written without one raises ``KeyError``."""
    path = filename if model_folder is None else f"{model_folder}/{filename}"
    if map_location is None:
        map_location = next(model.parameters()).device
    checkpoint = torch.load(path, map_location=map_location)
    if ema is not None and "ema" not in checkpoint:
        raise KeyError(f"{path} holds no weight average (no \"ema\" entry: it was saved without ema=)")
    model.load_state_dict(checkpoint["state_dict"])          # invalidates the packed-weight cache (post-hook in model.py)
    optimizer.load_state_dict(checkpoint["optimizer"])
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr
    if ema is not None:
        ema.load_state_dict(checkpoint["ema"])
    print(f"Checkpoint loaded from {filename}")
