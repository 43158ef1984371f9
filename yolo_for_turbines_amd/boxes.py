"""IoU, box decode, NMS, ``detect`` / ``detect_images`` (csrc/decode.hip, nms_*.hip); anchors: in grid cells, of a dataset (anchors.hip)."""
import collections
import ctypes as C
import math

import torch

from . import _lib as L


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


def _anchors_to_device(anchors, device, shape):
    """``anchors`` as fp32 of ``shape`` on ``device``: as they are if already there, else through one pinned buffer (no host sync)."""
    anc = torch.as_tensor(anchors, dtype=torch.float32).reshape(shape)
    if anc.device == device:
        return anc
    staged = torch.empty(anc.numel(), dtype=torch.float32, pin_memory=True)
    staged.copy_(anc.reshape(-1))
    return staged.to(device, non_blocking=True).reshape(shape)


def _grid_hw(grid_size):
    """None | g | (gh, gw) -> None | (gh, gw)."""
    if grid_size is None:
        return None
    if isinstance(grid_size, (tuple, list)):
        gh, gw = grid_size
        return int(gh), int(gw)
    return int(grid_size), int(grid_size)


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


def _decode3(preds, anchors, n, out, rows, offset=None, write_back=False, *, stream):
    """The three heads of a forward in one launch: the first ``n`` images of ``preds`` (5-d, one class count) with the three (3, 2)
    device ``anchors`` into ``out`` (B, rows, 6) fp32, filling an image's ``rows`` (``yolo_decode3_hw``) or from row ``offset`` on
    (``yolo_decode3_hw_at``). A head that is not fp32 is always cast first, as ``detect_tiled`` / ``tta_boxes`` did; ``detect`` comes with fp32 only."""
    preds = [p if p.dtype == torch.float32 else p.float() for p in preds]
    pp = (C.c_void_p * 3)(*[p.data_ptr() for p in preds])
    st = (C.c_int64 * 15)(*[v for p in preds for v in p.stride()])
    ap = (C.c_void_p * 3)(*[a.data_ptr() for a in anchors])
    gg = (C.c_int * 6)(*[v for p in preds for v in (p.shape[2], p.shape[3])])      # (gh, gw) per scale
    args = (pp, st, ap, gg, n, preds[0].shape[4] - 5, int(bool(write_back)), out.data_ptr(), rows)
    rc = L.lib().yolo_decode3_hw(*args, stream) if offset is None else L.lib().yolo_decode3_hw_at(*args, int(offset), stream)
    L.check(rc, "yolo_decode3")


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


NMSOptions = collections.namedtuple("NMSOptions", "method sigma score_threshold class_agnostic max_det",
                                    defaults=("gaussian", 0.5, None, False, None))
NMSOptions.__doc__ = """How :func:`soft_nms` (and ``nms=`` of the detect functions) suppresses: ``method`` "hard" | "linear" | "gaussian"
(Soft-NMS, Bodla et al. 2017: an overlapped box keeps its place and loses score), ``sigma`` of the Gaussian decay ``exp(-iou^2 / sigma)``,
``score_threshold`` a rescored box must still exceed to be kept (``None``: the ``obj_threshold`` of the call), ``class_agnostic``: boxes
of different classes suppress each other too, ``max_det``: at most that many detections per image, the best ones (``None``: no cap)."""
NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def _nms_options(nms, obj_threshold):
    """``nms`` (an :class:`NMSOptions` or a dict of its fields) checked, as the arguments of ``yolo_soft_nms``:
    (method code, sigma, score_threshold, class_agnostic, max_det)."""
    if isinstance(nms, dict):
        unknown = sorted(set(nms) - set(NMSOptions._fields))
        if unknown:
            raise ValueError(f"unknown NMS option {unknown[0]!r}; the options are {', '.join(NMSOptions._fields)}")
        nms = NMSOptions(**nms)
    if not isinstance(nms, NMSOptions):
        raise ValueError(f"nms must be None, an NMSOptions or a dict of its fields, got {nms!r}")
    if not isinstance(nms.method, str) or nms.method not in NMS_METHODS:
        raise ValueError(f"method must be 'hard', 'linear' or 'gaussian', got {nms.method!r}")
    try:
        sigma = float(nms.sigma)
    except (TypeError, ValueError):
        sigma = math.nan
    if isinstance(nms.sigma, bool) or not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be a finite number > 0, got {nms.sigma!r}")
    obj = float(obj_threshold)
    if not math.isfinite(obj):
        raise ValueError(f"obj_threshold must be finite, got {obj_threshold!r}")
    score = obj
    if nms.score_threshold is not None:
        try:
            score = float(nms.score_threshold)
        except (TypeError, ValueError):
            score = math.nan
        if isinstance(nms.score_threshold, bool) or not math.isfinite(score) or score < obj:
            raise ValueError(f"score_threshold must be None or a finite number >= obj_threshold ({obj}), got {nms.score_threshold!r}")
    if not isinstance(nms.class_agnostic, bool):
        raise ValueError(f"class_agnostic must be a bool, got {nms.class_agnostic!r}")
    max_det = 0
    if nms.max_det is not None:
        if isinstance(nms.max_det, bool) or not isinstance(nms.max_det, int) or not 1 <= nms.max_det < 2 ** 31:
            raise ValueError(f"max_det must be None or an integer >= 1, got {nms.max_det!r}")
        max_det = nms.max_det
    return NMS_METHODS[nms.method], sigma, score, int(bool(nms.class_agnostic)), max_det


def _soft_nms(boxes, iou_threshold, obj_threshold, box_format, opts, rescore):
    """``yolo_soft_nms`` on a contiguous (B, N, 6) fp32 CUDA tensor with the checked options of :func:`_nms_options`; ``rescore``:
    ``None`` or the (B, N, 6) buffer (``boxes`` itself is allowed) whose column 4 receives the kept rows' new scores."""
    iou = float(iou_threshold)
    if not (math.isfinite(iou) and iou >= 0):
        raise ValueError(f"iou_threshold must be a finite number >= 0, got {iou_threshold!r}")
    method, sigma, score, agnostic, max_det = opts
    B, N, _ = boxes.shape
    dev = boxes.device
    lib = L.lib()
    with torch.cuda.device(dev):
        if N == 0 or B == 0:
            return (torch.full((B, max(N, 1)), -1, dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev),
                    torch.zeros((B, max(N, 1)), dtype=torch.float32, device=dev))
        nbytes = lib.yolo_soft_nms_workspace_bytes(B, N)
        if nbytes == 0:
            raise ValueError(f"soft_nms takes at most 2,047 images of at most 163,456 boxes, got {B} x {N}")
        keep = torch.empty((B, N), dtype=torch.int32, device=dev)
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        scores = torch.empty((B, N), dtype=torch.float32, device=dev)
        ws = _workspace(max(nbytes, 256), dev)
        L.check(lib.yolo_soft_nms(boxes.data_ptr(), B, N, iou, float(obj_threshold), score, int(box_format == "center"), method, sigma,
                                  agnostic, max_det, keep.data_ptr(), count.data_ptr(), scores.data_ptr(), L.ptr(rescore), ws.data_ptr(),
                                  ws.numel(), L.current_stream()), "yolo_soft_nms")
    return keep, count, scores


def soft_nms(boxes, iou_threshold, obj_threshold, box_format="corners", **options):
    """Batched device Soft-NMS (``yolo_soft_nms``; the arithmetic is stated in include/yolo_mi355x.h). ``boxes``: (B, N, 6) or (N, 6)
    fp32 CUDA tensor of [x,y,w,h,obj,cls], never written. ``options``: the fields of :class:`NMSOptions` (default: Gaussian decay
    with sigma 0.5). Returns (keep_idx (B,N) int32, keep_count (B,) int32, scores (B,N) fp32): for image b the first
    ``keep_count[b]`` entries of ``keep_idx`` index its input rows, best rescored objectness first (ties in input order), and
    ``scores`` holds that objectness; behind them ``keep_idx`` is -1 and ``scores`` 0. ``method="hard"`` with nothing else set
    keeps exactly what :func:`nms_indices` keeps. No host synchronisation."""
    if not boxes.is_cuda:
        raise RuntimeError("soft_nms runs on MI355X only (no CPU fallback)")
    opts = _nms_options(options, obj_threshold)
    single = boxes.dim() == 2
    if single:
        boxes = boxes.unsqueeze(0)
    if boxes.dim() != 3 or boxes.shape[-1] != 6:
        raise ValueError("boxes must be (B, N, 6)")
    keep, count, scores = _soft_nms(boxes.float().contiguous(), iou_threshold, obj_threshold, box_format, opts, None)
    if single:
        return keep[0], count[0], scores[0]
    return keep, count, scores


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


def detect(predictions, scaled_anchors, iou_threshold=0.45, obj_threshold=0.5, box_format="center", mutate=False, nms=None):
    """Fused post-processing of a forward pass (the sequence of demo.py:44-55 /
    utils.py:300-321, all images at once, nothing leaves HBM):
    decode three scales into one (B, N, 6) buffer in the reference's concatenation order
    (scale 0, 1, 2), then per-image NMS. Returns (boxes (B,N,6), keep_idx (B,N), keep_count (B,)).
    ``mutate=True`` also performs the in-place sigmoid / exp write-back ``cells_to_boxes`` does to the prediction tensors
    (utils.py:106-110); the reference's callers of this sequence never read them again, so the default leaves them alone.
    ``nms``: ``None`` (the reference's suppression, :func:`nms_indices`) or an :class:`NMSOptions` / a dict of its fields: the
    suppression of :func:`soft_nms`. The return convention is the same (image b keeps ``boxes[b, keep[b, :count[b]]]``, now best
    rescored objectness first), and column 4 of the kept rows of ``boxes`` holds the rescored objectness."""
    opts = None if nms is None else _nms_options(nms, obj_threshold)
    B = predictions[0].shape[0]
    n_per = [3 * p.shape[2] * p.shape[3] for p in predictions]
    total = sum(n_per)
    dev = predictions[0].device
    boxes = torch.empty((B, total, 6), dtype=torch.float32, device=dev)
    if len(predictions) == 3 and all(p.is_cuda and p.dtype == torch.float32 and p.dim() == 5 for p in predictions) \
            and len({p.shape[4] for p in predictions}) == 1:
        with torch.cuda.device(dev):                      # the three scales in one launch
            anc = [torch.as_tensor(a, dtype=torch.float32).reshape(3, 2).to(dev).contiguous() for a in scaled_anchors]
            _decode3(predictions, anc, B, boxes, total, write_back=mutate, stream=L.current_stream())
    else:
        off = 0
        for p, a, n in zip(predictions, scaled_anchors, n_per):
            decode_boxes(p, a, (p.shape[2], p.shape[3]), True, out=boxes, box_offset=off, mutate=mutate)
            off += n
    if opts is not None:
        keep, count, _ = _soft_nms(boxes, iou_threshold, obj_threshold, box_format, opts, boxes)
        return boxes, keep, count
    keep, count = nms_indices(boxes, iou_threshold, obj_threshold, box_format)
    return boxes, keep, count


def detect_images(model, x, scaled_anchors, iou_threshold=0.45, obj_threshold=0.5, box_format="center", nms=None):
    """``detect(model(x), ...)`` with ONE host synchronisation instead of two back to back: the forward's NaN guards
    (model.py:175,183-184) are read after decode and NMS have been enqueued, so the GPU does not sit idle between the
    forward and the post-processing while the host wakes up and launches them (~0.1-0.25 ms per batch). Same results, same
    exceptions (``AssertionError`` for a NaN input, ``ValueError("Nan in layer")``), raised before anything is returned.
    ``nms``: as for :func:`detect`."""
    if nms is not None:
        _nms_options(nms, obj_threshold)                  # a bad option is reported before the forward runs
    eng = model._engine
    with eng.deferred_nan(), torch.no_grad():
        preds = model(x)
        flag = eng.take_pending_flag()
    out = detect(preds, scaled_anchors, iou_threshold, obj_threshold, box_format, nms=nms)
    if flag is not None:
        eng.raise_on_nan(flag)
    return out


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
