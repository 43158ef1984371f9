"""Weighted box fusion (csrc/fuse.hip) and test-time augmentation (csrc/tta.hip): the views of a frame, their boxes, their fusion."""
import torch

from . import _lib as L
from .boxes import _anchors_to_device, _decode3, _workspace, scaled_anchors
from .tiles import _scales

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
    scales = _scales(scales, top=4, distinct=False)             # a repeated scale is a repeated view, below
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
    n_view = [3 * ((hv // 32) * (wv // 32) + (hv // 16) * (wv // 16) + (hv // 8) * (wv // 8)) for hv, wv, _, _ in views]
    total = sum(n_view)
    with torch.cuda.device(dev):
        stream = L.current_stream()
        anc = _anchors_to_device(torch.cat([scaled_anchors(anchors, hv, wv) for hv, wv, _, _ in views]), dev, (len(views), 3, 3, 2))
        boxes = torch.empty((B, total, 6), dtype=torch.float32, device=dev)
        tail = torch.empty(len(views), dtype=torch.int32, device=dev)            # NaN flag per view
        L.check(lib.yolo_fill_zero(tail.data_ptr(), tail.numel() * 4, stream), "yolo_fill_zero")
        src = None
        with eng.deferred_nan():
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
                with torch.no_grad():
                    preds = model(xv)
                eng.keep_pending_flag(tail.data_ptr(), v, stream)
                if sum(3 * p.shape[2] * p.shape[3] for p in preds) != n_view[v]:
                    raise ValueError("tta_boxes needs the three heads at strides 32, 16 and 8")
                _decode3(preds, anc[v], B, boxes, total, off, stream=stream)
                L.check(lib.yolo_boxes_unflip(boxes.data_ptr(), B, total, off, n_view[v], flr, fud, stream), "yolo_boxes_unflip")
                off += n_view[v]
        res = post(boxes, len(views)) if post is not None else None
        flags = tail.tolist()                                                  # the one host synchronisation
    eng.raise_on_flags(flags)
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
