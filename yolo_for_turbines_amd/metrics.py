"""Evaluation (csrc/metrics.hip): mAP, one-pass evaluation at several IoU thresholds, accuracy counters, the boxes of a loader."""
import collections
import ctypes as C
import math

import torch

from . import _lib as L
from .boxes import decode_boxes, detect


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


def _class_offsets(t, nc):
    """Rows sorted by class (column 6) -> the int32 [nc + 1] start of every class."""
    cnt = torch.bincount(t[:, 6].long(), minlength=nc)[:nc]
    return torch.cat([torch.zeros(1, dtype=torch.long, device=t.device), torch.cumsum(cnt, 0)]).to(torch.int32).contiguous()


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
    d_off, g_off = _class_offsets(dets, nc), _class_offsets(gts, nc)
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
    d_off, g_off = _class_offsets(dets, nc), _class_offsets(gts, nc)
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
