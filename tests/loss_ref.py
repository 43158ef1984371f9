"""TEST INFRASTRUCTURE ONLY. The per-scale loss with its optional terms, restated from their definition in
plain torch under autograd: the yardstick of `csrc/loss_iou.hip`. Evaluated in the dtype of ``predictions`` (the tests give
it fp64 on the CPU; the same function on GPU tensors is "the PyTorch composition" of these terms, boolean masks included).
It mutates none of its arguments.

For one scale, with b = (sig(p0), sig(p1), exp(p2) aw, exp(p3) ah) and g = t0..3 on the cells with t4 == 1:
  x1 = cx - w/2, x2 = x1 + w (y alike);  inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1))
  union = bw bh + gw gh - inter + 1e-6;  IoU = inter / union;  cw = max(x2) - min(x1), ch = max(y2) - min(y1)
  GIoU = IoU - (C - union) / C with C = cw ch + 1e-6
  DIoU = IoU - rho2 / c2 with rho2 = (bx - gx)^2 + (by - gy)^2, c2 = cw^2 + ch^2 + 1e-6
  CIoU = DIoU - alpha v with v = 4/pi^2 (atan(gw/gh) - atan(bw/bh))^2, alpha = v / (1 - IoU + v + 1e-6) detached
  box    = mean(1 - XIoU), or for "mse" the reference's MSE([p0, sig(p1), sig(p2), p3], [t0, t1, log(1e-16 + t2/aw), log(1e-16 + t3/ah)])
  object = mean((p4 - IoU)^2) or mean(BCEWithLogits(p4, IoU)), IoU detached
  noobj  = mean over the cells with t4 == 0 of sig(p4)^gamma softplus(p4)
  class  = CrossEntropy(p5.., t5, label_smoothing)
Returns [l_box * box, l_obj * object, l_noobj * noobj, l_class * class]; no object cell: box = object = class = 0.
"""
import math

import torch
import torch.nn.functional as F

BOX_KINDS = ("mse", "giou", "diou", "ciou")
OBJ_KINDS = ("mse", "bce")
DEFAULT_LAMBDAS = (5, 1, 0.5, 1)


def box_geometry(b, g):
    """(IoU, union, cw, ch) of (N,4) cxcywh boxes, row by row."""
    bx1, by1, gx1, gy1 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, g[:, 0] - g[:, 2] / 2, g[:, 1] - g[:, 3] / 2
    bx2, by2, gx2, gy2 = bx1 + b[:, 2], by1 + b[:, 3], gx1 + g[:, 2], gy1 + g[:, 3]
    iw = (torch.minimum(bx2, gx2) - torch.maximum(bx1, gx1)).clamp(min=0)
    ih = (torch.minimum(by2, gy2) - torch.maximum(by1, gy1)).clamp(min=0)
    inter = iw * ih
    union = b[:, 2] * b[:, 3] + g[:, 2] * g[:, 3] - inter + 1e-6
    cw = torch.maximum(bx2, gx2) - torch.minimum(bx1, gx1)
    ch = torch.maximum(by2, gy2) - torch.minimum(by1, gy1)
    return inter / union, union, cw, ch


def xiou(b, g, kind):
    """(XIoU, IoU) per row for kind in giou / diou / ciou."""
    iou, union, cw, ch = box_geometry(b, g)
    if kind == "giou":
        c = cw * ch + 1e-6
        return iou - (c - union) / c, iou
    rho2 = (b[:, 0] - g[:, 0]) ** 2 + (b[:, 1] - g[:, 1]) ** 2
    c2 = cw ** 2 + ch ** 2 + 1e-6
    diou = iou - rho2 / c2
    if kind == "diou":
        return diou, iou
    assert kind == "ciou", kind
    v = (4 / math.pi ** 2) * (torch.atan(g[:, 2] / g[:, 3]) - torch.atan(b[:, 2] / b[:, 3])) ** 2
    alpha = (v / (1 - iou + v + 1e-6)).detach()
    return diou - alpha * v, iou


def yolo_loss_opts(predictions, targets, anchors, box_loss="mse", obj_loss="mse", focal_gamma=0.0, label_smoothing=0.0,
                   lambdas=DEFAULT_LAMBDAS):
    assert box_loss in BOX_KINDS and obj_loss in OBJ_KINDS
    dt = predictions.dtype
    targets = targets.to(dt)
    anchors = anchors.to(dt).reshape(1, 3, 1, 1, 2)
    obj = targets[..., 4] == 1
    noobj = targets[..., 4] == 0                     # -1 cells are ignored by both masks
    zero = torch.zeros((), dtype=dt, device=predictions.device)
    box = objectness = cls = zero
    x = predictions[..., 4][noobj]
    no_obj = (torch.sigmoid(x) ** focal_gamma * F.softplus(x)).mean() if focal_gamma > 0 else F.softplus(x).mean()
    if bool(obj.any()):
        decoded = torch.cat([torch.sigmoid(predictions[..., :2]), torch.exp(predictions[..., 2:4]) * anchors], -1)
        b, g, p = decoded[obj], targets[..., :4][obj], predictions[obj]
        if box_loss == "mse":
            iou = box_geometry(b, g)[0]
            anc = anchors.expand(predictions.shape[0], 3, predictions.shape[2], predictions.shape[3], 2)[obj]
            got = torch.stack([p[:, 0], torch.sigmoid(p[:, 1]), torch.sigmoid(p[:, 2]), p[:, 3]], 1)
            want = torch.cat([g[:, :2], torch.log(1e-16 + g[:, 2:4] / anc)], 1)
            box = F.mse_loss(got, want)
        else:
            val, iou = xiou(b, g, box_loss)
            box = (1 - val).mean()
        iou = iou.detach()
        if obj_loss == "mse":
            objectness = F.mse_loss(p[:, 4], iou)
        else:
            objectness = F.binary_cross_entropy_with_logits(p[:, 4], iou)
        cls = F.cross_entropy(p[:, 5:], targets[..., 5][obj].long(), label_smoothing=label_smoothing)
    lb, lo, ln, lc = lambdas
    return [lb * box, lo * objectness, ln * no_obj, lc * cls]
