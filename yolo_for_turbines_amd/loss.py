"""Drop-in mirror of the reference's per-scale loss (`/root/reference/code/loss.py:6-81`).

The loss stays ordinary PyTorch in the reference and it does here: it is
boolean-mask gathers plus four tiny reductions, and it defines the gradient that enters the HIP
backward kernels. Same constructor, same `forward(predictions, targets, anchors)` returning
``[5*box, 1*obj, 0.5*noobj, 1*class]``, same in-place side effects on its arguments.
"""
import torch
import torch.nn as nn

from .boxes import calc_iou


class YOLOLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.mse = nn.MSELoss()
        self.bce_logits = nn.BCEWithLogitsLoss()
        self.cross_entropy = nn.CrossEntropyLoss()
        self.sigmoid = nn.Sigmoid()
        self.lambda_box, self.lambda_obj, self.lambda_noobj, self.lambda_class = 5, 1, 0.5, 1

    def forward(self, predictions, targets, anchors):
        has_obj = targets[..., 4] == 1
        no_obj = targets[..., 4] == 0                      # cells marked -1 are ignored by both masks
        anchors = anchors.reshape(1, 3, 1, 1, 2)
        zero = torch.tensor(0.0, device=predictions.device)
        box_loss, object_loss, class_loss = zero, zero, zero
        no_obj_loss = self.bce_logits(predictions[..., 4][no_obj], targets[..., 4][no_obj])
        if has_obj.any():
            decoded = torch.cat([self.sigmoid(predictions[..., :2]), torch.exp(predictions[..., 2:4]) * anchors], dim=-1)
            ious = calc_iou(decoded[has_obj], targets[..., :4][has_obj]).unsqueeze(1).detach()
            object_loss = self.mse(predictions[..., 4:5][has_obj], ious * targets[..., 4:5][has_obj])
            predictions[..., 1:3] = self.sigmoid(predictions[..., 1:3])          # indices 1:3 as in loss.py:71
            targets[..., 2:4] = torch.log(1e-16 + targets[..., 2:4] / anchors)
            box_loss = self.mse(predictions[..., :4][has_obj], targets[..., :4][has_obj])
            class_loss = self.cross_entropy(predictions[..., 5:][has_obj], targets[..., 5][has_obj].long())
        return [self.lambda_box * box_loss, self.lambda_obj * object_loss, self.lambda_noobj * no_obj_loss,
                self.lambda_class * class_loss]


class _FusedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, anchors):
        import ctypes as C
        from . import _lib as L
        lib = L.lib()
        B, A, gh, gw, D = pred.shape
        dev = pred.device
        with torch.cuda.device(dev):
            out = torch.empty(4, dtype=torch.float32, device=dev)
            counts = torch.empty(2, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.yolo_loss_workspace_bytes_hw(B, gh, gw), dtype=torch.uint8, device=dev)
            strides = (C.c_int64 * 5)(*pred.stride())
            L.check(lib.yolo_loss_fwd_hw(pred.data_ptr(), strides, target.data_ptr(), anchors.data_ptr(), B, gh, gw, D - 5, out.data_ptr(),
                                         counts.data_ptr(), ws.data_ptr(), ws.numel(), L.current_stream()), "yolo_loss_fwd")
        ctx.save_for_backward(pred, target, anchors, counts)
        return out

    @staticmethod
    def backward(ctx, gout):
        import ctypes as C
        from . import _lib as L
        pred, target, anchors, counts = ctx.saved_tensors
        B, A, gh, gw, D = pred.shape
        with torch.cuda.device(pred.device):
            dpred = torch.empty((B, A, gh, gw, D), dtype=torch.float32, device=pred.device)
            gout = gout.float().contiguous()
            strides = (C.c_int64 * 5)(*pred.stride())
            L.check(L.lib().yolo_loss_bwd_hw(pred.data_ptr(), strides, target.data_ptr(), anchors.data_ptr(), B, gh, gw, D - 5,
                                             counts.data_ptr(), gout.data_ptr(), dpred.data_ptr(), L.current_stream()), "yolo_loss_bwd")
        return dpred, None, None


class _FusedLossOptsFn(torch.autograd.Function):
    """The same three launches through ``yolo_loss_fwd_opts`` / ``yolo_loss_bwd_opts`` (`csrc/loss_iou.hip`); ``opts`` is a
    `_lib.LossOpts`, read by the host when the kernels are launched."""

    @staticmethod
    def forward(ctx, pred, target, anchors, opts):
        import ctypes as C
        from . import _lib as L
        lib = L.lib()
        B, A, gh, gw, D = pred.shape
        dev = pred.device
        with torch.cuda.device(dev):
            out = torch.empty(4, dtype=torch.float32, device=dev)
            counts = torch.empty(2, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.yolo_loss_workspace_bytes_hw(B, gh, gw), dtype=torch.uint8, device=dev)
            strides = (C.c_int64 * 5)(*pred.stride())
            L.check(lib.yolo_loss_fwd_opts(pred.data_ptr(), strides, target.data_ptr(), anchors.data_ptr(), B, gh, gw, D - 5, out.data_ptr(),
                                           counts.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(opts), L.current_stream()),
                    "yolo_loss_fwd_opts")
        ctx.save_for_backward(pred, target, anchors, counts)
        ctx.opts = opts
        return out

    @staticmethod
    def backward(ctx, gout):
        import ctypes as C
        from . import _lib as L
        pred, target, anchors, counts = ctx.saved_tensors
        B, A, gh, gw, D = pred.shape
        with torch.cuda.device(pred.device):
            dpred = torch.empty((B, A, gh, gw, D), dtype=torch.float32, device=pred.device)
            gout = gout.float().contiguous()
            strides = (C.c_int64 * 5)(*pred.stride())
            L.check(L.lib().yolo_loss_bwd_opts(pred.data_ptr(), strides, target.data_ptr(), anchors.data_ptr(), B, gh, gw, D - 5,
                                               counts.data_ptr(), gout.data_ptr(), dpred.data_ptr(), C.byref(ctx.opts), L.current_stream()),
                    "yolo_loss_bwd_opts")
        return dpred, None, None, None


_BOX_LOSSES = ("mse", "giou", "diou", "ciou")
_OBJ_LOSSES = ("mse", "bce")
_DEFAULT_LAMBDAS = (5.0, 1.0, 0.5, 1.0)                       # loss.py:24-27


class FusedYOLOLoss(nn.Module):
    """Same values and gradients as :class:`YOLOLoss` (reference `loss.py:29-81`) from three fused HIP
    kernels per scale instead of ~35 boolean-mask / reduction launches: no data-dependent shapes, no host
    sync, deterministic sums — so a whole fine-tune step can be captured in a HIP graph
    (``tools/train_bench.py --graph``). Same call signature and return value; it does NOT mutate
    ``predictions`` / ``targets`` (the reference overwrites ``predictions[...,1:3]`` and ``targets[...,2:4]``).

    Every argument at its default is the reference's loss, through the same kernels as before. Anything else is NOT
    the reference's loss (`csrc/loss_iou.hip`); it keeps the call signature, the four returned parts and the
    graph capture:

    * ``box_loss``: ``"mse"`` (the reference), or ``"giou"`` / ``"diou"`` / ``"ciou"``: the mean over the object cells of
      ``1 - XIoU`` between the decoded box ``(sig(p0), sig(p1), exp(p2) aw, exp(p3) ah)`` and the target
    * ``obj_loss``: ``"mse"`` (the reference: ``(p4 - IoU)^2``) or ``"bce"`` (``BCEWithLogits(p4, IoU)``), IoU detached
    * ``focal_gamma`` >= 0: no-object cells cost ``sig(p4)^gamma * softplus(p4)``; 0 is the reference's BCE
    * ``label_smoothing`` in [0, 1): as ``torch.nn.CrossEntropyLoss(label_smoothing=...)``
    * ``lambdas``: the weights ``(box, obj, noobj, class)`` of the four parts
    """

    def __init__(self, box_loss="mse", obj_loss="mse", focal_gamma=0.0, label_smoothing=0.0, lambdas=_DEFAULT_LAMBDAS):
        super().__init__()
        import math
        if box_loss not in _BOX_LOSSES:
            raise ValueError(f"box_loss must be one of {_BOX_LOSSES}, not {box_loss!r}")
        if obj_loss not in _OBJ_LOSSES:
            raise ValueError(f"obj_loss must be one of {_OBJ_LOSSES}, not {obj_loss!r}")
        try:
            focal_gamma, label_smoothing = float(focal_gamma), float(label_smoothing)
            lambdas = tuple(float(v) for v in lambdas)
        except TypeError as e:
            raise ValueError(f"focal_gamma, label_smoothing and the four lambdas must be numbers: {e}") from e
        if not (math.isfinite(focal_gamma) and focal_gamma >= 0.0):
            raise ValueError(f"focal_gamma must be a finite number >= 0, not {focal_gamma}")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), not {label_smoothing}")
        if len(lambdas) != 4 or not all(math.isfinite(v) for v in lambdas):
            raise ValueError(f"lambdas must be four finite numbers (box, obj, noobj, class), not {lambdas}")
        self.box_loss, self.obj_loss, self.focal_gamma, self.label_smoothing, self.lambdas = (
            box_loss, obj_loss, focal_gamma, label_smoothing, lambdas)
        self._default = (box_loss, obj_loss, focal_gamma, label_smoothing, lambdas) == ("mse", "mse", 0.0, 0.0, _DEFAULT_LAMBDAS)
        self._opts = None

    def extra_repr(self):
        return (f"box_loss={self.box_loss!r}, obj_loss={self.obj_loss!r}, focal_gamma={self.focal_gamma}, "
                f"label_smoothing={self.label_smoothing}, lambdas={self.lambdas}")

    def _c_opts(self):
        if self._opts is None:
            from . import _lib as L
            self._opts = L.LossOpts(L.LOSS_BOX_KINDS[self.box_loss], L.LOSS_OBJ_KINDS[self.obj_loss], self.focal_gamma,
                                    self.label_smoothing, *self.lambdas)
        return self._opts

    def forward(self, predictions, targets, anchors):
        if not predictions.is_cuda:
            raise RuntimeError("FusedYOLOLoss runs on MI355X only (no CPU fallback); use YOLOLoss on the CPU")
        if predictions.dim() != 5 or predictions.shape[1] != 3:
            raise ValueError("predictions must be a (B,3,gh,gw,5+nc) tensor")
        if predictions.dtype in (torch.float16, torch.bfloat16):
            predictions = predictions.float()          # autocast heads (train.py:53): the loss terms are evaluated in fp32, as autocast does
        elif predictions.dtype != torch.float32:
            raise ValueError("predictions must be a floating-point (B,3,gh,gw,5+nc) tensor")
        t = targets.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.float().contiguous()
        a = anchors.detach().reshape(3, 2).to(device=predictions.device, dtype=torch.float32).contiguous()
        out = _FusedLossFn.apply(predictions, t, a) if self._default else _FusedLossOptsFn.apply(predictions, t, a, self._c_opts())
        # ONE backward node for the four parts (unbind -> stack): indexing out[0] .. out[3] gave four SelectBackward nodes, each a
        # zero-fill + a 4-byte blit copy + an accumulate - 36 tiny launches per step over the three scales
        return list(out.unbind(0))
