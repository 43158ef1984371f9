"""Whole-step HIP graph for fine-tuning: capture once, replay every step.

The reference's step (`/root/reference/code/train.py:41-69`: autocast forward, three per-scale losses, backward,
optimizer step) is ~1,000 kernel launches here, many of them a few microseconds long; issued from Python one by
one the GPU idles between them. Every kernel of this package launches on the current stream, allocates nothing
behind PyTorch's back and — with :class:`FusedYOLOLoss` and the per-forward NaN guard off — never waits for the host,
so ``torch.cuda.graph`` can record the whole step into ONE HIP graph. Static shapes only: one graph per
(batch, image size); multi-scale training keeps one per size.
"""
from __future__ import annotations

import os

import torch

from .loss import FusedYOLOLoss


class GraphedTrainStep:
    """``step = GraphedTrainStep(model, optimizer, scaled_anchors, x, targets)`` then ``loss = step(x, targets)``.

    ``x``: (B,3,H,W) batch, ``targets``: the three (B,3,gh,gw,6) tensors of the loader, ``scaled_anchors``: (3,3,2) anchors
    in grid units (`train.py:195-197`). The example batch passed to the constructor fixes the shapes and is used for
    the warm-up steps on a side stream (so they DO update the model, like three ordinary steps). ``autocast_dtype``
    (``torch.bfloat16`` / ``torch.float16`` / None) selects what `train.py:53` selects. Returns the summed loss as a
    0-dim tensor that is overwritten by the next call.

    ``grad_scaler`` (a :class:`yolo_for_turbines_amd.GradScaler`, with a :class:`yolo_for_turbines_amd.SGD`, ``Adam`` or
    ``AdamW``): the step is
    `train.py:67-69`, ``scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()``, all of it captured - the
    scale, the growth tracker and the skip decision are device memory read at replay time, so a replay whose gradients
    overflow skips its update and halves the scale like an eager step. The warm-up steps go through the scaler too. The
    returned loss is the unscaled one; ``grad_scaler.get_scale()`` reads the live value (and waits for the device).

    ``ema`` (a :class:`yolo_for_turbines_amd.ModelEMA` of ``model``): the weight average moves inside the captured step. With a
    :class:`yolo_for_turbines_amd.SGD`, ``Adam`` or ``AdamW`` it is attached to the optimizer (if it is not already) and rides in the step's own
    launch; with any other optimizer the step ends with ``ema.update()``. The warm-up steps go through it like everything
    else, its decay follows the device counter through the replays, and every replay invalidates the packed weights of
    ``ema.module`` along with the live model's.
    """

    def __init__(self, model, optimizer, scaled_anchors, x, targets, autocast_dtype=None, loss_fn=None, warmup=3,
                 zero_grad=True, allow_data_parallel=None, grad_scaler=None, ema=None):
        if not x.is_cuda:
            raise RuntimeError("GraphedTrainStep needs CUDA/HIP tensors (no CPU fallback)")
        if grad_scaler is not None:
            from .amp import GradScaler
            from .optim import NativeOptimizer
            if not isinstance(grad_scaler, GradScaler) or not isinstance(optimizer, NativeOptimizer):
                raise TypeError("GraphedTrainStep: grad_scaler must be a yolo_for_turbines_amd.GradScaler stepping a "
                                "yolo_for_turbines_amd.SGD, Adam or AdamW (torch.amp.GradScaler.step reads its inf flag on the "
                                "host, which cannot be captured)")
            if not grad_scaler.is_enabled():
                raise ValueError("GraphedTrainStep: grad_scaler is disabled; pass grad_scaler=None instead")
        self.scaler = grad_scaler
        self.ema = ema
        self._ema_update = False                        # the step body ends with ema.update() (the optimizer cannot carry it)
        if ema is not None:
            from .optim import NativeOptimizer
            if isinstance(optimizer, NativeOptimizer):
                ema.attach(optimizer)                   # raises if it is attached elsewhere
            elif ema._attached is not None:
                raise RuntimeError("GraphedTrainStep: ema is attached to another optimizer than the one this step runs")
            else:
                self._ema_update = True
        if allow_data_parallel is None:
            allow_data_parallel = os.environ.get("YOLO_DP_GRAPH", "0") == "1"
        self._dp = getattr(model._engine, "ddp", None) is not None and model._engine.ddp[0] is not None
        if self._dp and not allow_data_parallel:
            raise NotImplementedError("GraphedTrainStep does not capture the data-parallel gradient all-reduce by default (RCCL inside a "
                                      "HIP graph capture has only been exercised with a 1-rank group here: DESIGN.md); pass "
                                      "allow_data_parallel=True / YOLO_DP_GRAPH=1 to capture it, or replay per rank on one GPU")
        self.model, self.opt = model, optimizer
        self.loss_fn = loss_fn if loss_fn is not None else FusedYOLOLoss()
        self.autocast_dtype = autocast_dtype
        self.anchors = [a.detach().to(x.device, torch.float32).contiguous() for a in scaled_anchors]
        self.x = x.detach().clone()
        self.targets = [t.detach().clone().float().contiguous() for t in targets]
        self.zero_grad = zero_grad
        self._nan_check = model._engine.nan_check
        model._engine.nan_check = False                 # the guard reads a flag on the host: a sync, not capturable
        try:
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):         # allocator warm-up, plan build, lazily created optimizer state
                    self._step_body()
            torch.cuda.current_stream(x.device).wait_stream(side)
            # The graph bakes in raw pointers to the train plan's buffers (activations, statistics, workspaces, packed
            # gradient weights). Own the plan: a strong reference keeps its memory alive, `pinned` exempts it from the
            # model's LRU of plans (multi-scale training builds other sizes in between replays).
            plans = [pl for k, pl in model._engine._plans.items() if k[0] == "train" and k[1] == x.shape[0] and k[2] == tuple(x.shape[2:4])]
            if not plans:
                raise RuntimeError("GraphedTrainStep: the warm-up steps left no train plan for this shape")
            self._plan = plans[-1]
            self._plan.pinned = True
            self.graph = torch.cuda.CUDAGraph()
            # Hyper-parameters across replays: `yt.SGD` / `yt.Adam` / `yt.AdamW` keep them in device memory and read them when the kernel runs
            # (`sync_hyper` before each replay), so LR schedulers keep working. Any other optimizer bakes its Python floats
            # into the captured kernels: remember them and refuse a replay at different values rather than train silently
            # at the capture-time learning rate.
            self._baked = None if hasattr(self.opt, "sync_hyper") else self._hyper_snapshot()
            if self.zero_grad:
                self.opt.zero_grad(set_to_none=True)
            # data parallel (opt-in): the warm-up steps above have created the communicator and run every bucket's collective
            # once eagerly; inside the capture the buckets issue synchronous all-reduces on the capturing stream
            # (dist.GradBuckets.fire), and capture errors stay local to this thread
            kw = {"capture_error_mode": "thread_local"} if self._dp else {}
            # Clipping (`yt.SGD(max_grad_norm=...)`): the number is device memory like the learning rate, but whether the step
            # clips at all, and by which norm, decides WHICH launches were captured.
            self._clip = self._clip_kind()
            with torch.cuda.graph(self.graph, **kw):
                self.loss = self._step_body(zero=False)
        finally:
            model._engine.nan_check = self._nan_check

    def _step_body(self, zero=True):
        if zero and self.zero_grad:
            self.opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=self.autocast_dtype or torch.bfloat16, enabled=self.autocast_dtype is not None):
            preds = self.model(self.x)
            loss = sum(sum(self.loss_fn(preds[i], self.targets[i], self.anchors[i])) for i in range(3))
        if self.scaler is not None:
            self.scaler.scale(loss).backward()
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            loss.backward()
            self.opt.step()
        if self._ema_update:
            self.ema.update()
        return loss.detach()

    def _hyper_snapshot(self):
        keys = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "betas", "eps")
        return [tuple((k, g[k]) for k in keys if k in g and not isinstance(g[k], torch.Tensor)) for g in self.opt.param_groups]

    def _clip_kind(self):
        """None when the optimizer does not clip, else its norm type (what the captured launches depend on)."""
        if getattr(self.opt, "max_grad_norm", None) is None:
            return None
        return float(self.opt.grad_norm_type)

    def __call__(self, x, targets):
        if tuple(x.shape) != tuple(self.x.shape):
            raise ValueError(f"this graph was captured for input shape {tuple(self.x.shape)}, got {tuple(x.shape)}")
        if self._clip_kind() != self._clip:
            raise RuntimeError("GraphedTrainStep: the optimizer's gradient clipping was switched since the capture "
                               f"(norm type {self._clip} -> {self._clip_kind()}, None = no clipping): the graph holds the launches of "
                               "the capture; change max_grad_norm between numbers only, or capture a new GraphedTrainStep")
        if self._plan.dropped:
            raise RuntimeError("GraphedTrainStep: the model dropped its plans after this graph was captured (model.to(...) / "
                               ".float() / .half() move the parameters the graph points at): capture a new GraphedTrainStep")
        if self._baked is None:
            self.opt.sync_hyper()                       # stream-ordered in front of the replay; no-op when nothing changed
        elif self._hyper_snapshot() != self._baked:
            raise RuntimeError("GraphedTrainStep: the optimizer's hyper-parameters changed since the capture "
                               f"({self._baked} -> {self._hyper_snapshot()}) and this optimizer bakes them into the captured "
                               "kernels; use yolo_for_turbines_amd.SGD, Adam or AdamW (they read them from device memory at every replay) or "
                               "capture a new GraphedTrainStep")
        self.x.copy_(x, non_blocking=True)
        for dst, src in zip(self.targets, targets):
            dst.copy_(src, non_blocking=True)
        self.graph.replay()
        # the replay rewrote every parameter and BatchNorm statistic without dispatching a torch op: version counters did
        # not move, so every packed weight / BN fold cached for eval is stale by construction
        self.model._engine.invalidate()
        if self.ema is not None and hasattr(self.ema.module, "_engine"):
            self.ema.module._engine.invalidate()        # the averaged tensors were rewritten the same way
        if hasattr(self.opt, "forget_uploads"):
            self.opt.forget_uploads()                   # and the device row tables of `yt.SGD` hold the captured step's rows
        return self.loss

    def release(self):
        """Give the pinned plan back to the model's LRU (its memory is freed once evicted and the graph is dropped)."""
        self._plan.pinned = False
        self.graph = None
