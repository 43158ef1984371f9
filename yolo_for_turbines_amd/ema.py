"""Weight average of the fine-tune loop: an exponential moving average (EMA) of every parameter and BatchNorm statistic,
evaluated and saved in place of the raw weights (`csrc/optim.hip`).

The reference keeps no average; where one would sit it has `best_model = model` (`code/train.py:219`), an alias of the live
model, so its "best" checkpoint is whatever the last step left behind. :class:`ModelEMA` is the usual remedy, with three
properties the foreach form (`torch._foreach_mul_` + `torch._foreach_add_` over the state) does not have:

* attached to a :class:`yolo_for_turbines_amd.SGD` it moves in the SAME launch as the step, which holds the new parameter value
  in a register anyway: 8 more bytes per element on top of 20, instead of two more passes over everything;
* the decay is computed on the device from a device counter, so a step captured in a HIP graph (``GraphedTrainStep(...,
  ema=ema)``) follows the warm-up of the decay through its replays, and a step the loss scaler skipped is not counted;
* the averaged model's packed-weight cache is kept coherent (version counters eagerly, ``invalidate()`` after a replay).

Arithmetic (fp32, the same bits as ``e.mul_(d).add_(p, alpha=1 - d)`` on the GPU), ``t`` = updates applied so far::

    d = min(decay, float32(1 + t) / float32(10 + t)) if warmup else decay
    e = fma(1 - d, p, e * d)            # every floating-point entry of model.state_dict(); integer entries are copied
    t += 1

Frozen parameters and parameters without a gradient are averaged like the rest: every float entry, every update.
"""
import copy

import numpy as np
import torch

from . import _lib as L

_WHO = "yolo_for_turbines_amd.ModelEMA"


class _RowTable:
    """Device tables of one standalone launch over a fixed set of entries: chunks once, (src, dst, n) rows whenever an
    address moved. A row upload is a plain blocking copy: it happens on the first step and after a re-allocation, never in
    the steady state, and never inside a capture."""

    def __init__(self, counts, dev):
        ce = L.lib().yolo_sgd_chunk_elems()
        chunks = [(i, s) for i, n in enumerate(counts) for s in range(0, abs(n), ce)]
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev)
        self.rows = torch.zeros((len(counts), 3), dtype=torch.int64, device=dev)
        self.host = np.zeros((len(counts), 3), dtype=np.int64)
        self.host[:, 2] = counts
        self.uploaded = None

    def sync(self, srcs, dsts):
        for i, (s, d) in enumerate(zip(srcs, dsts)):
            self.host[i, 0] = s.data_ptr()
            self.host[i, 1] = d.data_ptr()
        if self.uploaded is None or not np.array_equal(self.host, self.uploaded):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{_WHO}: take one eager step before capturing")
            self.rows.copy_(torch.from_numpy(self.host))
            self.uploaded = self.host.copy()


class ModelEMA:
    """``ema = ModelEMA(model, decay=0.9998, warmup=True)``::

        ema.attach(optimizer)      # yt.SGD / Adam / AdamW: optimizer.step() now also moves the average, in the same launch
        ema.update()               # any other optimizer: one standalone launch after optimizer.step()
        ema.module                 # a model in eval mode whose parameters and buffers ARE the averaged tensors
        ema.updates                # updates applied so far (reads the device word: waits for the device)

    ``ema.module`` goes wherever a model goes (``detect_images``, ``evaluate_model``, ``save_checkpoint``, ``save_weights``).
    Under a loss scale a skipped step leaves the average and the counter untouched. Only contiguous fp32 entries on one GPU;
    anything else raises ``TypeError``. Data parallel: every rank holds the same parameters after the all-reduce and so
    computes the same average without any communication; rank 0's ``ema.module`` is the one to save.
    """

    def __init__(self, model, decay=0.9998, warmup=True):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"{_WHO}: decay must be in [0, 1), got {decay}")
        src = model.state_dict(keep_vars=True)
        if not src:
            raise TypeError(f"{_WHO}: the model has no state")
        dev = next(iter(src.values())).device
        for k, v in src.items():
            if not v.is_cuda or v.device != dev:
                raise TypeError(f"{_WHO}: every parameter and buffer must live on one GPU ({k} is on {v.device}; there is no CPU path)")
            if not v.is_contiguous():
                raise TypeError(f"{_WHO}: {k} is not contiguous")
            if v.dtype.is_floating_point or v.dtype.is_complex:
                if v.dtype != torch.float32:
                    raise TypeError(f"{_WHO}: floating-point entries must be fp32 ({k} is {v.dtype})")
            elif (v.numel() * v.element_size()) % 4:
                raise TypeError(f"{_WHO}: integer entry {k} is not a whole number of 32-bit words")
        self.decay, self.warmup = decay, bool(warmup)
        self.module = self._twin(model, dev)
        self.module.load_state_dict({k: v.detach() for k, v in src.items()})
        self.module.eval().requires_grad_(False)
        dst = self.module.state_dict(keep_vars=True)
        assert list(dst) == list(src)
        self._names = list(src)
        self._src, self._dst = list(src.values()), [dst[k] for k in src]
        # per entry: number of floats to average, or minus the number of 32-bit words to copy
        self._count = [v.numel() if v.dtype == torch.float32 else -(v.numel() * v.element_size() // 4) for v in self._src]
        self._index = {id(v): i for i, v in enumerate(self._src)}
        # yolo_ema_state: {updates, decay, warmup, reserved}, read by the kernels when they run
        self._state = torch.zeros(4, dtype=torch.int32, device=dev)
        self._push_state(0)
        self._tables = {}                                   # tuple of entry indices -> _RowTable
        self._attached = None

    @staticmethod
    def _twin(model, dev):
        from .model import YOLOv3
        if isinstance(model, YOLOv3):
            # the constructor and a fresh engine.ModelState, not a deep copy of a model whose engine owns plans and buffers
            return type(model)(in_channels=model.in_channels, num_classes=model.num_classes, activation=model.activation).to(dev)
        return copy.deepcopy(model)

    def _push_state(self, updates):
        words = np.zeros(4, dtype=np.int32)
        words[0] = updates
        words[1:2] = np.array([self.decay], dtype=np.float32).view(np.int32)
        words[2] = int(self.warmup)
        self._state.copy_(torch.from_numpy(words))

    # ------------------------------------------------------------------------------------------------- the optimizer's side
    def shadow_of(self, p):
        """The averaged tensor of parameter ``p`` of the model (None: not one of its entries)."""
        i = self._index.get(id(p))
        return None if i is None else self._dst[i]

    def _rest(self, done):
        """Tables for every entry whose tensor is not in ``done`` (ids of the parameters the fused step covers), addresses
        checked and uploaded if they moved. Called before the step's launches, like the optimizer's own tables."""
        key = tuple(i for i, v in enumerate(self._src) if id(v) not in done)
        tab = self._tables.get(key)
        if tab is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{_WHO}: take one eager step before capturing")
            # one table per distinct set of entries (a few KB), kept for good: a captured graph may point at any of them
            tab = self._tables[key] = _RowTable([self._count[i] for i in key], self._state.device)
        tab.sync([self._src[i] for i in key], [self._dst[i] for i in key])
        return tab

    def _finish(self, tab, found_inf=None):
        """The standalone launch over ``tab`` and the advance of the counter, both skipped on the device when ``found_inf``
        is set. The launch wrote through raw pointers: move the version counters (the engine re-packs a weight when its
        version moves)."""
        L.check(L.lib().yolo_ema_update(tab.rows.data_ptr(), tab.chunks.data_ptr(), tab.chunks.shape[0], self._state.data_ptr(),
                                        L.ptr(found_inf), 1, L.current_stream()), "yolo_ema_update")
        torch.autograd.graph.increment_version(self._dst)

    # ------------------------------------------------------------------------------------------------------ the user's side
    def attach(self, optimizer):
        """Let ``optimizer.step()`` (a :class:`yolo_for_turbines_amd.SGD`, ``Adam`` or ``AdamW``) move the average: parameters with a gradient in the
        step's own launch, everything else in one more."""
        from .optim import NativeOptimizer
        if not isinstance(optimizer, NativeOptimizer):
            raise TypeError(f"{_WHO}.attach needs a yolo_for_turbines_amd.SGD, Adam or AdamW; call update() after the step of any other "
                            "optimizer")
        if self._attached is not None and self._attached is not optimizer:
            raise RuntimeError(f"{_WHO}: already attached to another optimizer")
        if getattr(optimizer, "_ema", None) not in (None, self):
            raise RuntimeError(f"{_WHO}: the optimizer already carries another average")
        optimizer._ema = self
        self._attached = optimizer
        return self

    def detach(self):
        if self._attached is not None:
            self._attached._ema = None
            self._attached = None

    @torch.no_grad()
    def update(self):
        """One standalone launch over every entry (for optimizers other than the native ones)."""
        if self._attached is not None:
            raise RuntimeError(f"{_WHO}.update(): attached to an optimizer whose step() already moves the average; calling "
                               "update() as well would average twice")
        self._finish(self._rest(()))

    @property
    def updates(self):
        return int(self._state[0].item())

    def state_dict(self):
        return {"module": self.module.state_dict(), "updates": self.updates, "decay": self.decay, "warmup": self.warmup}

    def load_state_dict(self, sd):
        decay = float(sd["decay"])
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"{_WHO}: decay must be in [0, 1), got {decay}")
        self.module.load_state_dict(sd["module"])           # copies in place: the averaged tensors keep their addresses
        self.decay, self.warmup = decay, bool(sd["warmup"])
        self._push_state(int(sd["updates"]))
