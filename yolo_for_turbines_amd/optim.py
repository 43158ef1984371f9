"""SGD step of the fine-tune loop as one HIP launch (`csrc/optim.hip`).

Drop-in for `torch.optim.SGD` as the reference constructs it (`code/train.py:171-172`:
`SGD(model.parameters(), lr, momentum, weight_decay)`, stepped at `:68` through the GradScaler): same constructor,
same `state` / `state_dict()` layout (`momentum_buffer` per parameter, so `utils.py:383-416` checkpoints load
either way), same bits after every step. Only fp32 parameters on the GPU (what the model holds); anything
else raises instead of falling back.

Under a loss scale (`yolo_for_turbines_amd.GradScaler`, or anything that sets the two tensor attributes PyTorch's fused
optimizers use, `optimizer.grad_scale` and `optimizer.found_inf`) the step unscales in registers and is skipped on the device
when `found_inf` is set: no host wait, capturable. Whether a momentum buffer has been written yet is then a device fact
(a skipped first step leaves it unwritten), kept as one int32 word per parameter next to the tables.

With a weight average attached (`ema.ModelEMA.attach`) the same launch also moves the average of every parameter it updates
(the `_ema` entry points); without one the step is the launches it always was.
"""
import torch

from . import _lib as L


class _GroupTable:
    """What one parameter group needs for its launch: the chunk table (built once: tensor sizes never change) and the
    pointer table, which travels host -> device asynchronously every step."""

    def __init__(self, params):
        dev = params[0].device
        ce = L.lib().yolo_sgd_chunk_elems()
        chunks = []
        for i, p in enumerate(params):
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.device == dev):
                raise TypeError("yolo_for_turbines_amd.optim.SGD: parameters must be contiguous fp32 tensors on one GPU")
            chunks += [(i, s) for s in range(0, p.numel(), ce)]
        self.params = list(params)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev)
        self.items = torch.empty((len(params), 4), dtype=torch.int64, device=dev)
        # eager steps: a ring of pinned buffers, each guarded by the event of its last copy, so the host (which runs ahead of
        # the GPU) never rewrites a table the GPU has not read yet
        self.ring = [[self._pinned(), None] for _ in range(3)]
        self.next_slot = 0
        self.uploaded = None                                # host copy of the row table the device holds (None: unknown)
        # captures: a captured copy reads its pinned source at every replay, so each capture gets a buffer nothing else will
        # ever write; pinned memory cannot be allocated inside a capture, so eager steps keep two spares ready
        self.spares = []
        self.captured = []
        # {lr, momentum, dampening, weight_decay} live in DEVICE memory and the kernel reads them when it runs: a step
        # captured in a HIP graph then follows the LR scheduler (train.py:71-74 steps LinearLR after every batch) instead of
        # replaying the capture-time values. Written stream-ordered, outside any capture, whenever the group's values change
        # (SGD.sync_hyper); pinned staging ring guarded by events like the row tables.
        self.hyper = torch.zeros(4, dtype=torch.float32, device=dev)
        self.hyper_host = None                              # the values last pushed
        self.hyper_ring = [[torch.zeros(4, dtype=torch.float32).pin_memory(), None] for _ in range(4)]
        self.hyper_slot = 0
        # loss-scaled steps: written[i] != 0 once parameter i's momentum buffer holds a value (set on the device after an
        # applied step; SGD._table fills it in for buffers the host knows about). device_first: some buffer of this group was
        # allocated by a loss-scaled step, so only the device knows whether it was written - every later step of the group
        # then goes through the kernel that reads the words.
        self.written = torch.zeros(len(params), dtype=torch.int32, device=dev)
        self.device_first = False
        self.no_inf = torch.zeros(1, dtype=torch.float32, device=dev)
        # weight average (ema.ModelEMA.attach): one float* per parameter, the averaged tensor the step moves along with it
        # (0: none). The averaged tensors never move, so this is uploaded once per (table, average).
        self.shadows = None
        self.shadows_of = None

    def _pinned(self):
        return torch.zeros((len(self.params), 4), dtype=torch.int64).pin_memory()

    def matches(self, params):
        return len(self.params) == len(params) and all(a is b for a, b in zip(self.params, params))

    def push_hyper(self, values):
        """Enqueue {lr, momentum, dampening, weight_decay} -> device on the current stream if they changed."""
        if values == self.hyper_host:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("yolo_for_turbines_amd.optim.SGD: the hyper-parameters changed inside a stream capture; call "
                               "optimizer.sync_hyper() (GraphedTrainStep does) before the replay instead")
        slot = self.hyper_ring[self.hyper_slot]
        self.hyper_slot = (self.hyper_slot + 1) % len(self.hyper_ring)
        if slot[1] is not None:
            slot[1].synchronize()
        h = slot[0]
        h[0], h[1], h[2], h[3] = values
        self.hyper.copy_(h, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        self.hyper_host = values

    def host_buffer(self, capturing):
        """(pinned buffer to fill, ring slot or None)."""
        if capturing:
            if not self.spares:
                raise RuntimeError("yolo_for_turbines_amd.optim.SGD: take one eager step before capturing")
            host = self.spares.pop()
            self.captured.append(host)
            return host, None
        while len(self.spares) < 2:
            self.spares.append(self._pinned())
        slot = self.ring[self.next_slot]
        self.next_slot = (self.next_slot + 1) % len(self.ring)
        if slot[1] is not None:
            slot[1].synchronize()
        return slot[0], slot


class SGD(torch.optim.SGD):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        # foreach / fused select among PyTorch's own implementations: accepted for signature compatibility, irrelevant here
        if differentiable:
            raise ValueError("yolo_for_turbines_amd.optim.SGD: differentiable=True is not supported")
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize)
        self._tables = {}                                   # group index -> _GroupTable
        self._word = {}                                     # parameter -> its 1-element view of a table's `written`
        self._ema = None                                    # ema.ModelEMA.attach: step() moves that average in its own launch

    def _table(self, gi, params):
        t = self._tables.get(gi)
        if t is None or not t.matches(params):
            old = t
            t = self._tables[gi] = _GroupTable(params)
            # A buffer this optimizer has no word for came from a plain step or from load_state_dict: it is written. One the
            # device decides about (allocated by a loss-scaled step) keeps its word across a rebuild of the table.
            known = [int(p not in self._word and self.state.get(p, {}).get("momentum_buffer") is not None) for p in params]
            t.written.copy_(torch.tensor(known, dtype=torch.int32))
            for i, p in enumerate(params):
                if p in self._word:
                    t.written[i:i + 1].copy_(self._word[p])
                self._word[p] = t.written[i:i + 1]
            t.device_first = old is not None and old.device_first
        return t

    def _unwritten(self):
        """Parameters whose momentum buffer exists but has never been written (every loss-scaled step so far was skipped).
        Reads device memory, so it waits for the device: for checkpointing, not for the step."""
        out = set()
        for tab in self._tables.values():
            if tab.device_first:
                w = tab.written.cpu()
                out.update(p for i, p in enumerate(tab.params) if not int(w[i]) and "momentum_buffer" in self.state.get(p, {}))
        return out

    def state_dict(self):
        """`torch.optim.SGD.state_dict()`; a momentum buffer that was allocated but never written (the steps so far were all
        skipped by the loss scaler) is left out, which is PyTorch's meaning of "no buffer yet"."""
        sd = super().state_dict()
        skip = self._unwritten()
        if skip:
            index, n = {}, 0
            for group in self.param_groups:
                for p in group["params"]:
                    if id(p) not in index:
                        index[id(p)] = n
                        n += 1
            for p in skip:
                entry = {k: v for k, v in sd["state"][index[id(p)]].items() if k != "momentum_buffer"}
                if entry:
                    sd["state"][index[id(p)]] = entry
                else:
                    del sd["state"][index[id(p)]]
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # the "written" word of every parameter follows from whether a buffer came with the checkpoint (the tables stay: their
        # device memory may be part of a captured graph)
        for tab in self._tables.values():
            known = [int(self.state.get(p, {}).get("momentum_buffer") is not None) for p in tab.params]
            tab.written.copy_(torch.tensor(known, dtype=torch.int32))
            tab.device_first = False

    @staticmethod
    def _hyper_of(group):
        mom, damp = float(group["momentum"]), float(group["dampening"])
        if group["nesterov"] and (mom <= 0.0 or damp != 0.0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        return (float(group["lr"]), mom, damp, float(group["weight_decay"]))

    def sync_hyper(self):
        """Push every group's current {lr, momentum, dampening, weight_decay} to the device (stream-ordered, a no-op when
        nothing changed). `step()` does this itself in eager mode; call it before replaying a HIP graph that captured
        `step()` whenever an LR scheduler (train.py:71-74,187-189) or the user changed `param_groups` in between."""
        for gi, group in enumerate(self.param_groups):
            tab = self._tables.get(gi)
            if tab is not None:
                tab.push_hyper(self._hyper_of(group))

    def _prepare(self, gi, group, scaled):
        """Fill and (if it changed) upload the row table of one group for the gradients as they are now. Returns
        (table, indices of momentum buffers the host marked new, parameters this step updates)."""
        tab = self._table(gi, group["params"])
        mom = float(group["momentum"])
        capturing = torch.cuda.is_current_stream_capturing()
        hyper = self._hyper_of(group)
        if capturing and tab.hyper_host is None:
            raise RuntimeError("yolo_for_turbines_amd.optim.SGD: take one eager step before capturing")
        if not capturing or hyper != tab.hyper_host:      # inside a capture an unchanged value needs no node at all
            tab.push_hyper(hyper)
        scaled = scaled or tab.device_first
        if self._ema is not None and tab.shadows_of is not self._ema:
            if capturing:
                raise RuntimeError("yolo_for_turbines_amd.optim.SGD: take one eager step before capturing (the first step with a "
                                   "weight average attached uploads its pointer table)")
            tab.shadows = torch.tensor([L.ptr(self._ema.shadow_of(p)) for p in tab.params], dtype=torch.int64).to(tab.items.device)
            tab.shadows_of = self._ema
        host, slot = tab.host_buffer(capturing)
        rows = host.numpy()                              # [p, g, momentum buffer, n] per parameter (yolo_sgd_item)
        updated, fresh = [], []
        for i, p in enumerate(tab.params):
            g = p.grad
            if g is None:
                rows[i, 1] = 0                           # skipped by the kernel, like PyTorch
                continue
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device:
                raise TypeError("yolo_for_turbines_amd.optim.SGD: gradients must be dense contiguous fp32 on the parameter's GPU")
            n = p.numel()
            rows[i, 0] = p.data_ptr()
            rows[i, 1] = g.data_ptr()
            if mom != 0.0:
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if buf is None:
                    if capturing:
                        raise RuntimeError("yolo_for_turbines_amd.optim.SGD: take one eager step before capturing (the first step "
                                           "initialises the momentum buffers)")
                    if scaled:                           # whether this step writes it is decided on the device
                        buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        tab.device_first = True
                    else:
                        buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        n = -n                           # first step: the kernel writes buf = g + wd * p
                        fresh.append(i)
                rows[i, 2] = buf.data_ptr()
            else:
                rows[i, 2] = p.data_ptr()                # never touched
            rows[i, 3] = n
            updated.append(p)
        # the kernel writes through raw pointers: tell PyTorch's version counters (the engine re-packs a weight when its
        # version moves - without this the forward would keep using the weights of step 0)
        torch.autograd.graph.increment_version(updated)
        # With gradient buckets / a captured graph every address is the same step after step: upload the table only when it
        # differs from the one the device already holds (an H2D copy costs the GPU ~85 us of idle queue in front of it)
        same = (not capturing) and tab.uploaded is not None and bool((rows == tab.uploaded).all())
        if not same:
            tab.items.copy_(host, non_blocking=True)
            tab.uploaded = None if capturing else rows.copy()
            if slot is not None:
                slot[1] = torch.cuda.Event()
                slot[1].record()
        return tab, fresh, updated

    @staticmethod
    def _flag(t, dev, what):
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.numel() == 1):
            raise TypeError(f"yolo_for_turbines_amd.optim.SGD: {what} must be a one-element fp32 tensor on the parameters' GPU")
        return t

    @torch.no_grad()
    def step(self, closure=None, *, check_into=None):
        """One launch per parameter group. With the tensor attributes ``self.grad_scale`` / ``self.found_inf`` set (what
        ``GradScaler.step`` hands PyTorch's fused optimizers) the gradients are unscaled in registers (``p.grad`` keeps the
        scaled values) and nothing is touched when ``found_inf`` is non-zero; without them nothing changes. ``check_into``
        (one fp32 element on the GPU): first run the non-finite check over every group's gradients into it. With a weight
        average attached (``ModelEMA.attach``) the same launches also move the average of every parameter they update; one
        more launch does the entries left over (BatchNorm statistics, parameters without a gradient) and counts the update."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.lib()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        scaled = grad_scale is not None or found_inf is not None
        groups = [(gi, g) for gi, g in enumerate(self.param_groups) if g["params"]]
        ready = [(g,) + self._prepare(gi, g, scaled) for gi, g in groups]
        if check_into is not None:                           # every group is checked before any group is stepped
            self._check(ready, check_into)
        ema = self._ema
        if ema is not None:                                  # what these launches leave over, decided (and uploaded) before them
            rest = ema._rest({id(p) for r in ready for p in r[3]})
        # with a weight average attached: the `_ema` twins of the two entry points, which take {shadow table, EMA state} too
        step_amp, step_hp = (lib.yolo_sgd_step_amp, lib.yolo_sgd_step_hp) if ema is None else (lib.yolo_sgd_step_amp_ema, lib.yolo_sgd_step_hp_ema)
        for group, tab, fresh, _ in ready:
            dev = tab.hyper.device
            nest, maxi = int(bool(group["nesterov"])), int(bool(group["maximize"]))
            avg = () if ema is None else (tab.shadows.data_ptr(), ema._state.data_ptr())
            what = "yolo_sgd_step" + ("_amp" if scaled or tab.device_first else "_hp") + ("" if ema is None else "_ema")
            if scaled or tab.device_first:
                flag = self._flag(found_inf, dev, "found_inf")
                L.check(step_amp(tab.items.data_ptr(), len(tab.params), tab.chunks.data_ptr(), tab.chunks.shape[0], tab.hyper.data_ptr(),
                                 L.ptr(self._flag(grad_scale, dev, "grad_scale")), (flag if flag is not None else tab.no_inf).data_ptr(),
                                 tab.written.data_ptr(), *avg, nest, maxi, L.current_stream()), what)
                continue
            L.check(step_hp(tab.items.data_ptr(), tab.chunks.data_ptr(), tab.chunks.shape[0], tab.hyper.data_ptr(), *avg, nest, maxi,
                            L.current_stream()), what)
            if len(fresh) == len(tab.params):                # the host marked these buffers new and this step wrote them
                tab.written.fill_(1)
            else:
                for i in fresh:
                    tab.written[i:i + 1].fill_(1)
        if ema is not None:                                  # the entries left over, then the counter; both skipped with the step
            ema._finish(rest, self._flag(found_inf, rest.rows.device, "found_inf"))
        return loss

    def _check(self, ready, found_inf):
        lib = L.lib()
        if not ready:
            found_inf.zero_()
        for k, (_, tab, _, _) in enumerate(ready):
            L.check(lib.yolo_sgd_check_finite(tab.items.data_ptr(), tab.chunks.data_ptr(), tab.chunks.shape[0],
                                              self._flag(found_inf, tab.hyper.device, "found_inf").data_ptr(), int(k == 0),
                                              L.current_stream()), "yolo_sgd_check_finite")
