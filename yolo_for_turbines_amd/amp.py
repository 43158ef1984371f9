"""fp16 loss scaling that never waits for the host (`csrc/optim.hip`: check launch + scaled SGD step).

The reference trains in fp16 autocast through a `GradScaler` (`code/train.py:39,53,67-69`). `torch.amp.GradScaler.step`
unscales every gradient in place (a read and a write of all of them) and then calls `found_inf.item()`: the host waits for
the device in the middle of the step, and the step cannot be captured in a HIP graph. :class:`GradScaler` here keeps
PyTorch's scale arithmetic (`torch._amp_update_scale_`, one device-side kernel) and replaces the rest for a
:class:`yolo_for_turbines_amd.SGD`: one launch reads the gradients and raises a device flag, the SGD launch reads the flag
and the scale, unscales in registers and does nothing when the flag is set. Same bits as `torch.amp.GradScaler` +
`torch.optim.SGD` after every step, skipped steps included. :class:`yolo_for_turbines_amd.Adam` and ``AdamW`` take the same
path (their step count is a device word that a skipped step leaves alone).

This module is the one place that leans on private members of `torch.amp.GradScaler` (`_per_optimizer_states`, `OptState`,
`_check_scale_growth_tracker`; PyTorch 2.10); `tests/test_gpu_amp.py` pins the behaviour.
"""
import torch
from torch.amp.grad_scaler import OptState

from .optim import NativeOptimizer


class GradScaler(torch.amp.GradScaler):
    """Drop-in for ``torch.amp.GradScaler`` (same constructor, ``state_dict()``, ``get_scale()``; ``scale()``,
    ``unscale_()`` and ``update()`` are inherited)::

        scaler.scale(loss).backward()
        scaler.step(optimizer)          # yt.SGD / Adam / AdamW: check launch + scaled step, no host wait; anything else: PyTorch's path
        scaler.update()

    After a native ``step`` the ``.grad`` tensors still hold the SCALED gradients (PyTorch's ``step`` leaves them unscaled):
    the unscale happens in registers and is not written back. Call ``unscale_(optimizer)`` first to get unscaled gradients
    in memory; ``step`` then uses them as they are. Clipping needs neither: ``yt.SGD(max_grad_norm=...)`` takes the norm in
    the same read as the non-finite check and clips in registers. A skipped step still skips on the device, so
    ``step`` always returns ``None`` for a native optimizer and never reports whether it was applied.
    """

    def __init__(self, device="cuda", init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000,
                 enabled=True):
        super().__init__(device, init_scale=init_scale, growth_factor=growth_factor, backoff_factor=backoff_factor,
                         growth_interval=growth_interval, enabled=enabled)
        self._native_flags = {}          # id(optimizer) -> its found_inf word: one address for every step, so a capture can hold it

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled or not isinstance(optimizer, NativeOptimizer):
            return super().step(optimizer, *args, **kwargs)
        if "closure" in kwargs or args:
            raise RuntimeError("Closure use is not currently supported if GradScaler is enabled.")
        scale, _ = self._check_scale_growth_tracker("step")
        state = self._per_optimizer_states[id(optimizer)]
        if state["stage"] is OptState.STEPPED:
            raise RuntimeError("step() has already been called since the last update().")
        if state["stage"] is OptState.READY:
            flag = self._native_flags.get(id(optimizer))
            if flag is None or flag.device != scale.device:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("yolo_for_turbines_amd.GradScaler: take one eager step before capturing")
                flag = self._native_flags[id(optimizer)] = torch.zeros((), dtype=torch.float32, device=scale.device)
            state["found_inf_per_device"] = {scale.device: flag}        # what update() reads
            optimizer.grad_scale, optimizer.found_inf, check = scale, flag, flag
        else:                                                           # UNSCALED: unscale_() has checked and unscaled already
            found = list(state["found_inf_per_device"].values())
            assert found, "No inf checks were recorded for this optimizer."
            flag = found[0] if len(found) == 1 else sum(t.to(scale.device, non_blocking=True) for t in found)
            optimizer.grad_scale, optimizer.found_inf, check = None, flag, None
        try:
            optimizer.step(check_into=check)
        finally:
            del optimizer.grad_scale, optimizer.found_inf
        state["stage"] = OptState.STEPPED
        return None
