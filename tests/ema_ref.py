"""Reference of the weight average (`yolo_for_turbines_amd/ema.py`, `csrc/optim.hip`) in plain torch: the contract, nothing else.

    d   = min(decay, float32(1 + t) / float32(10 + t)) if warmup else decay      numpy.float32 arithmetic
    e   = e.mul_(d).add_(p, alpha=1 - d)                                          on whichever device the tensors live
    integer entries are copied;  t += 1
"""
import numpy as np
import torch


def coeffs(t, decay, warmup):
    """(d, 1 - d) of update number ``t`` (0-based) as Python floats that are exact fp32 values."""
    d = np.float32(decay)
    if warmup:
        d = min(d, np.float32(1 + t) / np.float32(10 + t))
    omd = np.float32(1.0) - d
    assert d.dtype == np.float32 and omd.dtype == np.float32
    return float(d), float(omd)


class EmaRef:
    """``shadow``: dict name -> tensor (clones of the source at construction); ``update(source)`` moves it."""

    def __init__(self, source, decay=0.9998, warmup=True):
        self.decay, self.warmup, self.updates = decay, warmup, 0
        self.shadow = {k: v.detach().clone() for k, v in source.items()}

    @torch.no_grad()
    def update(self, source):
        d, omd = coeffs(self.updates, self.decay, self.warmup)
        for k, e in self.shadow.items():
            p = source[k].detach()
            if e.dtype.is_floating_point:
                e.mul_(d).add_(p, alpha=omd)
            else:
                e.copy_(p)
        self.updates += 1
