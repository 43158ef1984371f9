"""Reference of the Adam / AdamW step (`yolo_for_turbines_amd/optim.py`, `csrc/optim_adam.hip`): the contract, nothing else.

The contract is `torch.optim.Adam` / `AdamW` in the mode PyTorch picks by default on the GPU (foreach, not capturable, not
fused): per-step scalars formed in Python doubles on the host, then nine elementwise passes. ``words`` are those scalars as the
fp32 values the passes receive; ``torch_chain`` is the passes written with the plain torch ops (`tests/test_adam_host.py` pins
it to the installed PyTorch bit for bit).
"""
import numpy as np
import torch


def words(t, lr, betas, eps, wd):
    """The seven fp32 words of step number ``t`` (1-based), each a Python-double expression cast once:
    (1 - lr*wd, 1 - beta1, beta2, 1 - beta2, eps, (1 - beta2**t) ** 0.5, (lr / (1 - beta1**t)) * -1)."""
    beta1, beta2 = betas
    t = float(t)                                             # PyTorch keeps the count as a float tensor and takes .item()
    bc1 = 1 - beta1 ** t
    bc2 = 1 - beta2 ** t
    return np.array([1 - lr * wd, 1 - beta1, beta2, 1 - beta2, eps, bc2 ** 0.5, (lr / bc1) * -1], dtype=np.float64).astype(np.float32)


@torch.no_grad()
def torch_chain(p, g, m, v, t, lr, betas, eps, wd, decoupled, maximize):
    """One step on ``p``, ``m`` (exp_avg) and ``v`` (exp_avg_sq) in place; ``g`` is left alone. ``t``: this step's number."""
    beta1, beta2 = betas
    if maximize:
        g = g.neg()                                          # 1
    if wd != 0:
        if decoupled:
            p.mul_(1 - lr * wd)                              # 2a
        else:
            g = g.add(p, alpha=wd)                           # 2b
    m.lerp_(g, 1 - beta1)                                    # 3
    v.mul_(beta2)                                            # 4
    v.addcmul_(g, g, value=1 - beta2)                        # 5
    d = v.sqrt()                                             # 6
    d.div_((1 - beta2 ** float(t)) ** 0.5)                   # 7
    d.add_(eps)                                              # 8
    p.addcdiv_(m, d, value=(lr / (1 - beta1 ** float(t))) * -1)   # 9
