"""CPU checks of the Adam / AdamW contract (`tests/adam_ref.py`) and of what `yt.Adam` / `yt.AdamW` refuse at construction.
`torch_chain` stepped by hand must give the bits of `torch.optim.Adam` / `AdamW` (``foreach=True``) on the same machine: that pins
the written-down chain, and the Python-double scalars of `words`, to the installed PyTorch."""
import numpy as np
import pytest
import torch

from tests import adam_ref
from tests.test_gpu_ema import SHAPES

CFGS = [("Adam", dict(lr=1e-3)), ("Adam", dict(lr=1e-3, weight_decay=5e-4)), ("AdamW", dict(lr=1e-3, weight_decay=0.05)),
        ("AdamW", dict(lr=2e-3, weight_decay=0.05, maximize=True)), ("Adam", dict(lr=1e-3, betas=(0.4, 0.9))),
        ("AdamW", dict(lr=1e-3, eps=1e-3, weight_decay=0.01))]


def _bag():
    """The parameter set of `tests/test_gpu_ema.py::Bag` on the CPU (same seeds, the view one element into its allocation)."""
    ps = [torch.randn(s, generator=torch.Generator().manual_seed(i)) for i, s in enumerate(SHAPES)]
    ps.append(torch.randn(1031, generator=torch.Generator().manual_seed(5))[1:])
    return ps


def _grad(i, step, shape):
    """The gradient pattern of `_set_grads` there: parameter 2 never gets one, parameter 4 from the third step on."""
    if i == 2 or (i == 4 and step < 2):
        return None
    return torch.randn(shape, generator=torch.Generator().manual_seed(100 * step + i))


@pytest.mark.parametrize("name,cfg", CFGS)
def test_chain_by_hand_is_torch_adam_bit_for_bit(name, cfg):
    ps = [torch.nn.Parameter(p.clone()) for p in _bag()]
    opt = getattr(torch.optim, name)(ps, foreach=True, **cfg)
    hand = [p.clone() for p in _bag()]
    ms, vs, ts = [torch.zeros_like(p) for p in hand], [torch.zeros_like(p) for p in hand], [0] * len(hand)
    betas, eps, wd = cfg.get("betas", (0.9, 0.999)), cfg.get("eps", 1e-8), cfg.get("weight_decay", 0.01 if name == "AdamW" else 0.0)
    for step in range(6):
        lr = cfg["lr"] * (1.0 - 0.1 * step)                              # moves every step, as under LinearLR
        opt.param_groups[0]["lr"] = lr
        for i, p in enumerate(ps):
            g = _grad(i, step, p.shape)
            p.grad = g
            if g is not None:
                ts[i] += 1
                adam_ref.torch_chain(hand[i], g.clone(), ms[i], vs[i], ts[i], lr, betas, eps, wd, name == "AdamW", cfg.get("maximize", False))
        opt.step()
        for i, p in enumerate(ps):
            assert torch.equal(p.detach(), hand[i]), (step, i)
            st = opt.state.get(p, {})
            assert int(st["step"]) == ts[i] if st else ts[i] == 0, (step, i)
            if st:
                assert torch.equal(st["exp_avg"], ms[i]) and torch.equal(st["exp_avg_sq"], vs[i]), (step, i)
    assert ts[2] == 0 and ts[4] == 4 and ts[0] == 6


def test_words_are_the_python_double_expressions():
    w = adam_ref.words(3, 1e-3, (0.9, 0.999), 1e-8, 0.05)
    assert w.dtype == np.float32 and w.shape == (7,)
    want = [1 - 1e-3 * 0.05, 1 - 0.9, 0.999, 1 - 0.999, 1e-8, (1 - 0.999 ** 3.0) ** 0.5, (1e-3 / (1 - 0.9 ** 3.0)) * -1]
    assert w.tolist() == [float(np.float32(x)) for x in want]
    assert adam_ref.words(1, 3e-4, (0.4, 0.9), 1e-8, 0.0)[0] == 1.0


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_constructor_refusals(name):
    import yolo_for_turbines_amd as yt
    cls = getattr(yt, name)
    assert issubclass(cls, getattr(torch.optim, name)) and name in yt.__all__
    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="amsgrad"):
        cls(ps, amsgrad=True)
    with pytest.raises(ValueError, match="differentiable"):
        cls(ps, differentiable=True)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="maximal norm"):
            cls(ps, max_grad_norm=bad)
    with pytest.raises(ValueError, match="norm_type"):
        cls(ps, max_grad_norm=1.0, grad_norm_type=3)
    opt = cls(ps, lr=1e-3, foreach=True, fused=False, capturable=True, max_grad_norm=2.0)          # accepted, irrelevant here
    group = opt.param_groups[0]
    assert group["decoupled_weight_decay"] == (name == "AdamW") and group["weight_decay"] == (0.01 if name == "AdamW" else 0.0)
    assert opt.max_grad_norm == 2.0 and opt.state_dict()["state"] == {}
