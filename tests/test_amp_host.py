"""Host tests (no GPU) of the loss-scaling surface: the new C entry points are declared, exported and bound, and
``yt.GradScaler`` hands every optimizer that is not a ``yt.SGD`` to PyTorch's own ``step``."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_amp_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    for name in ("yolo_sgd_check_finite", "yolo_sgd_step"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    # argument errors come back as codes, never as a launch
    assert _lib.lib().yolo_sgd_check_finite(None, None, 1, None, 1, None) < 0
    assert b"sgd_check_finite" in _lib.lib().yolo_last_error()
    assert _lib.lib().yolo_sgd_step(None, 1, None, 1, None, None, None, None, None, None, None, 0, 0, None) < 0    # NULL tables
    assert b"sgd_step" in _lib.lib().yolo_last_error()


def test_grad_scaler_falls_back_to_pytorch_for_other_optimizers():
    import yolo_for_turbines_amd as yt
    assert issubclass(yt.GradScaler, torch.amp.GradScaler)
    scaler = yt.GradScaler("cpu", enabled=False)
    p = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.SGD([p], lr=0.5)
    p.grad = torch.ones(3)
    assert scaler.scale(torch.tensor(2.0)) == 2.0
    scaler.step(opt)
    scaler.update()
    assert torch.equal(p.detach(), torch.full((3,), 0.5))
    assert scaler.state_dict() == {} and not scaler.is_enabled()
    # enabled, on CPU tensors, with a PyTorch optimizer: PyTorch's own path, skip included
    scaler = yt.GradScaler("cpu", init_scale=4.0, growth_interval=1)
    for grad, want in ((float("inf"), 0.5), (1.0, 0.0)):
        p.grad = torch.full((3,), grad) * scaler.scale(torch.ones(()))
        scaler.step(opt)
        scaler.update()
        assert torch.equal(p.detach(), torch.full((3,), want))
    assert scaler.get_scale() == 4.0                                   # halved by the skip, doubled by the applied step
    assert not getattr(yt.SGD, "_step_supports_amp_scaling", False)
