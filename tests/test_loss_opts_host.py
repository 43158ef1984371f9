"""CPU checks of the loss options: the yardstick `tests/loss_ref.py` against the oracle at its defaults, the constructor of
``FusedYOLOLoss`` (no device needed), and the boundary (header, exports, struct layout)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import loss as oloss
from tests import golden_inputs as gi
from tests import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nc,S,B", [(2, 96, 4), (80, 64, 2)])
def test_reference_at_its_defaults_is_the_oracle(nc, S, B):
    anchors = gi.TRAIN_CASE["anchors"]
    tg = [torch.from_numpy(t) for t in gi.synth_targets(B, S, nc, anchors, 77)]
    grids = [S // 32, S // 16, S // 8]
    sa = torch.tensor(anchors) * torch.tensor(grids).view(3, 1, 1)
    rng = np.random.Generator(np.random.PCG64(5))
    w = torch.tensor([1.0, 0.7, 1.3, 0.9], dtype=torch.float64)
    for i, g in enumerate(grids):
        p = torch.from_numpy(rng.standard_normal((B, 3, g, g, 5 + nc), dtype=np.float32)).double()
        pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
        t, t_before = tg[i].clone(), tg[i].clone()
        want = torch.stack(oloss.yolo_loss(pa * 1.0, tg[i].double(), sa[i].double()))
        got = torch.stack(loss_ref.yolo_loss_opts(pb, t, sa[i]))
        (want * w).sum().backward()
        (got * w).sum().backward()
        assert got.dtype == torch.float64 and torch.equal(t, t_before) and torch.equal(pb.detach(), p)
        np.testing.assert_allclose(got.detach().numpy(), want.detach().numpy(), rtol=1e-12, atol=1e-14)
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-12 * float(pa.grad.abs().max())


def test_reference_empty_sets():
    p = torch.zeros(1, 3, 2, 2, 7, dtype=torch.float64)
    t = torch.zeros(1, 3, 2, 2, 6)
    anc = torch.tensor([[1.0, 2.0], [2.5, 1.5], [4.0, 3.0]])
    parts = loss_ref.yolo_loss_opts(p, t, anc, "ciou", "bce", 1.5, 0.1)
    assert [float(v) for v in parts[:2]] == [0.0, 0.0] and float(parts[3]) == 0.0
    assert float(parts[2]) == pytest.approx(0.5 * 0.5 ** 1.5 * np.log(2.0), rel=1e-12)
    t[..., 4] = -1.0
    assert torch.isnan(loss_ref.yolo_loss_opts(p, t, anc)[2])               # an empty mean, like torch


def test_constructor_needs_no_device_and_keeps_its_arguments():
    import yolo_for_turbines_amd as yt
    lf = yt.FusedYOLOLoss(box_loss="ciou", obj_loss="bce", focal_gamma=1.5, label_smoothing=0.1)
    assert (lf.box_loss, lf.obj_loss, lf.focal_gamma, lf.label_smoothing, lf.lambdas) == ("ciou", "bce", 1.5, 0.1, (5.0, 1.0, 0.5, 1.0))
    assert not lf._default and yt.FusedYOLOLoss()._default and yt.FusedYOLOLoss("mse", "mse", 0.0, 0.0, (5, 1, 0.5, 1))._default
    assert not yt.FusedYOLOLoss(lambdas=(5, 1, 1, 1))._default and not yt.FusedYOLOLoss(label_smoothing=0.05)._default
    with pytest.raises(RuntimeError, match="MI355X only"):
        lf(torch.zeros(1, 3, 2, 2, 7), torch.zeros(1, 3, 2, 2, 6), torch.ones(3, 2))


@pytest.mark.parametrize("kw", [dict(box_loss="iou"), dict(box_loss=None), dict(obj_loss="focal"), dict(focal_gamma=-0.5),
                                dict(focal_gamma=float("nan")), dict(focal_gamma=float("inf")), dict(label_smoothing=1.0),
                                dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")), dict(lambdas=(5, 1, 0.5)),
                                dict(lambdas=(5, 1, 0.5, float("inf"))), dict(lambdas=(5, 1, float("nan"), 1)), dict(lambdas=5)])
def test_bad_values_raise_value_error(kw):
    import yolo_for_turbines_amd as yt
    with pytest.raises(ValueError):
        yt.FusedYOLOLoss(**kw)


def test_header_declares_and_the_binding_exports_the_entry_points():
    from yolo_for_turbines_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    for name in ("yolo_loss_fwd_opts", "yolo_loss_bwd_opts"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in L.EXPORTS
        assert L._SIGS[name][1].count(C.POINTER(L.LossOpts)) == 1
    assert re.search(r"typedef struct yolo_loss_opts \{[^}]*\} yolo_loss_opts;", hdr)
    kinds = dict(re.findall(r"YOLO_LOSS_(?:BOX|OBJ)_([A-Z]+) = (\d)", hdr))
    assert {k: int(kinds[k.upper()]) for k in L.LOSS_BOX_KINDS} == L.LOSS_BOX_KINDS
    assert L.LOSS_OBJ_KINDS == {"mse": 0, "bce": 1} and kinds["BCE"] == "1"


@pytest.mark.parametrize("field,value,word", [("box_kind", 4, "box_kind"), ("box_kind", -1, "box_kind"), ("obj_kind", 2, "obj_kind"),
                                              ("focal_gamma", -1.0, "focal_gamma"), ("focal_gamma", float("nan"), "focal_gamma"),
                                              ("label_smoothing", 1.0, "label_smoothing"), ("label_smoothing", -0.25, "label_smoothing"),
                                              ("lambda_noobj", float("inf"), "lambda"), ("lambda_class", float("nan"), "lambda")])
def test_library_refuses_bad_options_before_any_launch(field, value, word):
    """The options are checked on the host before a launch: host memory stands in for every device pointer, no GPU is touched."""
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    strides = (C.c_int64 * 5)(84, 28, 14, 7, 1)
    opts = L.LossOpts(3, 1, 1.5, 0.1, 5, 1, 0.5, 1)
    setattr(opts, field, value)
    rc = lib.yolo_loss_fwd_opts(ptr, strides, ptr, ptr, 1, 2, 2, 2, ptr, ptr, ptr, 4096, C.byref(opts), None)
    assert rc < 0 and word.encode() in lib.yolo_last_error()
    rc = lib.yolo_loss_bwd_opts(ptr, strides, ptr, ptr, 1, 2, 2, 2, ptr, ptr, ptr, C.byref(opts), None)
    assert rc < 0 and word.encode() in lib.yolo_last_error()
    assert lib.yolo_loss_fwd_opts(ptr, strides, ptr, ptr, 1, 2, 2, 2, ptr, ptr, ptr, 4096, None, None) < 0


def test_options_struct_layout():
    from yolo_for_turbines_amd import _lib as L
    assert C.sizeof(L.LossOpts) == 32
    assert [n for n, _ in L.LossOpts._fields_] == ["box_kind", "obj_kind", "focal_gamma", "label_smoothing", "lambda_box", "lambda_obj",
                                                   "lambda_noobj", "lambda_class"]
    assert L.LossOpts.lambda_box.offset == 16 and L.LossOpts.focal_gamma.offset == 8
