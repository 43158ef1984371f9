"""The augmentation extras without a device: the draws and the validation of yolo_for_turbines_amd/extras.py, properties of the
numpy restatement tests/augx_ref.py, and the condition that keeps the GPU comparison (tests/test_gpu_augx.py) from passing on empty
box tables: every shared case of tests/augx_cases.py keeps and drops boxes where it should."""
import math

import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests import augx_cases as xc
from tests import augx_ref as xr
from tests import crops_ref as cr
from yolo_for_turbines_amd import extras as ex


def test_header_columns_match():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yolo_mi355x.h")).read()
    cols = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define YOLO_AUGX_(\w+) (\d+)", text)}
    assert cols == dict(ROT_COS=0, ROT_SIN=1, DO_VFLIP=2, MIX_PARTNER=3, MIX_LAMBDA=4, CUT_N=5, CUT_COVER=6, CUT_FILL=7, CUT_RECT=8,
                        NPARAM=24)
    for name, v in cols.items():
        assert getattr(ex, "EXTRA_NPARAM" if name == "NPARAM" else name) == v
        assert getattr(xr, name) == v
    import yolo_for_turbines_amd as yt
    assert yt.extra_params is ex.extra_params and "extra_params" not in yt.__all__


def test_extra_params_one_state_one_table():
    kw = dict(degrees=30.0, flipud=0.5, mixup=0.5, cutout=0.7, cut_max=3, cut_fill=0.5)
    a = ex.extra_params(64, torch.Generator().manual_seed(5), **kw)
    b = ex.extra_params(64, torch.Generator().manual_seed(5), **kw)
    c = ex.extra_params(64, torch.Generator().manual_seed(6), **kw)
    assert a.shape == (64, 24) and a.dtype == torch.float64 and torch.equal(a, b) and not torch.equal(a, c)
    # one torch.rand call: the generator is left where one (n, 23) draw leaves it
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    ex.extra_params(64, g, **kw)
    torch.rand((64, 23), generator=h, dtype=torch.float64)
    assert torch.equal(g.get_state(), h.get_state())
    # the draws are what the docstring says
    assert bool(((a[:, 0] ** 2 + a[:, 1] ** 2 - 1).abs() < 1e-12).all()) and bool((a[:, 0] >= math.cos(math.radians(30)) - 1e-12).all())
    assert set(a[:, ex.DO_VFLIP].tolist()) == {0.0, 1.0}
    pt = a[:, ex.MIX_PARTNER]
    rows = torch.arange(64, dtype=torch.float64)
    assert bool(((pt == -1) | ((pt >= 0) & (pt < 64) & (pt != rows) & (pt == pt.floor()))).all()) and bool((pt >= 0).any())
    assert bool(((a[:, ex.MIX_LAMBDA] >= 0.4) & (a[:, ex.MIX_LAMBDA] <= 0.6)).all())
    cn = a[:, ex.CUT_N]
    assert set(cn.tolist()) <= {0.0, 1.0, 2.0, 3.0} and bool((cn > 0).any()) and bool((cn == 0).any())
    r = a[:, ex.CUT_RECT:].view(64, 4, 4)
    live = torch.arange(4)[None, :] < cn[:, None]
    w, h = (r[..., 2] - r[..., 0])[live], (r[..., 3] - r[..., 1])[live]
    assert bool(((w >= 0.05 - 1e-12) & (w <= 0.25 + 1e-12) & (h >= 0.05 - 1e-12) & (h <= 0.25 + 1e-12)).all())
    assert not r[~live].any()
    ex._extra_table(a, 64)                                   # what it draws passes its own validation
    assert ex.extra_params(1, mixup=1.0)[0, ex.MIX_PARTNER] == -1     # nobody to mix with


def test_defaults_are_neutral():
    t = ex.extra_params(5, torch.Generator().manual_seed(1))
    want = torch.zeros(5, 24, dtype=torch.float64)
    want[:, ex.ROT_COS], want[:, ex.MIX_PARTNER], want[:, ex.CUT_COVER] = 1.0, -1.0, 0.6
    lam = t[:, ex.MIX_LAMBDA].clone()
    t[:, ex.MIX_LAMBDA] = 0.0
    assert torch.equal(t, want) and bool(((lam >= 0.4) & (lam <= 0.6)).all())
    assert ex.extra_params(0).shape == (0, 24)


@pytest.mark.parametrize("kw, msg", [
    (dict(n=-1), "n must be >= 0"), (dict(degrees=-1.0), "degrees must be in"), (dict(degrees=float("nan")), "degrees must be in"),
    (dict(flipud=1.5), "flipud must be a probability"), (dict(mixup="x"), "mixup must be a probability"),
    (dict(cutout=-0.1), "cutout must be a probability"), (dict(mix_lambda=(0.6, 0.4)), "mix_lambda must satisfy"),
    (dict(mix_lambda=0.5), "mix_lambda must be a"), (dict(cut_size=(0.1, 1.5)), "cut_size must satisfy"),
    (dict(cut_cover=2.0), "cut_cover must be a probability"), (dict(cut_max=5), "cut_max must be an integer"),
    (dict(cut_max=2.0), "cut_max must be an integer"), (dict(cut_fill=float("inf")), "cut_fill must be finite")])
def test_extra_params_messages(kw, msg):
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        ex.extra_params(kw.pop("n", 4), **kw)


@pytest.mark.parametrize("col, value, msg", [
    (ex.ROT_COS, 0.9, "cos and sin of one angle"), (ex.ROT_SIN, float("nan"), "cos and sin of one angle"),
    (ex.MIX_PARTNER, float("inf"), "must be finite"), (ex.CUT_FILL, float("nan"), "must be finite"),
    (ex.MIX_LAMBDA, 1.5, "MIX_LAMBDA must lie in"), (ex.MIX_LAMBDA, float("nan"), "MIX_LAMBDA must lie in"),
    (ex.CUT_COVER, -0.1, "CUT_COVER must lie in"), (ex.CUT_N, 5.0, "CUT_N must be an integer"), (ex.CUT_N, 1.5, "CUT_N must be an integer"),
    (ex.CUT_N, -1.0, "CUT_N must be an integer"), (ex.CUT_RECT + 7, float("inf"), "CUT_RECT columns must be finite")])
def test_extra_table_messages(col, value, msg):
    t = xr.neutral(3)
    ex._extra_table(t, 3)
    t[1, col] = value
    with pytest.raises(ValueError, match=msg):
        ex._extra_table(t, 3)


def test_extra_table_shape_and_partners():
    with pytest.raises(ValueError, match=r"extra must have shape \(3, 24\)"):
        ex._extra_table(xr.neutral(4), 3)
    with pytest.raises(ValueError, match="extra must be an array or tensor"):
        ex._extra_table(object(), 3)
    t = xr.neutral(4)
    t[:, ex.MIX_PARTNER] = [1.0, 1.0, 4.0, 1.5]
    assert ex._host_partners(ex._extra_table(t, 4), 4) == [1, -1, -1, -1] == [xr.partner(t[b], b, 4) for b in range(4)]


# ------------------------------------------------------------------------------------------------- the restatement
def test_neutral_rows_give_augment_ref_bits():
    for case in (c for c in xc.CASES if c["kind"] == "neutral"):
        H, W = case["canvas"]
        images, boxes = xc.POOLS[case["canvas"]]
        x, bs = xc.reference(case, "augment")
        rx, rb, _ = ar.augment(images, boxes, case["params"], H, W, case["mosaic"])
        assert np.array_equal(x, rx) and bs == rb and any(bs)
        x, bs = xc.reference(case, "crop")
        rx, rb, _ = cr.crop(images, boxes, case["index"], case["cp"], H, W, params=case["params"])
        assert np.array_equal(x, rx) and bs == rb and any(bs)


def test_quarter_turn_swaps_the_sides():
    p, e = [0.0] * 29, xr.neutral(1)[0]
    p[ar.DO_SSR], p[ar.SCALE] = 1.0, 1.0
    e[xr.ROT_COS], e[xr.ROT_SIN] = 0.0, 1.0
    b = [0.3, 0.4, 0.6, 0.5]                                  # w 0.3, h 0.1
    r = xr.chain_box(b, p, e, 64, 64)
    assert abs((r[2] - r[0]) - 0.1) <= 1e-12 and abs((r[3] - r[1]) - 0.3) <= 1e-12
    assert abs((r[0] + r[2]) / 2 - 0.45) <= 1e-12 and abs((r[1] + r[3]) / 2 - 0.55) <= 1e-12     # (x, y) -> (y, 1 - x)


def test_lambda_ends_return_one_image():
    rng = np.random.default_rng(3)
    chains = [(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8), [([0.1, 0.1, 0.5, 0.5], 1.0)]) for _ in range(2)]
    e = xr.neutral(2)
    e[0, xr.MIX_PARTNER], e[0, xr.MIX_LAMBDA] = 1.0, 1.0
    e[1, xr.MIX_PARTNER], e[1, xr.MIX_LAMBDA] = 0.0, 0.0
    x, bs = xr.mix_cut(chains, e)
    own = ar.to_float_chw(chains[0][0])
    assert np.array_equal(x[0], own) and np.array_equal(x[1], own)
    assert len(bs[0]) == 2 and len(bs[1]) == 2                # the boxes of both rows whatever lambda is


def test_full_rectangle_leaves_fill_and_half_cover_survives():
    u8 = np.full((32, 32, 3), 200, np.uint8)
    box = ([0.25, 0.25, 0.75, 0.75], 1.0)
    e = xr.neutral(3)
    e[0, xr.CUT_N], e[0, xr.CUT_COVER], e[0, xr.CUT_FILL] = 1.0, 0.6, 0.5
    e[0, xr.CUT_RECT:xr.CUT_RECT + 4] = [0.0, 0.0, 1.0, 1.0]
    e[1, xr.CUT_N], e[1, xr.CUT_COVER] = 1.0, 0.5
    e[1, xr.CUT_RECT:xr.CUT_RECT + 4] = [0.5, 0.0, 1.0, 1.0]  # exactly half of the box
    e[2] = e[1]
    e[2, xr.CUT_COVER] = 0.5 - 2.0 ** -40
    x, bs = xr.mix_cut([(u8, [box])] * 3, e)
    assert np.all(x[0] == np.float32(0.5)) and bs[0] == []
    assert len(bs[1]) == 1 and bs[2] == [] and np.all(x[1][:, :, 16:] == 0) and np.all(x[1][:, :, :16] == np.float32(200) * np.float32(1 / 255))
    e[1, xr.CUT_RECT:xr.CUT_RECT + 4] = [0.6, 0.0, 0.4, 1.0]  # empty: erases nothing, drops nothing
    x, bs = xr.mix_cut([(u8, [box])] * 3, e)
    assert np.all(x[1] == x[1][0, 0, 0]) and len(bs[1]) == 1


# ------------------------------------------------------------------------------------------------- the shared cases
def _neutral_counts(case, user, ssr=True):
    """The box counts of a case with the neutral extras; ssr=False: also without ShiftScaleRotate, the boxes that reach that step."""
    H, W = case["canvas"]
    images, boxes = xc.POOLS[case["canvas"]]
    n, params = xr.neutral(xc.B), case["params"].copy()
    if not ssr:
        params[:, ar.DO_SSR] = 0.0
    if user == "augment":
        return [len(r) for r in xr.augment(images, boxes, params, n, H, W, case["mosaic"])[1]]
    return [len(r) for r in xr.crop(images, boxes, case["index"], case["cp"], params, n, H, W)[1]]


@pytest.mark.parametrize("user", ["augment", "crop"])
@pytest.mark.parametrize("case", xc.CASES, ids=[c["name"] for c in xc.CASES])
def test_cases_keep_and_drop_boxes(case, user):
    _, boxes = xc.POOLS[case["canvas"]]
    x, bs = xc.reference(case, user)
    assert x.shape == (xc.B, 3, *case["canvas"]) and x.dtype == np.float32
    src = [int(r[0]) for r in case["mosaic"]] if user == "augment" else case["index"]
    have = [b for b in range(xc.B) if boxes[src[b]]]
    kept = [b for b in have if bs[b]]
    assert have and 2 * len(kept) >= len(have), f"{case['name']} / {user}: boxes kept in rows {kept} of {have}"
    if case["kind"] in ("rotation", "cutout"):
        plain = _neutral_counts(case, user, ssr=case["kind"] != "rotation")    # the rotated box's visibility rule / the erase rule drops
        assert any(len(r) < n for r, n in zip(bs, plain)), f"{case['name']} / {user}: no box is dropped ({plain})"
    if case["kind"] == "mixup" and case["name"] != "mix_none":
        plain = _neutral_counts(case, user)
        assert any(len(r) > n for r, n in zip(bs, plain)), f"{case['name']} / {user}: no partner box is appended ({plain})"
