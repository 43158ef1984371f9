"""Training on tiles without a GPU: the draws of crop_params, the header's YOLO_CROP_* defines against the Python constants, the
exported names, the properties of the window rule on the numpy restatement (tests/crops_ref.py) alone, and the argument errors that
are raised before anything touches the device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import crops_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_crop_boxes", "yolo_crop_images")
NEW_NAMES = ("crop_params", "CropPool", "crop_batch", "train_crops")
TOP = 1.0 - 2.0 ** -53                                     # the largest double below 1: the top of a [0, 1) draw


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def test_crop_params_shape_determinism_ranges():
    import yolo_for_turbines_amd as yt
    p = yt.crop_params(1000, torch.Generator().manual_seed(3), scale=(0.5, 2.0), background=0.25)
    q = yt.crop_params(1000, torch.Generator().manual_seed(3), scale=(0.5, 2.0), background=0.25)
    r = yt.crop_params(1000, torch.Generator().manual_seed(4), scale=(0.5, 2.0), background=0.25)
    assert p.shape == (1000, 5) and p.dtype == torch.float64
    assert torch.equal(p, q) and not torch.equal(p, r)
    for col in (cr.U_PICK, cr.JX, cr.JY):
        assert float(p[:, col].min()) >= 0.0 and float(p[:, col].max()) < 1.0
    assert set(p[:, cr.BACKGROUND].tolist()) == {0.0, 1.0} and 150 < int(p[:, cr.BACKGROUND].sum()) < 350
    assert float(p[:, cr.SCALE].min()) >= 0.5 and float(p[:, cr.SCALE].max()) <= 2.0
    # one torch.rand call: the table is a function of the raw draws of the same generator state
    u = torch.rand((1000, 5), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    assert torch.equal(p[:, [cr.U_PICK, cr.JX, cr.JY]], u[:, [cr.U_PICK, cr.JX, cr.JY]])
    assert torch.equal(p[:, cr.BACKGROUND], (u[:, cr.BACKGROUND] < 0.25).double())
    assert torch.equal(p[:, cr.SCALE], 0.5 + (2.0 - 0.5) * u[:, cr.SCALE])
    fixed = yt.crop_params(64, torch.Generator().manual_seed(1), scale=(0.37, 0.37), background=0.0)
    assert set(fixed[:, cr.SCALE].tolist()) == {0.37} and float(fixed[:, cr.BACKGROUND].sum()) == 0.0
    assert float(yt.crop_params(64, torch.Generator().manual_seed(1), background=1.0)[:, cr.BACKGROUND].sum()) == 64.0
    assert yt.crop_params(0).shape == (0, 5)


@pytest.mark.parametrize("kw", [dict(scale=(0.0, 1.0)), dict(scale=(2.0, 1.0)), dict(scale=(1.0, 8.5)), dict(scale=(float("nan"), 1.0)),
                                dict(scale=1.0), dict(scale=(1.0,)), dict(background=-0.1), dict(background=1.5),
                                dict(background=float("nan")), dict(background="x")])
def test_crop_params_validation(kw):
    import yolo_for_turbines_amd as yt
    with pytest.raises(ValueError):
        yt.crop_params(4, **kw)


def test_header_defines_equal_python_constants(built):
    from yolo_for_turbines_amd import crops
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    want = {"U_PICK": crops.CROP_U_PICK, "BACKGROUND": crops.CROP_BACKGROUND, "JX": crops.CROP_JX, "JY": crops.CROP_JY,
            "SCALE": crops.CROP_SCALE, "NPARAM": crops.CROP_NPARAM}
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define YOLO_CROP_([A-Z_]+) (\d+)", hdr)}
    assert got == want
    assert (cr.U_PICK, cr.BACKGROUND, cr.JX, cr.JY, cr.SCALE, cr.NPARAM) == tuple(want.values())


def test_new_symbols_and_names_are_exported(built):
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import crops, utils
    lib = built.lib()
    for sym in NEW_SYMBOLS:
        assert sym in built.EXPORTS and hasattr(lib, sym)
    for name in NEW_NAMES:
        assert getattr(yt, name) is getattr(crops, name) and name in crops.__all__
        assert name not in yt.__all__ and not hasattr(utils, name)


def test_c_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    ok = dict(boxes=8, nbox=8, max_in=1, hw=8, n_pool=1, src=8, cp=8, org=None, ap=None, b=1, th=32, tw=32, vis=0.4, out=8, counts=8,
              max_out=1, win=8)

    def boxes(**kw):
        a = {**ok, **kw}
        return lib.yolo_crop_boxes(a["boxes"], a["nbox"], a["max_in"], a["hw"], a["n_pool"], a["src"], a["cp"], a["org"], a["ap"], a["b"],
                                   a["th"], a["tw"], a["vis"], a["out"], a["counts"], a["max_out"], a["win"], None)
    for bad in (dict(boxes=None), dict(nbox=None), dict(hw=None), dict(src=None), dict(cp=None), dict(out=None), dict(counts=None),
                dict(win=None), dict(max_in=0), dict(max_out=0), dict(n_pool=0), dict(b=0), dict(b=65536), dict(th=0), dict(th=48),
                dict(tw=33), dict(vis=float("nan")), dict(vis=-0.01), dict(vis=1.01)):
        assert boxes(**bad) == -1, bad                         # YOLO_ERR_ARG
        assert lib.yolo_last_error()
    oki = dict(pool=8, off=8, hw=8, n_pool=1, win=8, ap=None, b=1, th=32, tw=32, st=None, out=16)

    def images(**kw):
        a = {**oki, **kw}
        return lib.yolo_crop_images(a["pool"], a["off"], a["hw"], a["n_pool"], a["win"], a["ap"], a["b"], a["th"], a["tw"], a["st"], a["out"],
                                    None)
    for bad in (dict(pool=None), dict(off=None), dict(hw=None), dict(win=None), dict(out=None), dict(ap=8), dict(n_pool=0), dict(b=0),
                dict(b=65536), dict(th=16), dict(tw=100)):
        assert images(**bad) == -1, bad
        assert lib.yolo_last_error()


def test_level_sizes_round_half_to_even():
    assert cr.level_hw(37, 53, 0.5) == (18, 26)            # 18.5 -> 18, 26.5 -> 26
    assert cr.level_hw(37, 53, 1.0) == (37, 53)
    assert cr.level_hw(35, 55, 0.5) == (18, 28)            # 17.5 -> 18, 27.5 -> 28
    assert cr.level_hw(1, 1, 0.1) == (1, 1)
    assert cr.level_hw(20, 45, 2.0) == (40, 90)


def _window_properties(hw, boxes, cp, th, tw):
    y0, x0, LH, LW, picked = cr.window(hw, boxes, cp, th, tw)
    assert (LH, LW) == cr.level_hw(hw[0], hw[1], float(cp[cr.SCALE]))
    for o, L, t in ((y0, LH, th), (x0, LW, tw)):
        if L >= t:
            assert 0 <= o <= L - t                             # the window lies inside the level
        else:
            assert o == 0                                      # one tile at 0, zero-padded
    if cp[cr.BACKGROUND] != 0.0 or not boxes:
        assert picked == -1
        return
    assert 0 <= picked < len(boxes)
    cx, cy = boxes[picked][0], boxes[picked][1]
    for c, o, L, t in ((cy, y0, LH, th), (cx, x0, LW, tw)):
        if L > t and 0.0 <= c <= 1.0:
            assert 0.0 <= (c * L - o) / t <= 1.0               # the picked centre is in the closed unit tile


def test_window_rule_properties_random_draws():
    rng = np.random.default_rng(0)
    sizes = [(37, 53), (101, 67), (33, 200), (20, 45), (64, 96), (3000, 4000), (417, 416)]
    tiles = [(32, 32), (64, 32), (32, 96), (416, 416)]
    for _ in range(10000):
        hw = sizes[rng.integers(len(sizes))]
        th, tw = tiles[rng.integers(len(tiles))]
        nb = int(rng.integers(0, 5))
        boxes = [[float(rng.random()), float(rng.random()), float(rng.uniform(0.01, 0.5)), float(rng.uniform(0.01, 0.5)), 0.0]
                 for _ in range(nb)]
        cp = [float(rng.random()), float(rng.random() < 0.2), float(rng.random()), float(rng.random()),
              float(rng.choice([1.0, 0.5, 0.37, 2.0, rng.uniform(0.1, 3.0)]))]
        _window_properties(hw, boxes, cp, th, tw)


def test_window_rule_properties_extremes():
    for hw in ((37, 53), (101, 67), (33, 200), (20, 45), (64, 96), (3000, 4000)):
        for th, tw in ((32, 32), (64, 32), (32, 96)):
            for scale in (1.0, 0.5, 0.37, 2.0):
                for j in (0.0, TOP):
                    for u in (0.0, TOP):
                        for c in (0.0, 1.0):
                            boxes = [[c, c, 0.1, 0.1, 0.0], [1.0 - c, c, 0.2, 0.2, 1.0], [0.5, 0.5, 0.1, 0.1, 0.0]]
                            for bg in (0.0, 1.0):
                                _window_properties(hw, boxes, [u, bg, j, j, scale], th, tw)
    # U_PICK just below 1 picks the last row, 0 the first; a background window at the top jitter is flush with the far edge
    assert cr.window((100, 100), [[0.5, 0.5, 0.1, 0.1, 0]] * 3, [TOP, 0.0, 0.5, 0.5, 1.0], 32, 32)[4] == 2
    assert cr.window((100, 100), [[0.5, 0.5, 0.1, 0.1, 0]] * 3, [0.0, 0.0, 0.5, 0.5, 1.0], 32, 32)[4] == 0
    assert cr.window((100, 100), [], [0.0, 0.0, TOP, 0.0, 1.0], 32, 32)[:2] == (0, 68)
    assert cr.window((100, 100), None, [0.0, 0.0, 0.0, TOP, 1.0], 32, 32)[:2] == (68, 0)


def test_visibility_rule_on_powers_of_two():
    """Level 128 wide, tile 32, x0 = 64: 4 of 10 pixels visible is exactly 0.4 and kept, 6 of 16 (0.375) is dropped."""
    win = (0, 64, 32, 128, -1)
    def box(a, b):
        return [(a + b) / 256.0, 0.5, (b - a) / 128.0, 0.5, 1.0]
    assert len(cr.crop_boxes((32, 128), [box(58, 68)], win, 32, 32)) == 1
    assert len(cr.crop_boxes((32, 128), [box(54, 70)], win, 32, 32)) == 0
    assert len(cr.crop_boxes((32, 128), [box(10, 40)], win, 32, 32)) == 0
    assert len(cr.crop_boxes((32, 128), [[0.6, 0.5, 0.0, 0.5, 0.0]], win, 32, 32)) == 0
    assert len(cr.crop_boxes((32, 128), [box(54, 70)], win, 32, 32, min_visibility=0.0)) == 1
    assert len(cr.crop_boxes((32, 128), [box(58, 68), box(66, 90)], win, 32, 32, min_visibility=1.0)) == 1


def test_value_errors_need_no_gpu():
    import yolo_for_turbines_amd as yt
    u8 = lambda *s: np.zeros(s, np.uint8)
    for images, boxes, pattern in (([], [], "empty"), ([u8(4, 4)], [[]], "image 0.*\\(H, W, 3\\)"),
                                   ([u8(4, 4, 3), np.zeros((4, 4, 3), np.float32)], [[], []], "image 1.*uint8"),
                                   ([u8(0, 4, 3)], [[]], "image 0.*no pixels"), ([u8(4, 4, 3)], [[], []], "one entry"),
                                   ([u8(4, 4, 3)], [[[0.5, 0.5, 0.1, 0.1]]], "image 0.*box rows")):
        with pytest.raises(ValueError, match=pattern):
            yt.CropPool(images, boxes)
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.CropPool([u8(4, 4, 3)], [[]], device="cpu")
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.crop_batch([u8(4, 4, 3)], [[]], tile=32, device="cpu")
