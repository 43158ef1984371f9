"""CPU-side checks of rectangular (H != W) support: program builder shapes, scaled anchors and the letterbox canvas query
(host entry points of the library only; no kernel runs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import net as onet
from tests import golden_inputs as gi


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def test_program_builder_rect_shapes(built):
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine
    m = yt.YOLOv3(num_classes=2)
    m.load_state_dict(onet.synth_state_dict(0, 3, 2))
    H, W = 352, 608
    p = engine.build_network_program(m, 2, H, W=W)
    assert p.input.H == H and p.input.W == W
    assert p.buf_numel[p.input.buf] == 2 * H * W * 4
    heads = sorted((op["pred"], op["Ho"], op["Wo"]) for op in p.ops if op["pred"] is not None)
    assert heads == [(0, 11, 19), (1, 22, 38), (2, 44, 76)]
    for op in p.ops:                                   # every map keeps the aspect ratio of the input
        assert op["x"].H * W == op["x"].W * H
    sq = engine.build_network_program(m, 2, 416)
    sq2 = engine.build_network_program(m, 2, 416, W=416)
    assert sq.buf_numel == sq2.buf_numel and [(o["Ho"], o["Wo"]) for o in sq.ops] == [(o["Ho"], o["Wo"]) for o in sq2.ops]
    t = engine.build_network_program(m, 1, W, W=H)     # transposed input: transposed maps
    assert [(o["Ho"], o["Wo"]) for o in t.ops] == [(o["Wo"], o["Ho"]) for o in p.ops]


def test_scaled_anchors():
    import yolo_for_turbines_amd as yt
    A = gi.COCO_ANCHORS
    for S in (320, 416, 608):
        ref = torch.tensor(A) * torch.tensor([S // 32, S // 16, S // 8]).unsqueeze(1).unsqueeze(1).repeat(1, 3, 2)   # train.py:195-197
        assert torch.equal(yt.scaled_anchors(A, S, S), ref)
        assert torch.equal(yt.scaled_anchors(A, S), ref)
    assert torch.equal(yt.scaled_anchors(A, 352, 608), yt.scaled_anchors(A, 608, 608))
    assert torch.equal(yt.scaled_anchors(A, 608, 224), yt.scaled_anchors(A, 608))
    with pytest.raises(ValueError):
        yt.scaled_anchors(A, 100, 96)


def _canvas(lib, sizes, size, rect):
    hw = (C.c_int32 * (2 * len(sizes)))(*[v for s in sizes for v in s])
    out = (C.c_int32 * 2)()
    assert lib.yolo_letterbox_canvas(hw, len(sizes), size, rect, out) == 0
    return int(out[0]), int(out[1])


def test_letterbox_canvas_sizes(built):
    lib = built.lib()
    assert _canvas(lib, [(1080, 1920)], 608, 0) == (608, 608)
    assert _canvas(lib, [(1080, 1920)], 608, 1) == (352, 608)        # 342 rows -> 352
    assert _canvas(lib, [(1920, 1080)], 608, 1) == (608, 352)
    assert _canvas(lib, [(720, 1280)], 416, 1) == (256, 416)         # 234 rows -> 256
    assert _canvas(lib, [(1080, 1920), (1000, 1000)], 608, 1) == (608, 608)
    assert _canvas(lib, [(300, 700), (1080, 1920)], 608, 1) == (352, 608)
    assert _canvas(lib, [(480, 640)], 416, 1) == (320, 416)          # 312 -> 320
    assert _canvas(lib, [(352, 608)], 608, 1) == (352, 608)          # resized side already a multiple of 32
    # against the rule restated: banker's rounding of dim * scale, then the smallest multiple of 32
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(200):
        n = int(rng.integers(1, 4))
        sizes = [(int(rng.integers(20, 3000)), int(rng.integers(20, 3000))) for _ in range(n)]
        size = int(rng.choice([320, 416, 608]))
        hh, ww = 0, 0
        for h, w in sizes:
            sc = size / max(h, w)
            nh, nw = (h, w) if sc == 1.0 else (max(1, round(h * sc)), max(1, round(w * sc)))
            hh, ww = max(hh, nh), max(ww, nw)
        assert _canvas(lib, sizes, size, 1) == (-(-hh // 32) * 32, -(-ww // 32) * 32)
    out = (C.c_int32 * 2)()
    assert lib.yolo_letterbox_canvas(None, 0, 416, 1, out) != 0      # a batch needs images


def test_forward_rejects_non_multiple_of_32_before_touching_the_gpu():
    import yolo_for_turbines_amd as yt
    m = yt.YOLOv3(num_classes=2)
    with pytest.raises((ValueError, RuntimeError)):
        m(torch.zeros(1, 3, 96, 160))                  # CPU tensor: no CPU fallback
