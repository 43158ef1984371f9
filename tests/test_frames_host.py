"""The frame front end without a GPU: the numpy restatement (tests/frames_ref.py) against the oracle's letterbox and against the
definition of the colour conversion, the library's constants against the ones derived from Kr and Kb, the frame row's layout, the
exported names, and every ValueError that preprocess_frames raises before it touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import preprocess as opre
from tests import frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yolo_frames_tile", "yolo_frames_csc_constants", "yolo_frames_letterbox", "yolo_frames_to_rgb", "yolo_boxes_to_frames")
NEW_NAMES = ("preprocess_frames", "FrameStager", "frames_to_rgb", "boxes_to_frames", "detect_frames")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


@pytest.mark.parametrize("h,w", [(20, 48), (48, 20), (32, 17), (10, 12), (1, 1), (1, 7), (97, 131)])
def test_reference_rgb_path_is_the_oracles_letterbox(h, w):
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want, want_meta = opre.letterbox(img, 32)
    got, meta = R.preprocess([img], 32, "rgb")
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32)) and tuple(meta[0]) == want_meta
    flipped, _ = R.preprocess([img[:, :, ::-1]], 32, "bgr")
    assert np.array_equal(flipped.view(np.uint32), got.view(np.uint32))


def grey_nv12(levels, u=128, v=128):
    """A 2 x 2n frame whose column pair i has luma levels[i]."""
    y = np.repeat(np.asarray(levels, np.uint8), 2)[None].repeat(2, 0)
    uv = np.tile(np.array([u, v], np.uint8), len(levels))[None]
    return np.concatenate([y, uv], 0)


def test_bt601_limited_white_and_black():
    rgb = R.nv12_to_rgb(grey_nv12([235, 16, 0, 255]), "bt601")
    assert rgb[0, 0].tolist() == [255, 255, 255] and rgb[0, 2].tolist() == [0, 0, 0]
    assert rgb[1, 4].tolist() == [0, 0, 0] and rgb[1, 6].tolist() == [255, 255, 255]          # below black and above white: clipped


@pytest.mark.parametrize("csc", [k for k in R.CSC_KINDS if k != "bt601"])
def test_derived_constants_reproduce_a_grey_ramp(csc):
    """U = V = 128: R = G = B = the luma scaled to full range, rounded half up in exact arithmetic (the fixed point is within 2^-13
    of the exact value, and no exact value lies that close to a half: it is a multiple of 1 / 219 and 2 (Y - 16) 255 = 219 (2 k + 1)
    has no solution). Full range is the identity. (OpenCV's BT.601 literals are rounded from three decimals and do not pass this.)"""
    levels = np.arange(256)
    rgb = R.nv12_to_rgb(grey_nv12(levels), csc)[0, ::2]
    if csc.endswith("-full"):
        want = levels
    else:
        want = np.array([min(255, max(0, (2 * (int(y) - 16) * 255 + 219) // (2 * 219))) for y in levels])
    for c in range(3):
        assert np.array_equal(rgb[:, c], want), (csc, c)


def test_library_constants_are_the_derived_ones(built):
    lib = built.lib()
    for csc in R.CSC_KINDS:
        out = (C.c_int32 * 6)()
        assert lib.yolo_frames_csc_constants(built.CSC_KINDS[csc], out) == 0
        want = R.OPENCV_BT601 if csc == "bt601" else R.derived_constants(csc)
        assert tuple(out) == want, csc
    assert lib.yolo_frames_csc_constants(4, (C.c_int32 * 6)()) < 0 and lib.yolo_frames_csc_constants(0, None) < 0
    d = R.derived_constants("bt601")                       # OpenCV's literals are close to, not equal to, the derived BT.601 set
    assert d != R.OPENCV_BT601 and all(abs(a - b) < 1024 for a, b in zip(d, R.OPENCV_BT601))


def test_frame_row_layout_matches_header(built):
    row = built.FrameRow
    assert C.sizeof(row) == 24
    assert [(n, getattr(row, n).offset, getattr(row, n).size) for n, _ in row._fields_] == \
        [("offset", 0, 8), ("h", 8, 4), ("w", 12, 4), ("pitch", 16, 4), ("reserved", 20, 4)]
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    body = re.search(r"typedef struct yolo_frame_row \{(.*?)\} yolo_frame_row;\s*/\* 24 bytes \*/", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [s.strip() for s in decl.split(";") if s.strip()] == ["int64_t offset", "int32_t h, w", "int32_t pitch", "int32_t reserved"]
    for name, val in (("YOLO_FRAMES_RGB24", "rgb"), ("YOLO_FRAMES_BGR24", "bgr"), ("YOLO_FRAMES_NV12", "nv12")):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == built.FRAME_FORMATS[val]
    for name, val in (("YOLO_CSC_BT601", "bt601"), ("YOLO_CSC_BT601_FULL", "bt601-full"), ("YOLO_CSC_BT709", "bt709"),
                      ("YOLO_CSC_BT709_FULL", "bt709-full")):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == built.CSC_KINDS[val]


def test_new_symbols_and_names_are_exported(built):
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import frames, utils
    lib = built.lib()
    for sym in NEW_SYMBOLS:
        assert sym in built.EXPORTS and hasattr(lib, sym)
    tw, th = C.c_int(), C.c_int()
    lib.yolo_frames_tile(C.byref(tw), C.byref(th))
    assert tw.value > 0 and th.value > 0 and tw.value % 4 == 0
    for name in NEW_NAMES:
        assert getattr(yt, name) is getattr(frames, name) and name in frames.__all__
        assert name not in yt.__all__ and not hasattr(utils, name)


def test_c_entry_points_refuse_bad_arguments_before_any_launch(built):
    lib = built.lib()
    ok = dict(pool=8, table=8, n=1, fmt=0, csc=0, size=32, ch=32, cw=32, out=16, meta=16)
    call = lambda **kw: (lambda a: lib.yolo_frames_letterbox(a["pool"], a["table"], a["n"], a["fmt"], a["csc"], a["size"], a["ch"], a["cw"], a["out"],
                                                             a["meta"], None))({**ok, **kw})
    for bad in (dict(pool=None), dict(table=None), dict(table=12), dict(n=0), dict(fmt=3), dict(fmt=-1), dict(csc=4), dict(size=0), dict(ch=0),
                dict(cw=-1), dict(out=None), dict(n=2 ** 31 - 1, ch=64, cw=128)):
        assert call(**bad) == -1, bad                      # YOLO_ERR_ARG
        assert lib.yolo_last_error()
    assert lib.yolo_frames_to_rgb(8, 8, 1, 3, 4, 2, 0, 8, None) == -1          # NV12 with an odd height
    assert lib.yolo_frames_to_rgb(8, 8, 1, 16385, 4, 0, 0, 8, None) == -1
    assert lib.yolo_boxes_to_frames(8, 0, 4, 8, 32, 32, 8, None) == -1
    assert lib.yolo_boxes_to_frames(None, 2, 0, 8, 32, 32, None, None) == 0     # no rows: nothing to launch


def test_value_errors_name_the_frame_and_need_no_gpu(built):
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import frames as F
    u8 = lambda *s: np.zeros(s, np.uint8)
    bad = [
        (dict(frames=[u8(4, 4, 3), np.zeros((4, 4, 3), np.float32)]), "frame 1.*uint8"),
        (dict(frames=[u8(4, 4)]), "frame 0.*\\(H, W, 3\\)"),
        (dict(frames=[u8(4, 4, 4)]), "frame 0.*\\(H, W, 3\\)"),
        (dict(frames=[u8(6, 4), u8(6, 4, 3)], format="nv12"), "frame 1.*NV12"),
        (dict(frames=[u8(4, 4, 3)], format="yuv"), "format"),
        (dict(frames=[u8(6, 4)], format="nv12", csc="bt2020"), "csc"),
        (dict(frames=[u8(6, 4), (u8(64), 3, 4, 4)], format="nv12"), "frame 1.*even"),
        (dict(frames=[u8(6, 4), u8(8, 4)], format="nv12"), "frame 1.*H \\* 3 / 2"),
        (dict(frames=[u8(6, 3)], format="nv12"), "frame 0.*even"),
        (dict(frames=[(u8(64), 4, 4, 11)]), "frame 0.*pitch 11"),
        (dict(frames=[u8(4, 4, 3), (u8(64), 4, 4, 3)], format="nv12"), "frame 0"),
        (dict(frames=[(u8(64), 6, 4, 3)], format="nv12"), "frame 0.*pitch 3"),
        (dict(frames=[(u8(40), 4, 4, 12)]), "frame 0.*40 bytes"),
        (dict(frames=[(u8(64), 4, 4)]), "frame 0.*pitch"),
        (dict(frames=[]), "empty"),
        (dict(frames=[u8(0, 4, 3)]), "frame 0.*no pixels"),
        (dict(frames=[u8(4, 4, 3)], image_size=0), "image_size"),
        (dict(frames=[u8(4, 4, 3)], image_size=32, out=torch.zeros(1, 3, 32, 32)), "out"),             # on the host
        (dict(frames=[u8(4, 4, 3)], image_size=32, out=torch.zeros(2, 3, 32, 32)), "out"),
        (dict(frames=[u8(4, 4, 3)], image_size=32, out=torch.zeros(1, 3, 32, 32, dtype=torch.float64)), "out"),
    ]
    for kw, pattern in bad:
        with pytest.raises(ValueError, match=pattern):
            yt.preprocess_frames(**kw)
    with pytest.raises(ValueError, match="frame 1.*frame 0 is"):
        yt.frames_to_rgb([u8(4, 4, 3), u8(4, 6, 3)], "rgb")
    with pytest.raises(ValueError, match="frame 1: 40 x 64 resizes to 20 x 32.*canvas 16 x 32"):
        F._check_fits([(8, 64), (40, 64)], 32, (16, 32))
    F._check_fits([(8, 64), (40, 64)], 32, (32, 32))
    with pytest.raises(ValueError, match="frame 0.*even"):
        yt.FrameStager(2, 7, 8, "nv12", 32)
    with pytest.raises(ValueError, match="format"):
        yt.FrameStager(2, 8, 8, "i420", 32)
    with pytest.raises(ValueError, match="boxes"):
        yt.boxes_to_frames(torch.zeros(2, 3, 5), torch.zeros(2, 6, dtype=torch.int32), (32, 32))
    with pytest.raises(ValueError, match="meta"):
        yt.boxes_to_frames(torch.zeros(2, 3, 6), torch.zeros(2, 6), (32, 32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.boxes_to_frames(torch.zeros(2, 3, 6), torch.zeros(2, 6, dtype=torch.int32), (32, 32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.preprocess_frames([u8(4, 4, 3)], device="cpu")


def test_reference_canvas_is_the_librarys(built):
    lib = built.lib()
    shapes = [(60, 100), (50, 40), (31, 17), (7, 9), (64, 33)]
    for rect in (0, 1):
        for sub in (shapes, shapes[:1], shapes[1:2], [(30, 100), (40, 90)]):
            hw = (C.c_int32 * (2 * len(sub)))(*[v for s in sub for v in s])
            canvas = (C.c_int32 * 2)()
            assert lib.yolo_letterbox_canvas(hw, len(sub), 64, rect, canvas) == 0
            assert tuple(canvas) == R.canvas_hw(sub, 64, bool(rect))
