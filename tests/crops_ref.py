"""numpy restatement of training on tiles (csrc/crops.hip) — TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED.**

Written from the contract in include/yolo_mi355x.h ("training on tiles"): the window of a crop, the boxes remapped to it and
filtered by visibility, the pixels of its level. The pieces it shares with the training augmentation - the box chain
(``finish_box``), the pixel chain (``augment_pixels``), the uint8 INTER_LINEAR resize and the normalisation - are imported from
tests/augment_ref.py, not restated.

Crop parameter row (float64): ``[u_pick, background, jx, jy, scale]``. Python floats are IEEE doubles and every expression below is
written operation by operation, so the arithmetic is the kernel's (fp64, every operation rounded once).
"""
from __future__ import annotations

import math

import numpy as np

from tests import augment_ref as ar
from tests.augment_ref import area_nz, augment_pixels, clip01, finish_box, resize_linear_u8, to_float_chw, yolo_to_albu

NPARAM = 5
U_PICK, BACKGROUND, JX, JY, SCALE = range(5)


def level_hw(h, w, scale):
    """yolo_tile_level_hw: max(1, rint(side * scale)), half to even; a scale outside (0, 8] is taken as 1."""
    if not (scale > 0.0 and scale <= 8.0):
        scale = 1.0
    return max(1, int(np.rint(h * scale))), max(1, int(np.rint(w * scale)))


def _origin(L, t, j, obj, c):
    if L <= t:
        return 0
    v = math.floor(c * L - j * (t - 1)) if obj else math.floor(j * (L - t + 1))
    return int(min(max(v, 0), L - t))


def window(hw, boxes, cp, th, tw, origin=None):
    """The windows row of one crop without its image index: (y0, x0, LH, LW, picked)."""
    cp = [float(v) for v in cp]
    LH, LW = level_hw(hw[0], hw[1], cp[SCALE])
    if origin is not None:
        return int(origin[0]), int(origin[1]), LH, LW, -1
    nb = 0 if boxes is None else len(boxes)
    picked, cx, cy = -1, 0.0, 0.0
    if cp[BACKGROUND] == 0.0 and nb > 0:
        picked = min(int(math.floor(cp[U_PICK] * nb)), nb - 1)
        cx, cy = float(boxes[picked][0]), float(boxes[picked][1])
    x0 = _origin(LW, tw, cp[JX], picked >= 0, cx)
    y0 = _origin(LH, th, cp[JY], picked >= 0, cy)
    return y0, x0, LH, LW, picked


def crop_boxes(hw, boxes, win, th, tw, min_visibility=0.4, p=None):
    """The kept rows of one crop, [[x, y, w, h, cls]] in fp64 (the caller rounds to fp32 as the store does)."""
    y0, x0, LH, LW, _ = win
    h, w = hw
    out = []
    for bx in boxes or []:
        b = yolo_to_albu(*[float(v) for v in bx[:4]])
        if not area_nz(b, h, w):
            continue
        t = [(b[0] * LW - x0) / tw, (b[1] * LH - y0) / th, (b[2] * LW - x0) / tw, (b[3] * LH - y0) / th]
        ta = (t[2] * tw - t[0] * tw) * (t[3] * th - t[1] * th)
        c = [clip01(v) for v in t]
        ca = (c[2] * tw - c[0] * tw) * (c[3] * th - c[1] * th)
        if not (ca != 0.0 and ca / ta >= min_visibility):
            continue
        if p is not None:
            r = finish_box(c, bx[4], p, th, tw)
            if r is not None:
                out.append(r)
        else:
            out.append([(c[0] + c[2]) / 2.0, (c[1] + c[3]) / 2.0, c[2] - c[0], c[3] - c[1], float(bx[4])])
    return out


_LEVELS = {}


def level_u8(img, LH, LW):
    """The image resized to its (LH, LW) level; computed once per (image, level) and shared (never written to)."""
    key = (id(img), LH, LW)
    if key not in _LEVELS:
        _LEVELS[key] = (img, resize_linear_u8(img, LH, LW))      # the image is kept so that its id stays taken
    return _LEVELS[key][1]


def canvas_u8(img, win, th, tw):
    """The uint8 (th, tw, 3) staging canvas of one crop before the HSV shift: level pixels, 0 outside the level."""
    y0, x0, LH, LW, _ = win
    lev = level_u8(img, LH, LW)
    out = np.zeros((th, tw, 3), np.uint8)
    ya, yb, xa, xb = max(y0, 0), min(y0 + th, LH), max(x0, 0), min(x0 + tw, LW)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = lev[ya:yb, xa:xb]
    return out


def crop_one(img, boxes, cp, th, tw, origin=None, p=None, min_visibility=0.4):
    """One crop: (x (3, th, tw) fp32, boxes as fp32-rounded rows, (y0, x0, LH, LW, picked))."""
    win = window(img.shape[:2], boxes, cp, th, tw, origin)
    p = None if p is None else [float(v) for v in p]
    u8 = canvas_u8(img, win, th, tw)
    if p is not None:
        u8 = augment_pixels(u8, p)
    rows = crop_boxes(img.shape[:2], boxes, win, th, tw, min_visibility, p)
    return to_float_chw(u8), ar._f32(rows), win


def crop(images, boxes, index, crop_params, th, tw, origins=None, params=None, min_visibility=0.4):
    """The whole batch: (x (B, 3, th, tw) fp32, list of per-crop box lists, windows (B, 6) int32)."""
    xs, bs, ws = [], [], []
    for b, k in enumerate(index):
        k = int(k)
        x, rows, win = crop_one(images[k], boxes[k], crop_params[b], th, tw, None if origins is None else origins[b],
                                None if params is None else params[b], min_visibility)
        xs.append(x); bs.append(rows); ws.append([k, *win])
    return np.stack(xs), bs, np.asarray(ws, np.int32).reshape(-1, 6)
