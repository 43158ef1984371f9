"""numpy restatement of the augmentation extras (csrc/augment.h: rotation, vertical flip, MixUp, Cutout) — TEST INFRASTRUCTURE
ONLY.  **PARITY UNPINNED.**

Written from the contract in include/yolo_mi355x.h ("augmentation extras"). cv2 and albumentations are not installed here; the
rules are the published ones: ``getRotationMatrix2D``, the ``largest_box`` method of albumentations 1.x
``bbox_shift_scale_rotate``, and the erase-and-drop rule of the common YOLO Cutout. Everything the extras do not change - the
letterbox, the mosaic, the crop window, the HSV shift, the fixed-point warp, the box rules - is imported from tests/augment_ref.py
and tests/crops_ref.py, not restated; only the orchestration of one row is repeated here, with the rotated matrix, the four-corner
box rule and the vertical flip put in.

Extras row (float64, 24): ``[cos, sin, do_vflip, mix_partner, mix_lambda, cut_n, cut_cover, cut_fill, (x0, y0, x1, y1) k < 4]``.
Python floats are IEEE doubles and every expression is written operation by operation, so the arithmetic is the kernel's.
"""
from __future__ import annotations

import math

import numpy as np

from tests import augment_ref as ar
from tests import crops_ref as cr

NPARAM = 24
ROT_COS, ROT_SIN, DO_VFLIP, MIX_PARTNER, MIX_LAMBDA, CUT_N, CUT_COVER, CUT_FILL, CUT_RECT = range(9)


def neutral(n):
    """The table with which every call gives the bits of the call without extras."""
    e = np.zeros((n, NPARAM), np.float64)
    e[:, ROT_COS] = 1.0
    e[:, MIX_PARTNER] = -1.0
    e[:, MIX_LAMBDA] = 1.0
    return e


def ssr_matrix(p, e, H, W):
    """getRotationMatrix2D((W/2, H/2), theta, scale) with (dx W, dy H) added to the translation column."""
    alpha, beta = p[ar.SCALE] * e[ROT_COS], p[ar.SCALE] * e[ROT_SIN]
    cx, cy = 0.5 * W, 0.5 * H
    m = [alpha, beta, (1.0 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1.0 - alpha) * cy]
    m[2] += p[ar.DX] * W
    m[5] += p[ar.DY] * H
    return m


def chain_box(b, p, e, H, W):
    """ShiftScaleRotate with the rotation (largest_box) + clip + min_visibility 0.4, both flips; albumentations box or None."""
    b = list(b)
    if p[ar.DO_SSR]:
        m = ssr_matrix(p, e, H, W)
        if e[ROT_COS] == 1.0 and e[ROT_SIN] == 0.0:
            t = [(m[0] * (b[0] * W) + m[2]) / W, (m[4] * (b[1] * H) + m[5]) / H, (m[0] * (b[2] * W) + m[2]) / W,
                 (m[4] * (b[3] * H) + m[5]) / H]
        else:
            xs, ys = [], []
            for x, y in ((b[0], b[1]), (b[2], b[1]), (b[0], b[3]), (b[2], b[3])):
                px, py = x * W, y * H
                xs.append((m[0] * px + m[1] * py + m[2]) / W)
                ys.append((m[3] * px + m[4] * py + m[5]) / H)
            t = [min(xs), min(ys), max(xs), max(ys)]
        ta = (t[2] * W - t[0] * W) * (t[3] * H - t[1] * H)
        b = [ar.clip01(v) for v in t]
        ca = (b[2] * W - b[0] * W) * (b[3] * H - b[1] * H)
        if not (ca != 0.0 and ca / ta >= 0.4):
            return None
    if p[ar.DO_FLIP]:
        b[0], b[2] = 1.0 - b[2], 1.0 - b[0]
    if e[DO_VFLIP]:
        b[1], b[3] = 1.0 - b[3], 1.0 - b[1]
    return b


def chain_pixels(u8, p, e):
    """HueSaturationValue -> ShiftScaleRotate with the rotation -> HorizontalFlip -> VerticalFlip on a uint8 HWC canvas."""
    H, W, _ = u8.shape
    if p[ar.DO_HSV]:
        u8 = ar.hsv_shift(u8, p[ar.HUE], p[ar.SAT], p[ar.VAL])
    if p[ar.DO_SSR]:
        u8 = ar.warp_affine_u8(u8, ssr_matrix(p, e, H, W))
    if p[ar.DO_FLIP]:
        u8 = u8[:, ::-1]
    if e[DO_VFLIP]:
        u8 = u8[::-1]
    return u8


def cut_rects(e, H, W):
    """The erase rectangles of a row in pixels, [(X0, Y0, X1, Y1)]: truncation of the clipped corner times the canvas side."""
    n = int(e[CUT_N]) if e[CUT_N] >= 1.0 else 0
    out = []
    for k in range(min(n, 4)):
        x0, y0, x1, y1 = (0.0 if math.isnan(v) else ar.clip01(v) for v in e[CUT_RECT + 4 * k:CUT_RECT + 4 * k + 4])
        out.append((int(x0 * W), int(y0 * H), int(x1 * W), int(y1 * H)))
    return out


def cut_drops(b, e, H, W):
    """Cutout's box rule: more than CUT_COVER of the box inside ONE rectangle (strict)."""
    lim = e[CUT_COVER] * ((b[2] - b[0]) * (b[3] - b[1]))
    for X0, Y0, X1, Y1 in cut_rects(e, H, W):
        if X1 <= X0 or Y1 <= Y0:
            continue
        R = (X0 / W, Y0 / H, X1 / W, Y1 / H)
        inter = max(0.0, min(b[2], R[2]) - max(b[0], R[0])) * max(0.0, min(b[3], R[3]) - max(b[1], R[1]))
        if inter > lim:
            return True
    return False


def partner(e, b, B):
    v = float(e[MIX_PARTNER])
    if not (0.0 <= v < B) or v != math.floor(v) or int(v) == b:
        return -1
    return int(v)


def _yolo(b, cls):
    return [(b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0, b[2] - b[0], b[3] - b[1], float(cls)]


# ------------------------------------------------------------------------------------------------- chain(r) of the two users
def augment_chain(images, boxes, src, p, e, H, W):
    """chain(r) of augment_batch: (uint8 HWC output canvas, [(albumentations box, class)]); augment_ref.augment_one with the
    extras' box chain and pixel chain in place of finish_box / augment_pixels."""
    s0 = src[0]
    if boxes[s0] is None:
        return ar.letterbox_u8(images[s0], H, W), []          # letterbox only: no transform of its own, no extras of its own
    if src[1] >= 0:
        S = W
        h, w = ar.resized_hw(*images[s0].shape[:2], S)
        tile = ar.mosaic_tile_boxes([boxes[k] for k in src], h, w, S)
        a, cut = ar.mosaic_cutout(tile, p[ar.MOSAIC:ar.MOSAIC + 20])
        if a >= 0:
            big = np.full((2 * S, 2 * S, 3), 255, np.uint8)
            top, left = (2 * S - 2 * h) // 2, (2 * S - 2 * w) // 2
            for q, k in enumerate(src):
                oy, ox = top + (q >> 1) * h, left + (q & 1) * w
                big[oy:oy + h, ox:ox + w] = ar.resize_linear_u8(images[k], h, w)
            xp, yp = int(p[ar.MOSAIC + 2 * a] * 2 * S), int(p[ar.MOSAIC + 2 * a + 1] * 2 * S)
            out = []
            for c in cut:
                b = ar.yolo_to_albu(*c[:4])
                if ar.area_nz(b, S, S):
                    r = chain_box(b, p, e, S, S)
                    if r is not None:
                        out.append((r, c[4]))
            return chain_pixels(big[yp:yp + S, xp:xp + S], p, e), out
    h, w = images[s0].shape[:2]
    nh, nw = ar.resized_hw(h, w, max(H, W))
    top, left = (H - nh) // 2, (W - nw) // 2
    out = []
    for bx in boxes[s0]:
        b = ar.yolo_to_albu(*[float(v) for v in bx[:4]])
        if not ar.area_nz(b, nh, nw):
            continue
        b = [(b[0] * nw + left) / W, (b[1] * nh + top) / H, (b[2] * nw + left) / W, (b[3] * nh + top) / H]
        r = chain_box(b, p, e, H, W)
        if r is not None:
            out.append((r, bx[4]))
    return chain_pixels(ar.letterbox_u8(images[s0], H, W), p, e), out


def crop_chain(img, boxes, cp, p, e, th, tw, origin=None, min_visibility=0.4):
    """chain(r) of CropPool.batch: (uint8 canvas, [(box, class)], window); crops_ref.crop_one with the extras' chains."""
    win = cr.window(img.shape[:2], boxes, cp, th, tw, origin)
    y0, x0, LH, LW, _ = win
    h, w = img.shape[:2]
    out = []
    for bx in boxes or []:
        b = ar.yolo_to_albu(*[float(v) for v in bx[:4]])
        if not ar.area_nz(b, h, w):
            continue
        t = [(b[0] * LW - x0) / tw, (b[1] * LH - y0) / th, (b[2] * LW - x0) / tw, (b[3] * LH - y0) / th]
        ta = (t[2] * tw - t[0] * tw) * (t[3] * th - t[1] * th)
        c = [ar.clip01(v) for v in t]
        ca = (c[2] * tw - c[0] * tw) * (c[3] * th - c[1] * th)
        if not (ca != 0.0 and ca / ta >= min_visibility):
            continue
        r = chain_box(c, p, e, th, tw)
        if r is not None:
            out.append((r, bx[4]))
    return chain_pixels(cr.canvas_u8(img, win, th, tw), p, e), out, win


# ------------------------------------------------------------------------------------------------- MixUp and Cutout on outputs
def mix_cut(chains, extra, max_out=None):
    """out[b] of every row from the rows' chains [(uint8 canvas, [(box, class)])]: (x (B, 3, H, W) fp32, per-row box lists as
    fp32-rounded yolo rows). The partner contributes its chain, whatever its own partner and rectangles say."""
    f32 = np.float32
    B = len(chains)
    H, W, _ = chains[0][0].shape
    inv = f32(1.0 / 255.0)
    xs, bs = [], []
    for b in range(B):
        e = [float(v) for v in extra[b]]
        pt = partner(e, b, B)
        x = chains[b][0].astype(f32) * inv
        kept = list(chains[b][1])
        if pt >= 0:
            l = f32(e[MIX_LAMBDA])
            m = f32(1.0) - l
            x = x * l + (chains[pt][0].astype(f32) * inv) * m
            kept += chains[pt][1]
        x = np.ascontiguousarray(x.transpose(2, 0, 1)).astype(f32)
        for X0, Y0, X1, Y1 in cut_rects(e, H, W):
            if X1 > X0 and Y1 > Y0:
                x[:, Y0:Y1, X0:X1] = f32(e[CUT_FILL])
        rows = [_yolo(bb, cls) for bb, cls in kept if not cut_drops(bb, e, H, W)]
        xs.append(x)
        bs.append(ar._f32(rows if max_out is None else rows[:max_out]))
    return np.stack(xs), bs


def augment(images, boxes, params, extra, H, W, mosaic=None, max_out=None):
    """augment_batch(..., extra=): (x, per-row box lists)."""
    B = len(images) if mosaic is None else len(mosaic)
    srcs = [[b, -1, -1, -1] for b in range(B)] if mosaic is None else [[int(v) for v in r] for r in mosaic]
    chains = [augment_chain(images, boxes, srcs[b], [float(v) for v in params[b]], [float(v) for v in extra[b]], H, W)
              for b in range(B)]
    return mix_cut(chains, extra, max_out)


def crop(images, boxes, index, crop_params, params, extra, th, tw, origins=None, min_visibility=0.4, max_out=None):
    """CropPool.batch(..., extra=): (x, per-crop box lists, windows (B, 6) int32)."""
    chains, ws = [], []
    for b, k in enumerate(index):
        k = int(k)
        u8, rows, win = crop_chain(images[k], boxes[k], crop_params[b], [float(v) for v in params[b]], [float(v) for v in extra[b]],
                                   th, tw, None if origins is None else origins[b], min_visibility)
        chains.append((u8, rows))
        ws.append([k, *win])
    x, bs = mix_cut(chains, extra, max_out)
    return x, bs, np.asarray(ws, np.float64).astype(np.int32).reshape(-1, 6)
