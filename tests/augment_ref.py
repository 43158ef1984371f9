"""numpy restatement of the training augmentation (csrc/augment.hip) — TEST INFRASTRUCTURE ONLY.  **PARITY UNPINNED.**

The reference runs ``config.set_train_transforms`` (config.py:60-87) and, with ``MOSAIC``, ``mosaic_augmentation``
(utils.py:503-662) through albumentations 1.x and OpenCV, neither of which is installed here. This file restates their
published uint8 algorithms — OpenCV ``RGB2HSV_b`` / ``HSV2RGB_b`` (hrange 180), ``warpAffine`` INTER_LINEAR (AB_BITS 10,
INTER_BITS 5, 15-bit bilinear table, constant border per tap), the resize of ``oracle.preprocess.resize_linear_u8`` — and
albumentations' box rules (yolo <-> (x_min, y_min, x_max, y_max), clip, ``calculate_bbox_area``, ``filter_bboxes`` with
``min_visibility`` 0.4). The kernels are tested bit for bit against it; the mosaic box arithmetic is also pinned to the
reference's own ``mosaic_augmentation`` by ``tests/golden/mosaic_boxes.npz``.

Parameter row (float64): ``[do_hsv, hue, sat, val, do_ssr, scale, dx, dy, do_flip, (mx_k, my_k) for k < 10]``.
"""
from __future__ import annotations

import numpy as np

from oracle.preprocess import py3round, resize_linear_u8

NPARAM = 29
DO_HSV, HUE, SAT, VAL, DO_SSR, SCALE, DX, DY, DO_FLIP, MOSAIC = range(10)


def resized_hw(h, w, size):
    scale = size / float(max(h, w))
    nh, nw = (py3round(h * scale), py3round(w * scale)) if scale != 1.0 else (h, w)
    return max(nh, 1), max(nw, 1)


# ------------------------------------------------------------------------------------------------- pixels
def rgb2hsv_u8(img):
    """OpenCV RGB2HSV_b: integer arithmetic, hsv_shift 12, H in [0, 180)."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    sdiv = np.where(v > 0, np.rint(1044480.0 / np.maximum(v, 1).astype(np.float64)), 0).astype(np.int64)
    hdiv = np.where(diff > 0, np.rint(737280.0 / (6.0 * np.maximum(diff, 1).astype(np.float64))), 0).astype(np.int64)
    s = (diff * sdiv + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))))
    h = (h * hdiv + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def hsv2rgb_u8(h, s, v):
    """OpenCV HSV2RGB_b: fp32 arithmetic, saturate_cast<uchar>(x * 255) = round half to even, clamp."""
    f32 = np.float32
    fs = s.astype(f32) * f32(1.0 / 255.0)
    fv = v.astype(f32) * f32(1.0 / 255.0)
    hh = h.astype(f32) * (f32(6.0) / f32(180.0))
    hh = np.fmod(hh, f32(6.0))
    sector = np.floor(hh).astype(np.int64)
    hh = hh - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hh = np.where(bad, f32(0), hh).astype(f32)
    one = f32(1.0)
    tab = np.stack([fv, fv * (one - fs), fv * (one - fs * hh), fv * (one - fs * (one - hh))], -1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    bf = np.take_along_axis(tab, sd[sector, 0][..., None], -1)[..., 0]
    gf = np.take_along_axis(tab, sd[sector, 1][..., None], -1)[..., 0]
    rf = np.take_along_axis(tab, sd[sector, 2][..., None], -1)[..., 0]
    gray = fs == 0
    rf, gf, bf = (np.where(gray, fv, t) for t in (rf, gf, bf))
    out = np.stack([rf, gf, bf], -1).astype(f32) * f32(255.0)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def hsv_shift(img, hue, sat, val):
    """albumentations _shift_hsv_uint8: HSV round trip through LUTs; identity when all three shifts are 0."""
    if hue == 0 and sat == 0 and val == 0:
        return img.copy()
    h, s, v = rgb2hsv_u8(img)
    lut = np.arange(256, dtype=np.int16)
    lut_h = np.mod(lut + hue, 180).astype(np.uint8)
    lut_s = np.clip(lut + sat, 0, 255).astype(np.uint8)
    lut_v = np.clip(lut + val, 0, 255).astype(np.uint8)
    return hsv2rgb_u8(lut_h[h].astype(np.int64), lut_s[s].astype(np.int64), lut_v[v].astype(np.int64))


def ssr_matrix(scale, dx, dy, H, W):
    """getRotationMatrix2D((W/2, H/2), 0, scale) with (dx W, dy H) added to the translation column."""
    alpha, beta = scale, 0.0 * scale
    cx, cy = 0.5 * W, 0.5 * H
    m = [alpha, beta, (1.0 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1.0 - alpha) * cy]
    m[2] += dx * W
    m[5] += dy * H
    return m


def warp_affine_u8(img, m):
    """cv2.warpAffine(img, m, (W, H), INTER_LINEAR, BORDER_CONSTANT, 0) in OpenCV's fixed point."""
    H, W, _ = img.shape
    m = list(m)
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    xs = np.arange(W, dtype=np.float64)
    ys = np.arange(H, dtype=np.float64)
    adelta = np.rint(m[0] * xs * 1024).astype(np.int64)
    bdelta = np.rint(m[3] * xs * 1024).astype(np.int64)
    X0 = np.rint((m[1] * ys + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * ys + m[5]) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
    src = img.astype(np.int64)
    acc = np.zeros((H, W, 3), np.int64)
    for t, wt in enumerate(((32 - ay) * (32 - ax) * 32, (32 - ay) * ax * 32, ay * (32 - ax) * 32, ay * ax * 32)):
        ty, tx = sy + (t >> 1), sx + (t & 1)
        ok = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        v = src[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)] * ok[..., None]
        acc += v * wt[..., None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def letterbox_u8(img, H, W):
    h, w, _ = img.shape
    nh, nw = resized_hw(h, w, max(H, W))
    top, left = (H - nh) // 2, (W - nw) // 2
    canvas = np.zeros((H, W, 3), np.uint8)
    canvas[top:top + nh, left:left + nw] = resize_linear_u8(img, nh, nw)
    return canvas


def to_float_chw(img):
    return np.ascontiguousarray((img.astype(np.float32) * np.float32(1.0 / 255.0)).transpose(2, 0, 1))


def augment_pixels(u8, p):
    """HueSaturationValue -> ShiftScaleRotate -> HorizontalFlip on a uint8 HWC canvas (the staging buffer's rounding)."""
    H, W, _ = u8.shape
    if p[DO_HSV]:
        u8 = hsv_shift(u8, p[HUE], p[SAT], p[VAL])
    if p[DO_SSR]:
        u8 = warp_affine_u8(u8, ssr_matrix(p[SCALE], p[DX], p[DY], H, W))
    if p[DO_FLIP]:
        u8 = u8[:, ::-1]
    return u8


# ------------------------------------------------------------------------------------------------- boxes
def clip01(v):
    return min(max(v, 0.0), 1.0)


def yolo_to_albu(cx, cy, w, h):
    x0, y0 = cx - w / 2, cy - h / 2
    return [clip01(x0), clip01(y0), clip01(x0 + w), clip01(y0 + h)]


def area_nz(b, H, W):
    return (b[2] * W - b[0] * W) * (b[3] * H - b[1] * H) != 0.0


def finish_box(b, cls, p, H, W):
    """ShiftScaleRotate (+ clip, min_visibility 0.4), HorizontalFlip, back to yolo; None when dropped."""
    b = list(b)
    if p[DO_SSR]:
        m = ssr_matrix(p[SCALE], p[DX], p[DY], H, W)
        t = [(m[0] * (b[0] * W) + m[2]) / W, (m[4] * (b[1] * H) + m[5]) / H, (m[0] * (b[2] * W) + m[2]) / W,
             (m[4] * (b[3] * H) + m[5]) / H]
        ta = (t[2] * W - t[0] * W) * (t[3] * H - t[1] * H)
        b = [clip01(v) for v in t]
        ca = (b[2] * W - b[0] * W) * (b[3] * H - b[1] * H)
        if not (ca != 0.0 and ca / ta >= 0.4):
            return None
    if p[DO_FLIP]:
        b[0], b[2] = 1.0 - b[2], 1.0 - b[0]
    return [(b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0, b[2] - b[0], b[3] - b[1], float(cls)]


def standard_boxes(boxes, hw, p, H, W):
    h, w = hw
    nh, nw = resized_hw(h, w, max(H, W))
    top, left = (H - nh) // 2, (W - nw) // 2
    out = []
    for bx in boxes:
        b = yolo_to_albu(*[float(v) for v in bx[:4]])
        if not area_nz(b, nh, nw):
            continue
        b = [(b[0] * nw + left) / W, (b[1] * nh + top) / H, (b[2] * nw + left) / W, (b[3] * nh + top) / H]
        r = finish_box(b, bx[4], p, H, W)
        if r is not None:
            out.append(r)
    return out


def mosaic_tile_boxes(quad_boxes, h, w, S):
    """Boxes of the four quadrants in the padded 2S x 2S mosaic, yolo + class, in concatenation order (utils.py:546-592)."""
    out = []
    for q, boxes in enumerate(quad_boxes):
        for bx in boxes or []:
            b = yolo_to_albu(*[float(v) for v in bx[:4]])
            if not area_nz(b, h, w):
                continue
            cx, cy, bw, bh = (b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0, b[2] - b[0], b[3] - b[1]
            cx, cy, bw, bh = cx / 2, cy / 2, bw / 2, bh / 2
            if q & 1:
                cx += 0.5
            if q & 2:
                cy += 0.5
            b = yolo_to_albu(cx, cy, bw, bh)
            if not area_nz(b, 2 * h, 2 * w):
                continue
            top, left = (2 * S - 2 * h) // 2, (2 * S - 2 * w) // 2
            b = [(b[0] * (2 * w) + left) / (2 * S), (b[1] * (2 * h) + top) / (2 * S), (b[2] * (2 * w) + left) / (2 * S),
                 (b[3] * (2 * h) + top) / (2 * S)]
            if not area_nz(b, 2 * S, 2 * S):
                continue
            out.append([(b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0, b[2] - b[0], b[3] - b[1], float(bx[4])])
    return out


def _hit(o, a, x, y):
    u, v = o[0], o[1]
    for _ in range(a + 1):                 # the reference re-applies cx -> x1 on every attempt (utils.py:607-608)
        u = u - o[2] / 2
        v = v - o[3] / 2
    xa, ya, xb, yb = max(u, x), max(v, y), min(u + o[2], x + 0.5), min(v + o[3], y + 0.5)
    return max(0.0, xb - xa) * max(0.0, yb - ya) > 0.0, u, v


def mosaic_cutout(tile, draws):
    """Cutout choice and box arithmetic of utils.py:597-659 on the tile boxes; (attempt, boxes yolo + class in cutout units)
    or (-1, None) when no attempt hits a box (and when there is no box at all)."""
    for a in range(10 if tile else 0):
        x, y = draws[2 * a], draws[2 * a + 1]
        if any(_hit(o, a, x, y)[0] for o in tile):
            out = []
            for o in tile:
                ok, bx, by = _hit(o, a, x, y)
                if not ok:
                    continue
                bw, bh = o[2], o[3]
                if bx < x:
                    bw -= x - bx; bx = x
                if by < y:
                    bh -= y - by; by = y
                if bx >= x:
                    bx -= x
                if by >= y:
                    by -= y
                if bw + bx > x + 0.5:
                    bw = (x + 0.5) - bx
                if bh + by > y + 0.5:
                    bh = (y + 0.5) - by
                bx, by, bw, bh = bx * 2, by * 2, bw * 2, bh * 2
                out.append([bx + bw / 2, by + bh / 2, bw, bh, o[4]])
            return a, out
    return -1, None


def augment_one(images, boxes, src, p, H, W):
    """One output image: (x (3, H, W) fp32, boxes [[x, y, w, h, cls]] as fp32, path) with path -2 letterbox only, -1 standard,
    a >= 0 mosaic cutout draw a. ``images`` / ``boxes`` are the pool; ``src`` the four slots (-1 = unused)."""
    p = [float(v) for v in p]
    s0 = src[0]
    if boxes[s0] is None:
        return to_float_chw(letterbox_u8(images[s0], H, W)), [], -2
    if src[1] >= 0:
        S = W
        h, w = resized_hw(*images[s0].shape[:2], S)
        tile = mosaic_tile_boxes([boxes[k] for k in src], h, w, S)
        a, cut = mosaic_cutout(tile, p[MOSAIC:MOSAIC + 20])
        if a >= 0:
            big = np.full((2 * S, 2 * S, 3), 255, np.uint8)
            top, left = (2 * S - 2 * h) // 2, (2 * S - 2 * w) // 2
            for q, k in enumerate(src):
                oy, ox = top + (q >> 1) * h, left + (q & 1) * w
                big[oy:oy + h, ox:ox + w] = resize_linear_u8(images[k], h, w)
            xp, yp = int(p[MOSAIC + 2 * a] * 2 * S), int(p[MOSAIC + 2 * a + 1] * 2 * S)
            u8 = big[yp:yp + S, xp:xp + S]
            out = []
            for c in cut:
                b = yolo_to_albu(*c[:4])
                if not area_nz(b, S, S):
                    continue
                r = finish_box(b, c[4], p, S, S)
                if r is not None:
                    out.append(r)
            return to_float_chw(augment_pixels(u8, p)), _f32(out), a
    u8 = letterbox_u8(images[s0], H, W)
    return to_float_chw(augment_pixels(u8, p)), _f32(standard_boxes(boxes[s0], images[s0].shape[:2], p, H, W)), -1


def _f32(rows):
    return [[float(np.float32(v)) for v in r] for r in rows]


def augment(images, boxes, params, H, W, mosaic=None):
    """The whole batch: (x (B, 3, H, W) fp32, list of per-image box lists, paths)."""
    B = len(images) if mosaic is None else len(mosaic)
    srcs = [[b, -1, -1, -1] for b in range(B)] if mosaic is None else [[int(v) for v in r] for r in mosaic]
    xs, bs, paths = [], [], []
    for b in range(B):
        x, bx, path = augment_one(images, boxes, srcs[b], params[b], H, W)
        xs.append(x); bs.append(bx); paths.append(path)
    return np.stack(xs), bs, paths
