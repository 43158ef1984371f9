"""TEST INFRASTRUCTURE ONLY: a numpy restatement of the frame front end's contract (include/yolo_mi355x.h), written
from the formulas and not from csrc/frames.hip. NV12 -> RGB in 20-bit fixed point, the three derived constant sets from the
standards' Kr and Kb in exact rationals (BT.601 limited range carries OpenCV's literals, as the contract says); BGR is a channel flip;
the letterbox is ``oracle.preprocess.resize_linear_u8`` with the size, canvas and centring rules of ``yolo_letterbox_hw``; the
unletterbox is the Python expression of ``unletterbox_boxes(meta=)`` rounded to fp32. **PARITY UNPINNED** against cv2, like the oracle."""
from fractions import Fraction as F

import numpy as np

from oracle import preprocess as opre

CSC_KINDS = ("bt601", "bt601-full", "bt709", "bt709-full")
KR_KB = {"bt601": (F(299, 1000), F(114, 1000)), "bt709": (F(2126, 10000), F(722, 10000))}
OPENCV_BT601 = (1220542, 1673527, -852492, -409993, 2116026, 16)          # ITUR_BT_601_CY, _CVR, _CVG, _CUG, _CUB; the luma offset


def derived_constants(csc):
    """(CY, CVR, CVG, CUG, CUB, yoff) = round(c 2^20) of the exact coefficients: with Kg = 1 - Kr - Kb, R = Y' + 2 (1 - Kr) Cr,
    B = Y' + 2 (1 - Kb) Cb, G = Y' - 2 Kr (1 - Kr) / Kg Cr - 2 Kb (1 - Kb) / Kg Cb; limited range: Y' = (Y - 16) / 219 and
    C = (c - 128) / 224, full range: Y' = Y / 255 and C = (c - 128) / 255; the output is 255 R, 255 G, 255 B."""
    kr, kb = KR_KB[csc.split("-")[0]]
    full = csc.endswith("-full")
    kg = 1 - kr - kb
    sy, sc = (F(1), F(1)) if full else (F(255, 219), F(255, 224))
    one = 1 << 20
    return (round(sy * one), round(2 * (1 - kr) * sc * one), round(-2 * kr * (1 - kr) / kg * sc * one),
            round(-2 * kb * (1 - kb) / kg * sc * one), round(2 * (1 - kb) * sc * one), 0 if full else 16)


def constants(csc):
    return OPENCV_BT601 if csc == "bt601" else derived_constants(csc)


def unpitch(buf, h, w, pitch, fmt):
    """The tight frame of a pitched surface: (h, w, 3) or (h * 3 / 2, w)."""
    rows, row = (h * 3 // 2, w) if fmt == "nv12" else (h, 3 * w)
    flat = np.asarray(buf, np.uint8).reshape(-1)
    out = np.stack([flat[r * pitch:r * pitch + row] for r in range(rows)])
    return out if fmt == "nv12" else out.reshape(h, w, 3)


def nv12_to_rgb(nv12, csc):
    """(h * 3 / 2, w) uint8 -> (h, w, 3) uint8 RGB; chroma replicated over its 2 x 2 block."""
    cy, cvr, cvg, cug, cub, yoff = constants(csc)
    h, w = nv12.shape[0] * 2 // 3, nv12.shape[1]
    assert h % 2 == 0 and w % 2 == 0
    Y = nv12[:h].astype(np.int64)
    uv = nv12[h:].reshape(h // 2, w // 2, 2).astype(np.int64) - 128
    u = np.repeat(np.repeat(uv[:, :, 0], 2, 0), 2, 1)
    v = np.repeat(np.repeat(uv[:, :, 1], 2, 0), 2, 1)
    y = np.maximum(0, Y - yoff) * cy + (1 << 19)
    rgb = np.stack([(y + cvr * v) >> 20, (y + cvg * v + cug * u) >> 20, (y + cub * u) >> 20], -1)          # >> on int64: arithmetic
    return np.clip(rgb, 0, 255).astype(np.uint8)


def to_rgb(frame, fmt, csc="bt601"):
    """A frame (an array, or a (buffer, h, w, pitch) surface) as packed RGB uint8."""
    if isinstance(frame, tuple):
        frame = unpitch(frame[0], frame[1], frame[2], frame[3], fmt)
    frame = np.asarray(frame, np.uint8)
    if fmt == "nv12":
        return nv12_to_rgb(frame, csc)
    return np.ascontiguousarray(frame[:, :, ::-1]) if fmt == "bgr" else frame


def resized_hw(h, w, size):
    scale = size / float(max(h, w))
    nh, nw = (opre.py3round(h * scale), opre.py3round(w * scale)) if scale != 1.0 else (h, w)
    return max(nh, 1), max(nw, 1)


def canvas_hw(shapes, size, rect):
    if not rect:
        return size, size
    r = [resized_hw(h, w, size) for h, w in shapes]
    return (max(a for a, _ in r) + 31) // 32 * 32, (max(b for _, b in r) + 31) // 32 * 32


def letterbox_rgb(rgb, size, canvas):
    """(3, Hc, Wc) fp32 and the meta row of one packed RGB frame."""
    h, w, _ = rgb.shape
    nh, nw = resized_hw(h, w, size)
    top, left = (canvas[0] - nh) // 2, (canvas[1] - nw) // 2
    cv = np.zeros((canvas[0], canvas[1], 3), np.uint8)
    cv[top:top + nh, left:left + nw] = opre.resize_linear_u8(rgb, nh, nw)
    out = cv.astype(np.float32) * np.float32(1.0 / 255.0)
    return np.ascontiguousarray(out.transpose(2, 0, 1)), (h, w, nh, nw, top, left)


def preprocess(frames, size, fmt, csc="bt601", rect=False):
    """The contract of preprocess_frames: (x (B, 3, Hc, Wc) fp32, meta (B, 6) int32)."""
    rgbs = [to_rgb(f, fmt, csc) for f in frames]
    canvas = canvas_hw([r.shape[:2] for r in rgbs], size, rect)
    xs, metas = zip(*[letterbox_rgb(r, size, canvas) for r in rgbs])
    return np.stack(xs), np.array(metas, np.int32)


def unletterbox(boxes, meta, canvas):
    """boxes (B, N, 6) fp32, meta (B, 6), canvas (Hc, Wc) -> fp32: the expression of unletterbox_boxes(meta=) on Python floats,
    rounded once."""
    r_h, r_w = (int(v) for v in canvas)
    out = np.empty(boxes.shape, np.float32)
    for s in range(boxes.shape[0]):
        _, _, new_height, new_width, pad_height, pad_width = (int(v) for v in meta[s])
        for j in range(boxes.shape[1]):
            b = [float(v) for v in boxes[s, j]]
            with np.errstate(all="ignore"):
                row = [np.float64(b[0] * r_w - pad_width) / new_width, np.float64(b[1] * r_h - pad_height) / new_height,
                       np.float64(b[2] * r_w) / new_width, np.float64(b[3] * r_h) / new_height, b[4], b[5]]
                out[s, j] = np.array(row, np.float64).astype(np.float32)
    return out
