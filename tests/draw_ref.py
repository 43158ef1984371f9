"""A numpy restatement of the drawing contract (include/yolo_mi355x.h): one painter's loop over the selected boxes
of a frame, each box scattered into the frame with slices. The kernel does the opposite (a gather per pixel tile). Geometry in
np.float32 with one rounding per operation, blending in integers; the font is passed in as the (95, 8) table of yolo_draw_font."""
import numpy as np

F = np.float32
CLAMP = F(1048576.0)
TEXT_CAPACITY = 32


def blend(src, colour, a):
    """out = (src (255 - a) + colour a + 127) / 255 on integer arrays (or ints)."""
    return (src * (255 - a) + colour * a + 127) // 255


def unmap(box, meta, canvas_hw, center=True):
    """The fp32 unletterbox_boxes(..., meta=) of the first four numbers of a row."""
    _, _, nh, nw, pt, pl = (F(v) for v in meta)
    ch, cw = F(canvas_hw[0]), F(canvas_hw[1])
    a0, a1, a2, a3 = (F(v) for v in box[:4])
    with np.errstate(all="ignore"):
        x = F(F(F(a0 * cw) - pl) / nw)
        y = F(F(F(a1 * ch) - pt) / nh)
        if center:
            return x, y, F(F(a2 * cw) / nw), F(F(a3 * ch) / nh)
        return x, y, F(F(F(a2 * cw) - pl) / nw), F(F(F(a3 * ch) - pt) / nh)


def edges(box, h, w, center=True):
    """(l, t, r, b) in fp32 pixels, before the clamp."""
    a0, a1, a2, a3 = (F(v) for v in box[:4])
    W, H = F(w), F(h)
    with np.errstate(all="ignore"):
        if center:
            hw, hh = F(a2 / F(2)), F(a3 / F(2))
            return F(F(a0 - hw) * W), F(F(a1 - hh) * H), F(F(a0 + hw) * W), F(F(a1 + hh) * H)
        return F(a0 * W), F(a1 * H), F(a2 * W), F(a3 * H)


def edge_int(e):
    e = min(max(F(e), -CLAMP), CLAMP)
    return int(np.floor(F(e + F(0.5))))


def rectangle(box, h, w, center=True):
    """The integer box (x0, y0, x1, y1), x1 and y1 exclusive, or None for a row that draws nothing."""
    l, t, r, b = edges(box, h, w, center)
    if not all(np.isfinite(v) for v in (l, t, r, b)) or r < l or b < t:
        return None
    return edge_int(l), edge_int(t), edge_int(r), edge_int(b)


def ring(rect, thickness):
    """(outer, inner) rectangles of the outline."""
    x0, y0, x1, y1 = rect
    g = thickness // 2
    s = thickness - g
    return (x0 - g, y0 - g, x1 + g, y1 + g), (x0 + s, y0 + s, x1 - s, y1 - s)


def percent(score):
    with np.errstate(all="ignore"):
        v = np.floor(F(F(F(score) * F(100)) + F(0.5)))
    return 0 if not v >= 0 else 100 if v > 100 else int(v)


def label_text(name, track_id, score):
    """name: str or None; track_id: int or None (no ids given); score: number or None (scores off)."""
    text = "".join(c if 0x20 <= ord(c) <= 0x7E else "?" for c in (name or ""))
    if track_id is not None and track_id > 0:
        text += (" " if text else "") + "#%d" % track_id
    if score is not None:
        text += (" " if text else "") + "%02d%%" % percent(score)
    return text[:TEXT_CAPACITY]


def plate(outer, n_chars, scale, w):
    pw, ph = 6 * scale * n_chars, 8 * scale
    px0 = outer[0]
    if px0 + pw > w:
        px0 = max(0, w - pw)
    py0 = outer[1] - ph
    if py0 < 0:
        py0 = outer[1]
    return px0, py0, px0 + pw, py0 + ph


def _clip(rect, h, w):
    return max(rect[0], 0), max(rect[1], 0), min(rect[2], w), min(rect[3], h)


def draw_frame(frame, boxes, font, *, keep=None, count=None, ids=None, class_names=None, center=True, meta=None, canvas_hw=None,
               thickness=1, font_scale=1, line_alpha=255, fill_alpha=0, labels=True, scores=True, palette=None, color_by_id=False,
               touched=None):
    """One frame: ``frame`` (H, W, 3) uint8, ``boxes`` (N, 6); ``keep`` (N,), ``count`` int, ``ids`` (N,) or None. Alphas in 0 .. 255.
    Returns the drawn copy. ``touched``: an optional (H, W) bool array that receives every pixel inside a command's rectangles."""
    out = frame.astype(np.int64)
    h, w = frame.shape[:2]
    n = len(boxes)
    cnt = n if count is None else min(max(int(count), 0), n)
    palette = np.asarray(palette, dtype=np.int64)
    font = np.asarray(font).reshape(95, 8)
    for j in range(cnt):
        row = int(keep[j]) if keep is not None else j
        if not 0 <= row < n:
            continue
        box = boxes[row]
        geo = unmap(box, meta, canvas_hw, center) if meta is not None else box[:4]
        rect = rectangle(geo, h, w, center)
        if rect is None:
            continue
        tid = int(ids[row]) if ids is not None else 0
        cls = F(box[5])
        ci = int(cls) if abs(cls) <= F(2.0 ** 30) else -1            # int(): truncation; NaN and Inf fail the comparison
        named = labels and class_names is not None
        if named and not 0 <= ci < len(class_names):
            continue
        colour = palette[(tid if color_by_id else ci) % len(palette)]
        outer, inner = ring(rect, thickness)
        if outer[0] >= outer[2] or outer[1] >= outer[3] or outer[0] >= w or outer[1] >= h or outer[2] <= 0 or outer[3] <= 0:
            continue
        text = label_text(class_names[ci] if named else None, tid if ids is not None else None, box[4] if scores else None) if labels else ""
        ox0, oy0, ox1, oy1 = _clip(outer, h, w)
        ix0, iy0, ix1, iy1 = _clip(inner, h, w)
        has_inner = ix0 < ix1 and iy0 < iy1
        region = out[oy0:oy1, ox0:ox1]
        if has_inner:
            keep_inner = region[iy0 - oy0:iy1 - oy0, ix0 - ox0:ix1 - ox0].copy()
        region[...] = blend(region, colour, line_alpha)               # the ring (the inner part is put back and filled below)
        if has_inner:
            region[iy0 - oy0:iy1 - oy0, ix0 - ox0:ix1 - ox0] = blend(keep_inner, colour, fill_alpha)
        if touched is not None:
            touched[oy0:oy1, ox0:ox1] = True
        if text:
            px0, py0, px1, py1 = plate(outer, len(text), font_scale, w)
            for y in range(max(py0, 0), min(py1, h)):
                for x in range(max(px0, 0), min(px1, w)):
                    u, v = (x - px0) // font_scale, (y - py0) // font_scale
                    cell, cu = divmod(u, 6)
                    on = cu < 5 and (int(font[ord(text[cell]) - 0x20, v]) >> (4 - cu)) & 1
                    out[y, x] = 255 if on else colour
                    if touched is not None:
                        touched[y, x] = True
    return out.astype(np.uint8)


def draw_batch(frames, boxes, font, keep=None, count=None, ids=None, meta=None, **kw):
    """(B, H, W, 3) frames: draw_frame per frame with row b of every table."""
    return np.stack([draw_frame(frames[b], boxes[b], font, keep=None if keep is None else keep[b], count=None if count is None else count[b],
                                ids=None if ids is None else ids[b], meta=None if meta is None else meta[b], **kw)
                     for b in range(len(frames))])
