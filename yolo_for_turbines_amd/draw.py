"""Drawing detections and tracks onto frames on the device (``yolo_draw_boxes``, csrc/draw.hip): class-coloured rectangles with a
filled label plate and white text per box, the picture ``plot_original`` / ``plot_image_with_boxes`` of the reference end in
(utils.py:418-501), for batches of frames that stay in HBM. The geometry, the blend, the font and the order are defined to the bit
in include/yolo_mi355x.h and DESIGN.md 7.25; nothing here computes pixels."""
from __future__ import annotations

import torch

from . import _lib as L
from .data import unletterbox_boxes

__all__ = ["draw_boxes", "draw_tracks", "plot_image_with_boxes", "plot_original", "default_palette", "TAB20B"]

MAX_THICKNESS, MAX_FONT_SCALE, MAX_HW = 64, 8, 16384          # the limits of yolo_draw_boxes
# matplotlib's tab20b, each channel int(v * 255 + 0.5)
TAB20B = ((57, 59, 121), (82, 84, 163), (107, 110, 207), (156, 158, 222), (99, 121, 57), (140, 162, 82), (181, 207, 107), (206, 219, 156),
          (140, 109, 49), (189, 158, 57), (231, 186, 82), (231, 203, 148), (132, 60, 57), (173, 73, 74), (214, 97, 107), (231, 150, 156),
          (123, 65, 115), (165, 81, 148), (206, 109, 189), (222, 158, 214))

_name_tables, _palettes = {}, {}                              # device copies, kept: a captured call keeps their addresses


def default_palette(n_classes=None):
    """The colours of the reference (utils.py:427-428): ``tab20b`` sampled at ``np.linspace(0, 1, n)``, that is for class c of n > 1
    the entry ``min(19, int(c / (n - 1) * 20))``; without ``n_classes`` the 20 colours themselves. A tuple of (r, g, b)."""
    if n_classes is None:
        return TAB20B
    n = int(n_classes)
    return tuple(TAB20B[min(19, int(c / (n - 1) * 20)) if n > 1 else 0] for c in range(n))


def default_style(h, w):
    """(thickness, font_scale) in the reference's proportions (utils.py:451,458), inside the kernel's bounds."""
    m = max(int(h), int(w))
    return min(MAX_THICKNESS, max(1, int(0.003 * m))), min(MAX_FONT_SCALE, max(1, int(0.01 * m) // 8))


def _int_in(name, v, top):
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
        raise ValueError(f"{name} must be an integer in [1, {top}], got {v!r}")
    return v


def _alpha(name, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in [0, 1], got {v!r}") from None
    if isinstance(v, bool) or not 0.0 <= f <= 1.0:
        raise ValueError(f"{name} must be a number in [0, 1], got {v!r}")
    return int(f * 255 + 0.5)


def _names(class_names):
    if class_names is None:
        return None
    if isinstance(class_names, (str, bytes)) or not hasattr(class_names, "__len__") or len(class_names) == 0 \
            or not all(isinstance(s, str) for s in class_names):
        raise ValueError(f"class_names must be a non-empty sequence of strings, got {class_names!r}")
    return tuple(class_names)


def _palette_rows(palette):
    """A host palette as a tuple of (r, g, b) ints; a CUDA uint8 (K, 3) tensor is passed through."""
    if isinstance(palette, torch.Tensor):
        if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] < 1:
            raise ValueError("palette must be a uint8 (K, 3) table with K >= 1")
        if palette.is_cuda:
            return palette.contiguous()
        palette = palette.tolist()
    try:
        rows = tuple(tuple(int(c) for c in row) for row in palette)
    except (TypeError, ValueError):
        raise ValueError("palette must be a uint8 (K, 3) table with K >= 1") from None
    if len(rows) < 1 or any(len(r) != 3 or not all(0 <= c <= 255 for c in r) for r in rows):
        raise ValueError("palette must be a uint8 (K, 3) table with K >= 1")
    return rows


def _device_names(names, dev):
    key = (names, str(dev))
    if key not in _name_tables:
        enc = [s.encode("ascii", "replace") for s in names]
        width = (max(1, max(len(e) for e in enc)) + 3) // 4 * 4
        host = torch.tensor([list(e.ljust(width, b"\0")) for e in enc], dtype=torch.uint8)
        _name_tables[key] = (host.to(dev), width)
    return _name_tables[key]


def _device_palette(rows, dev):
    if isinstance(rows, torch.Tensor):
        return rows
    key = (rows, str(dev))
    if key not in _palettes:
        _palettes[key] = torch.tensor(rows, dtype=torch.uint8).to(dev)
    return _palettes[key]


def draw_boxes(frames, boxes, keep=None, count=None, *, ids=None, class_names=None, box_format="center", meta=None, thickness=None,
               font_scale=None, fill_alpha=0.0, line_alpha=1.0, labels=True, scores=True, palette=None, color_by="class", inplace=False):
    """Draw the selected rows of ``boxes`` onto ``frames`` and return the drawn frames; one device call, no host synchronisation.

    ``frames``: uint8 CUDA (B, H, W, 3) or (H, W, 3) (then ``boxes`` may be (N, 6)), or a list of B (H, W, 3) tensors of any sizes
    (one call per frame, a list is returned). ``boxes``: (B, N, 6) rows [x, y, w, h, score, cls] normalised to the frame, or corners
    [x0, y0, x1, y1, score, cls] with ``box_format="corners"``. Selection as for :meth:`Tracker.update`: ``keep`` + ``count`` (the
    output of :func:`detect`), ``count`` alone (:func:`fuse_boxes`, a :class:`TrackResult`), or every row. ``ids``: int (B, N), per
    row; an id > 0 is printed as ``#id`` and, with ``color_by="id"``, picks the colour. ``class_names``: the label text and, unless
    ``palette`` (a (K, 3) uint8 table, indexed ``class mod K`` or ``id mod K``) is given, the reference's colour per class; a row
    whose class is outside the names draws nothing. ``meta = (table, (canvas_h, canvas_w))``: the boxes are normalised to a
    letterboxed canvas and ``table`` is what :func:`letterbox` returned for the frames (a list of tuples, or an int32 CUDA (B, 6)
    tensor): they are mapped back as by ``unletterbox_boxes(..., meta=)``. ``thickness``, ``font_scale``: pixels; by default the
    reference's proportions ``max(1, int(0.003 max(H, W)))`` and ``max(1, int(0.01 max(H, W)) // 8)``. ``line_alpha``,
    ``fill_alpha`` in [0, 1]: opacity of the outline and of the box's interior. ``scores``: append the score in percent.
    ``inplace``: draw into ``frames`` (which must be contiguous) instead of a copy. There is no CPU fallback."""
    if isinstance(frames, (list, tuple)):
        if len(frames) == 0 or not all(isinstance(f, torch.Tensor) and f.dim() == 3 for f in frames):
            raise ValueError("a list of frames must hold uint8 (H, W, 3) tensors")
        if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[0] != len(frames):
            raise ValueError(f"boxes must be a floating-point ({len(frames)}, N, 6) tensor for a list of {len(frames)} frames")
        one = lambda t, i: t[i:i + 1] if isinstance(t, torch.Tensor) else t
        if meta is not None and (not isinstance(meta, (tuple, list)) or len(meta) != 2 or isinstance(meta[0], torch.Tensor)
                                 or len(meta[0]) != len(frames)):
            raise ValueError("meta of a list of frames must be (the letterbox's list of tuples, (canvas_h, canvas_w))")
        return [draw_boxes(f, boxes[i:i + 1], one(keep, i), one(count, i),
                           ids=one(ids, i), class_names=class_names, box_format=box_format,
                           meta=None if meta is None else ([meta[0][i]], meta[1]), thickness=thickness, font_scale=font_scale,
                           fill_alpha=fill_alpha, line_alpha=line_alpha, labels=labels, scores=scores, palette=palette, color_by=color_by,
                           inplace=inplace) for i, f in enumerate(frames)]
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError("frames must be a uint8 (B, H, W, 3) or (H, W, 3) tensor")
    single = frames.dim() == 3
    if not isinstance(boxes, torch.Tensor) or not boxes.is_floating_point() or boxes.shape[-1:] != (6,) \
            or boxes.dim() not in ((2, 3) if single else (3,)):
        raise ValueError("boxes must be a floating-point (B, N, 6) tensor")
    fr = frames[None] if single else frames
    bx = boxes[None] if boxes.dim() == 2 else boxes
    B, H, W, _ = fr.shape
    N = bx.shape[1]
    if bx.shape[0] != B:
        raise ValueError(f"boxes of {bx.shape[0]} frames, {B} frames")
    if not 1 <= H <= MAX_HW or not 1 <= W <= MAX_HW or B < 1:
        raise ValueError(f"frames must be at least one frame of 1 .. {MAX_HW} pixels a side, got {tuple(fr.shape)}")
    if keep is not None and count is None:
        raise ValueError("keep needs count")
    for name, t, shape in (("keep", keep, (B, max(N, 1))), ("count", count, (B,)), ("ids", ids, (B, N))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.is_floating_point() or t.dtype == torch.bool or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be an integer tensor of shape {shape}")
    if box_format not in ("center", "corners"):
        raise ValueError(f"box_format must be 'center' or 'corners', got {box_format!r}")
    if color_by not in ("class", "id"):
        raise ValueError(f"color_by must be 'class' or 'id', got {color_by!r}")
    if color_by == "id" and ids is None:
        raise ValueError("color_by='id' needs ids")
    d_thick, d_scale = default_style(H, W)
    thickness = d_thick if thickness is None else _int_in("thickness", thickness, MAX_THICKNESS)
    font_scale = d_scale if font_scale is None else _int_in("font_scale", font_scale, MAX_FONT_SCALE)
    la, fa = _alpha("line_alpha", line_alpha), _alpha("fill_alpha", fill_alpha)
    names = _names(class_names)
    if palette is not None:
        pal = _palette_rows(palette)
    else:
        pal = default_palette(len(names) if names is not None and color_by == "class" else None)
    table = canvas = None
    if meta is not None:
        try:
            table, (ch, cw) = meta
            canvas = (int(ch), int(cw))
        except (TypeError, ValueError):
            raise ValueError("meta must be (table, (canvas_h, canvas_w))") from None
        if canvas[0] < 1 or canvas[1] < 1:
            raise ValueError(f"meta: canvas size {canvas} must be positive")
        if isinstance(table, torch.Tensor):
            if table.dtype != torch.int32 or tuple(table.shape) != (B, 6):
                raise ValueError(f"meta: the table must be an int32 tensor of shape {(B, 6)}")
        else:
            try:
                rows = [[int(v) for v in r] for r in table]
            except (TypeError, ValueError):
                raise ValueError(f"meta: the table must hold {B} tuples of 6 integers") from None
            if len(rows) != B or any(len(r) != 6 for r in rows):
                raise ValueError(f"meta: the table must hold {B} tuples of 6 integers")
            table = torch.tensor(rows, dtype=torch.int32)
    if inplace and not fr.is_contiguous():
        raise ValueError("inplace needs contiguous frames")

    dev = fr.device
    on_dev = [fr, bx] + [t for t in (keep, count, ids, pal if isinstance(pal, torch.Tensor) else None) if t is not None]
    if dev.type != "cuda" or any(t.device != dev for t in on_dev):
        raise RuntimeError("draw_boxes runs on MI355X only (no CPU fallback): frames, boxes, keep, count, ids and a tensor palette "
                           "must be on one CUDA device")
    if isinstance(table, torch.Tensor) and table.is_cuda and table.device != dev:
        raise RuntimeError(f"meta on {table.device}, frames on {dev}")
    lib = L.lib()
    src = fr.contiguous()
    bx = bx.float().contiguous()
    keep = None if keep is None or N == 0 else keep.to(torch.int32).contiguous()
    count = None if count is None else count.to(torch.int32).contiguous()
    ids = None if ids is None or N == 0 else ids.to(torch.int32).contiguous()
    params = L.DrawParams(thickness, font_scale, la, fa, int(bool(labels)), int(bool(scores)), int(color_by == "id" and ids is not None), 0)
    with torch.cuda.device(dev):
        name_t, width = _device_names(names, dev) if names is not None else (None, 0)
        pal_t = _device_palette(pal, dev)
        table = None if table is None else table.to(dev).contiguous()
        out = src if inplace else torch.empty_like(src)
        nbytes = lib.yolo_draw_workspace_bytes(B, N)
        if nbytes == 0:
            raise ValueError(f"draw_boxes takes at most 65,535 frames of 16,777,216 boxes, got {B} x {N}")
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        chw = (L.C.c_int32 * 2)(*(canvas or (0, 0)))
        L.check(lib.yolo_draw_boxes(src.data_ptr(), out.data_ptr(), B, H, W, bx.data_ptr(), N, int(box_format == "center"), L.ptr(keep),
                                    L.ptr(count), L.ptr(ids), L.ptr(table), chw if table is not None else None, L.C.byref(params),
                                    L.ptr(name_t), len(names) if names is not None else 0, width, pal_t.data_ptr(), pal_t.shape[0],
                                    ws.data_ptr(), ws.numel(), L.current_stream()), "yolo_draw_boxes")
    return out[0] if single else out


def draw_tracks(frames, result, class_names=None, **style):
    """Draw a :class:`TrackResult` (one frame per stream): its confirmed tracks, coloured by track id and labelled
    ``name #id score``. ``style``: the keyword arguments of :func:`draw_boxes`."""
    if not all(hasattr(result, f) for f in ("boxes", "ids", "count")):
        raise ValueError("result must be a TrackResult")
    style.setdefault("color_by", "id")
    return draw_boxes(frames, result.boxes, count=result.count, ids=result.ids, class_names=class_names, **style)


def plot_image_with_boxes(image, boxes, class_list, image_name="example", savefig=False):
    """``plot_image_with_boxes`` of the reference (utils.py:418-473) with one device draw: ``image`` (H, W, 3) uint8 array,
    ``boxes`` a list of [x, y, w, h, obj, class_label] normalised to the image, ``class_list`` the names. An empty list prints
    "No objects detected." and returns the image unchanged, as the reference does. Deviations: the result is a uint8 (H, W, 3)
    numpy array, not a PIL image, and no figure is shown; it has the reference's geometry (rectangle centred on the box edge,
    line width and text size in its proportions, a filled plate with white text on the box's top-left corner) and colours, but a
    built-in 5 x 7 font and no anti-aliasing, so it is not pixel-equal to matplotlib; ``savefig`` writes ``{image_name}.png`` only
    if PIL imports."""
    import numpy as np
    if len(boxes) == 0:
        print("No objects detected.")
        return image
    arr = np.ascontiguousarray(np.asarray(image))
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError("image must be uint8 (H, W, 3)")
    rows = torch.tensor([[float(v) for v in b] for b in boxes], dtype=torch.float64)
    if rows.dim() != 2 or rows.shape[1] != 6:
        raise ValueError("boxes must be a list of [x, y, w, h, obj, class_label]")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = draw_boxes(torch.from_numpy(arr).to(dev), rows.float().to(dev), class_names=list(class_list), scores=False)
    res = out.cpu().numpy()
    if savefig:
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None:
            Image.fromarray(res).save(f"{image_name}.png")
    return res


def plot_original(original_image, resized_image, boxes, class_list):
    """``plot_original`` of the reference (utils.py:475-501): ``boxes`` normalised to the letterboxed ``resized_image`` are mapped to
    ``original_image`` by :func:`unletterbox_boxes` (the reference's arithmetic, on the host) and drawn on it by
    :func:`plot_image_with_boxes`, whose deviations apply."""
    o_h, o_w, _ = original_image.shape
    r_h, r_w, _ = resized_image.shape
    return plot_image_with_boxes(original_image, unletterbox_boxes(boxes, (o_h, o_w), (r_h, r_w)), class_list)
