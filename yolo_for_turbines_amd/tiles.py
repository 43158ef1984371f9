"""Tiled detection of frames larger than the network input (csrc/tiles.hip): the tile grid, the pyramid and ``detect_tiled``."""
import ctypes as C
import math

import torch

from . import _lib as L
from .boxes import _anchors_to_device, _decode3, _grid_hw, _nms_options, _soft_nms, _workspace, nms_indices


def _tile_hw(tile):
    th, tw = _grid_hw(tile)
    if th <= 0 or tw <= 0 or th % 32 or tw % 32:
        raise ValueError(f"tile sides must be positive multiples of 32, got {th} x {tw}")
    return th, tw


def _overlap_px(overlap, th, tw):
    """fraction | pixels | (per axis) -> (oh, ow) pixels: an int is a pixel count, anything else a fraction of the tile side."""
    oh, ow = overlap if isinstance(overlap, (tuple, list)) else (overlap, overlap)

    def px(o, t):
        return int(o) if isinstance(o, int) and not isinstance(o, bool) else int(round(float(o) * t))
    oh, ow = px(oh, th), px(ow, tw)
    if not (0 <= oh < th and 0 <= ow < tw):
        raise ValueError(f"overlap must satisfy 0 <= overlap < tile, got {oh} of {th}, {ow} of {tw} pixels")
    return oh, ow


def _tile_origins(h, w, th, tw, oh, ow):
    """yolo_tile_grid: the flat [y0, x0, y0, x0, ...] list of one image's tiles in row-major order."""
    lib = L.lib()
    n = lib.yolo_tile_grid(h, w, th, tw, oh, ow, None, 0)
    L.check(min(n, 0), "yolo_tile_grid")
    buf = (C.c_int32 * (2 * n))()
    L.check(min(lib.yolo_tile_grid(h, w, th, tw, oh, ow, buf, n), 0), "yolo_tile_grid")
    return list(buf)


def tile_grid(h, w, tile=416, overlap=0.2):
    """Origins of the overlapping tiles an h x w image is cut into, an int32 (T, 2) tensor of [y0, x0] rows in row-major tile
    order (``yolo_tile_grid``). ``tile``: t or (th, tw), any size. ``overlap``: a fraction of the tile side (``int(round(overlap *
    t))`` pixels per axis), or pixels when given as int(s); a pair is (rows, columns). Per axis the stride is t - overlap; an axis
    that is no longer than the tile has one tile at 0 (zero-padded), otherwise the last tile is flush with the edge."""
    th, tw = _grid_hw(tile)
    oh, ow = _overlap_px(overlap, th, tw)
    return torch.tensor(_tile_origins(int(h), int(w), th, tw, oh, ow), dtype=torch.int32).reshape(-1, 2)


def _scales(scales, top=8, distinct=True):
    """A non-empty sequence of finite floats in (0, top], no two equal when ``distinct`` -> list of float."""
    try:
        if isinstance(scales, (str, bytes)) or any(isinstance(v, (bool, str, bytes)) for v in scales):
            raise TypeError
        out = [float(v) for v in scales]
    except (TypeError, ValueError):
        raise ValueError(f"scales must be a non-empty sequence of numbers, got {scales!r}") from None
    if not out or not all(math.isfinite(v) and 0.0 < v <= top for v in out):
        raise ValueError(f"scales must be a non-empty sequence of finite numbers in (0, {top}], got {scales!r}")
    if distinct and len(set(out)) != len(out):
        raise ValueError(f"scales must not repeat a level, got {scales!r}")
    return out


def _level_hw(h, w, scale):
    """yolo_tile_level_hw: (max(1, rint(h scale)), max(1, rint(w scale))), half to even."""
    lh, lw = C.c_int(), C.c_int()
    L.check(L.lib().yolo_tile_level_hw(int(h), int(w), float(scale), C.byref(lh), C.byref(lw)), "yolo_tile_level_hw")
    return lh.value, lw.value


def tile_pyramid(h, w, tile=416, overlap=0.2, scales=(1.0,)):
    """The levels :func:`detect_tiled` cuts an h x w image into: a list with one ``((lh, lw), origins)`` entry per scale, in the
    order given. ``(lh, lw)`` is the size of the image resized by that scale (``yolo_tile_level_hw``: ``max(1, rint(h * scale))``,
    half to even; scale 1.0 is the image itself) and ``origins`` is ``tile_grid(lh, lw, tile, overlap)``, in pixels of the level.
    ``scales``: distinct finite numbers in (0, 8]."""
    out = []
    for sc in _scales(scales):
        lh, lw = _level_hw(h, w, sc)
        out.append(((lh, lw), tile_grid(lh, lw, tile, overlap)))
    return out


def detect_tiled(model, images, scaled_anchors, tile=416, overlap=0.2, iou_threshold=0.45, obj_threshold=0.5, box_format="center",
                 batch=32, max_candidates=65536, scales=(1.0,), edge_margin=None, nms=None):
    """Detection on frames that are larger than the network input: every frame is cut into overlapping tiles
    (:func:`tile_grid`), the tiles of all frames run through ``model(x)`` in chunks of ``batch``, the decoded boxes
    above ``obj_threshold`` are mapped back to their frame and compacted on the device (``yolo_tile_collect``), and one
    per-class NMS per frame merges the duplicates along the seams. ``images``: one uint8 (H, W, 3) tensor / array or a list of
    them (any sizes; on the host or already on the device). ``scaled_anchors``: for the TILE size, as for
    :func:`detect_images` (``scaled_anchors(anchors, th, tw)``), whatever the level.

    ``scales``: the pyramid (:func:`tile_pyramid`), distinct finite numbers in (0, 8]. Every frame is tiled once per scale, on
    the frame resized by it (``max(1, rint(side * scale))`` per side, half to even; the library's one uint8 INTER_LINEAR, sampled
    by the gather, no resized frame is stored; a scale below 0.5 skips source pixels as :func:`letterbox` does), so an object
    that no native tile sees whole is seen whole by a coarser level; the levels meet in the one NMS. The default ``(1.0,)`` is
    native resolution only. A level that is no larger than the tile is a single zero-padded tile: with tile 416 a 5472 x 3648
    frame is one at scale 416 / 5472 = 0.076 or below, and ``(1.0, 0.5, 0.25)`` ends at 1368 x 912, 4 x 3 tiles (187 + 48 + 12 tiles per frame).
    ``edge_margin``: ``None`` (off) or pixels of the tile, >= 0. On, a box that reaches within ``edge_margin`` of a side of its
    tile is dropped before the NMS when that side is interior, i.e. not on the level's border (``yolo_tile_collect_ex``): it is
    the truncated copy of an object that a neighbouring tile or a coarser level reports whole, and its IoU with the whole box
    is too low for the NMS to remove it. An object is lost if every tile of every level cuts it, so use it with an overlap
    larger than the objects of the finest level or with a coarser level.
    ``nms``: ``None`` (the hard NMS) or an :class:`NMSOptions` / a dict of its fields: the frame's candidates go through
    :func:`soft_nms` instead, and column 4 of the kept rows of ``boxes`` holds the rescored objectness. The Gaussian decay has no
    threshold: a truncated copy along a seam loses score in proportion to its overlap with the whole box.

    Returns ``(boxes (F, max_candidates, 6), keep (F, max_candidates) int32, count (F,) int32, candidates (F,) int32)``:
    ``boxes[f, :candidates[f]]`` are frame f's candidates ``[cx, cy, w, h, obj, cls]`` normalised to that frame, in (level, tile,
    row) order with the levels in the order of ``scales`` (the order :func:`nms_indices` breaks score ties by), zero rows behind
    them; ``keep`` / ``count`` index them as from :func:`nms_indices`. ``max_candidates`` counts a frame's candidates over all its
    levels. The tiles are in (frame, level, tile) order and a chunk runs across levels and frames. Everything is stream-ordered
    with ONE host synchronisation, which reads ``candidates`` and the forwards' NaN flags together; the forward's exceptions are
    raised as by :func:`detect_images`, and a frame with more than ``max_candidates`` candidates raises ``ValueError``.
    A last chunk shorter than ``batch`` runs at its own size (a second plan of the model, at most two per call).
    ``fuse_boxes(boxes, ..., class_agnostic=...)`` on the returned candidates is the fusing (weighted box fusion instead of the
    NMS's one winner per object) and the class-agnostic merge.
    Not built: area-filtered downscaling; merging the two halves of a box across a seam."""
    th, tw = _tile_hw(tile)
    oh, ow = _overlap_px(overlap, th, tw)
    if not float(obj_threshold) >= 0:
        raise ValueError(f"obj_threshold must be >= 0 (the zero rows behind the candidates must not pass it), got {obj_threshold}")
    opts = None if nms is None else _nms_options(nms, obj_threshold)
    batch, cap = int(batch), int(max_candidates)
    if batch < 1 or cap < 1:
        raise ValueError(f"batch and max_candidates must be >= 1, got {batch} and {cap}")
    scales = _scales(scales)
    if edge_margin is not None:
        try:
            margin = float(edge_margin)
        except (TypeError, ValueError):
            margin = math.nan
        if isinstance(edge_margin, bool) or not (math.isfinite(margin) and margin >= 0):
            raise ValueError(f"edge_margin must be None or a finite number >= 0 (pixels of the tile), got {edge_margin!r}")
    plain = scales == [1.0] and edge_margin is None             # today's launches: yolo_tile_gather, yolo_tile_collect
    if isinstance(images, torch.Tensor) and images.dim() == 3 or not isinstance(images, (list, tuple)):
        images = [images]
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
            raise ValueError("images must be uint8 (H, W, 3)")
        ts.append(t)
    if not ts:
        raise ValueError("detect_tiled needs at least one image")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("detect_tiled runs on MI355X only (no CPU fallback)")
    F = len(ts)
    lib = L.lib()
    # host tables: per tile [y0, x0] (gather) and {image, y0, x0, level} (collect), per image [H, W], per level [H, W].
    # A level is one (frame, scale) pair, numbered f * len(scales) + k; runs[r] = (first tile, frame, level H, level W).
    origins, tiles, runs, lev = [], [], [], []
    for f, t in enumerate(ts):
        for sc in scales:
            lh, lw = _level_hw(t.shape[0], t.shape[1], sc)
            o = _tile_origins(lh, lw, th, tw, oh, ow)
            runs.append((len(origins) // 2, f, lh, lw))
            origins += o
            for k in range(0, len(o), 2):
                tiles += [f, o[k], o[k + 1], 0 if plain else len(lev) // 2]   # yolo_tile_collect's spare field stays 0
            lev += [lh, lw]
    T = len(origins) // 2
    runs.append((T, F, 0, 0))
    hw = [int(v) for t in ts for v in t.shape[:2]]
    if plain:
        lev = []
    host = torch.empty(6 * T + 2 * F + len(lev), dtype=torch.int32, pin_memory=True)
    host.copy_(torch.tensor(origins + tiles + hw + lev, dtype=torch.int32))
    anc = [torch.as_tensor(a, dtype=torch.float32).reshape(3, 2) for a in scaled_anchors]
    chunks = [(s, min(batch, T - s)) for s in range(0, T, batch)]
    eng = model._engine
    with torch.cuda.device(dev):
        stream = L.current_stream()
        tab = host.to(dev, non_blocking=True)
        d_origins, d_tiles, d_hw, d_lev = tab[:2 * T], tab[2 * T:6 * T], tab[6 * T:6 * T + 2 * F], tab[6 * T + 2 * F:]
        if any(a.device != dev for a in anc):
            anc = _anchors_to_device(torch.cat([a.cpu().reshape(-1) for a in anc]), dev, (3, 3, 2))
        anc = [a.contiguous() for a in anc]
        frames = []
        for t in ts:
            if t.device.type != "cuda":
                staged = torch.empty(t.numel(), dtype=torch.uint8, pin_memory=True)
                staged.copy_(t.reshape(-1))
                t = staged.to(dev, non_blocking=True)
            frames.append(t.to(dev).contiguous())
        cand = torch.empty((F, cap, 6), dtype=torch.float32, device=dev)
        tail = torch.empty(F + len(chunks), dtype=torch.int32, device=dev)       # candidates per image | NaN flag per chunk
        L.check(lib.yolo_fill_zero(cand.data_ptr(), cand.numel() * 4, stream), "yolo_fill_zero")
        L.check(lib.yolo_fill_zero(tail.data_ptr(), tail.numel() * 4, stream), "yolo_fill_zero")
        x = torch.empty((min(batch, T), 3, th, tw), dtype=torch.float32, device=dev)
        boxes = ws = None
        with eng.deferred_nan():
            for c, (s, n) in enumerate(chunks):
                r = max(k for k in range(len(runs) - 1) if runs[k][0] <= s)
                while runs[r][0] < s + n:                           # one gather per (frame, level) that has tiles in this chunk
                    a, b = max(runs[r][0], s), min(runs[r + 1][0], s + n)
                    f, lh, lw = runs[r][1:]
                    if b > a and (lh, lw) == (hw[2 * f], hw[2 * f + 1]):
                        L.check(lib.yolo_tile_gather(frames[f].data_ptr(), hw[2 * f], hw[2 * f + 1], d_origins.data_ptr() + 8 * a, b - a,
                                                     th, tw, x.data_ptr() + 4 * (a - s) * 3 * th * tw, stream), "yolo_tile_gather")
                    elif b > a:
                        L.check(lib.yolo_tile_gather_scaled(frames[f].data_ptr(), hw[2 * f], hw[2 * f + 1], lh, lw,
                                                            d_origins.data_ptr() + 8 * a, b - a, th, tw,
                                                            x.data_ptr() + 4 * (a - s) * 3 * th * tw, stream), "yolo_tile_gather_scaled")
                    r += 1
                with torch.no_grad():
                    preds = model(x[:n])
                eng.keep_pending_flag(tail.data_ptr(), F + c, stream)
                n_per = sum(3 * p.shape[2] * p.shape[3] for p in preds)
                if boxes is None:
                    boxes = torch.empty((x.shape[0], n_per, 6), dtype=torch.float32, device=dev)
                    ws = _workspace(max(int(lib.yolo_tile_collect_workspace_bytes(x.shape[0], n_per)), 256), dev)
                _decode3(preds, anc, n, boxes, n_per, stream=stream)
                if plain:
                    L.check(lib.yolo_tile_collect(boxes.data_ptr(), n, n_per, d_tiles.data_ptr() + 16 * s, d_hw.data_ptr(), F, th, tw,
                                                  float(obj_threshold), cand.data_ptr(), cap, tail.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  stream), "yolo_tile_collect")
                else:
                    L.check(lib.yolo_tile_collect_ex(boxes.data_ptr(), n, n_per, d_tiles.data_ptr() + 16 * s, d_lev.data_ptr(),
                                                     len(lev) // 2, F, th, tw, float(obj_threshold),
                                                     -1.0 if edge_margin is None else margin, cand.data_ptr(), cap,
                                                     tail.data_ptr(), ws.data_ptr(), ws.numel(), stream), "yolo_tile_collect_ex")
        for t in frames:
            t.record_stream(torch.cuda.current_stream())
        if opts is not None:
            keep, count, _ = _soft_nms(cand, iou_threshold, obj_threshold, box_format, opts, cand)
        else:
            keep, count = nms_indices(cand, iou_threshold, obj_threshold, box_format)
        tail_host = tail.tolist()                                   # the one host synchronisation
    eng.raise_on_flags(tail_host[F:])
    for f in range(F):
        if tail_host[f] > cap:
            raise ValueError(f"image {f} has {tail_host[f]} candidates above obj_threshold {obj_threshold}, max_candidates is {cap}")
    return cand, keep, count, tail[:F]
