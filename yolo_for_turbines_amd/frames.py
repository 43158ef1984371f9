"""The frame front end (csrc/frames.hip): what sits between a decoder's output surface and ``model(x)``. A batch of
RGB, BGR (OpenCV) or NV12 (hardware decoders) frames becomes the letterboxed network input in ONE launch, with one pinned staging copy
for host frames, none for device frames, and no value read back: the resized sizes and paddings stay on the device as the ``meta``
table that :func:`draw_boxes` and :func:`boxes_to_frames` take. The pixels are those of :func:`letterbox` on the frame converted to
packed RGB, to the bit; parity with cv2 is unpinned for the resize and for the NV12 conversion alike (include/yolo_mi355x.h).
Nothing here computes pixels, and there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .boxes import detect_images
from .data import _resized_hw

__all__ = ["preprocess_frames", "FrameStager", "frames_to_rgb", "boxes_to_frames", "detect_frames"]

_ROW = C.sizeof(L.FrameRow)
MAX_HW = 16384                                                # the limit of yolo_frames_to_rgb (and of draw_boxes)


def _kinds(format, csc):
    if format not in L.FRAME_FORMATS:
        raise ValueError(f"format must be one of {sorted(L.FRAME_FORMATS)}, got {format!r}")
    if csc not in L.CSC_KINDS:
        raise ValueError(f"csc must be one of {sorted(L.CSC_KINDS)}, got {csc!r}")
    return L.FRAME_FORMATS[format], L.CSC_KINDS[csc]


def _geometry(format, h, w, pitch=None):
    """(rows, row bytes, pitch) of an h x w frame: NV12 has h luma rows and h / 2 rows of (U, V) pairs, w bytes each."""
    row = w if format == "nv12" else 3 * w
    return (h * 3 // 2 if format == "nv12" else h), row, (row if pitch is None else pitch)


class _Frame:
    """One parsed frame: ``t`` is a contiguous uint8 tensor whose first byte is the frame's, ``span`` the bytes the kernel may read."""
    __slots__ = ("t", "h", "w", "pitch", "span")

    def __init__(self, t, h, w, pitch, span):
        self.t, self.h, self.w, self.pitch, self.span = t, h, w, pitch, span


def _as_u8(buf, i):
    try:
        t = torch.as_tensor(buf)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"frame {i}: not an array or tensor ({type(buf).__name__})") from None
    if t.dtype != torch.uint8:
        raise ValueError(f"frame {i}: dtype must be uint8, got {t.dtype}")
    return t


def _parse_one(item, i, format):
    if isinstance(item, (tuple, list)):
        if len(item) != 4:
            raise ValueError(f"frame {i}: a pitched surface is (buffer, h, w, pitch)")
        t = _as_u8(item[0], i)
        h, w, pitch = (int(v) for v in item[1:])
        if not t.is_contiguous():
            raise ValueError(f"frame {i}: the buffer of a pitched surface must be contiguous")
    else:
        t = _as_u8(item, i)
        if format == "nv12":
            if t.dim() != 2 or t.shape[0] % 3:
                raise ValueError(f"frame {i}: an NV12 frame is (H * 3 / 2, W), got {tuple(t.shape)}")
            h, w = t.shape[0] // 3 * 2, int(t.shape[1])
        else:
            if t.dim() != 3 or t.shape[2] != 3:
                raise ValueError(f"frame {i}: an RGB / BGR frame is (H, W, 3), got {tuple(t.shape)}")
            h, w = int(t.shape[0]), int(t.shape[1])
        pitch = None
        t = t.contiguous()
    if h < 1 or w < 1:
        raise ValueError(f"frame {i}: has no pixels ({h} x {w})")
    if format == "nv12" and (h % 2 or w % 2):
        raise ValueError(f"frame {i}: NV12 needs even sizes, got {h} x {w}")
    rows, row, pitch = _geometry(format, h, w, pitch)
    if pitch < row:
        raise ValueError(f"frame {i}: pitch {pitch} is below the row size {row}")
    span = (rows - 1) * pitch + row
    if t.numel() < span:
        raise ValueError(f"frame {i}: {t.numel()} bytes, {h} x {w} with pitch {pitch} needs {span}")
    return _Frame(t, h, w, pitch, span)


def _parse(frames, format):
    """``frames`` (a list, one batch tensor or one frame) -> a list of :class:`_Frame`; every error is a ValueError that names the
    frame, raised before anything touches the device."""
    batch_dim = 3 if format == "nv12" else 4
    if isinstance(frames, tuple) and len(frames) == 4 and isinstance(frames[1], int):
        frames = [frames]                                     # one pitched surface
    elif not isinstance(frames, (list, tuple)):
        t = _as_u8(frames, 0)
        if t.dim() == batch_dim:
            if t.is_cuda and not t.is_contiguous():
                raise ValueError("frame 0: a device batch must be one contiguous tensor")
            t = t.contiguous()
            frames = [t[i] for i in range(t.shape[0])]
        elif t.dim() == batch_dim - 1:
            frames = [t]
        else:
            raise ValueError(f"frame 0: {format} frames are {batch_dim - 1}-dimensional (a batch: {batch_dim}), got {tuple(t.shape)}")
    if len(frames) == 0:
        raise ValueError("frames is empty: at least one frame is needed")
    return [_parse_one(f, i, format) for i, f in enumerate(frames)]


def _device(items, device):
    devs = {f.t.device for f in items if f.t.is_cuda}
    if len(devs) > 1:
        raise ValueError(f"frames are on different devices: {sorted(str(d) for d in devs)}")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("the frame front end runs on MI355X only (no CPU fallback)")
    if devs:
        have = next(iter(devs))
        if device is not None and dev.index is not None and dev != have:
            raise ValueError(f"frames are on different devices: {have}, and device={dev}")
        dev = have
    return dev


def _check_out(name, out, shape, dtype, dev):
    if out is None:
        return
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device.type != "cuda" \
            or (dev.index is not None and out.device != dev) or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")


def _canvas(shapes, S, rect):
    hw = (C.c_int32 * (2 * len(shapes)))(*[v for s in shapes for v in s])
    canvas = (C.c_int32 * 2)()
    L.check(L.lib().yolo_letterbox_canvas(hw, len(shapes), S, int(bool(rect)), canvas), "yolo_letterbox_canvas")
    return int(canvas[0]), int(canvas[1])


def _check_fits(shapes, S, canvas):
    """The check the kernel cannot report without a wait: every frame's resized size fits the canvas."""
    for i, (h, w) in enumerate(shapes):
        nh, nw = _resized_hw(h, w, S)
        if nh > canvas[0] or nw > canvas[1]:
            raise ValueError(f"frame {i}: {h} x {w} resizes to {nh} x {nw}, which exceeds the canvas {canvas[0]} x {canvas[1]}")


def _image_size(image_size):
    if isinstance(image_size, bool) or not isinstance(image_size, int) or image_size < 1:
        raise ValueError(f"image_size must be a positive integer, got {image_size!r}")
    return image_size


def _upload(items, dev):
    """The frames where the kernel reads them: host frames through ONE pinned buffer and one non-blocking copy (the table rides in
    front of them), device frames in place, addressed from the lowest of all. Returns (pool address, table tensor, what to keep)."""
    n = len(items)
    tab_bytes = (n * _ROW + 255) // 256 * 256
    offs, o = [None] * n, tab_bytes
    for i, f in enumerate(items):
        if not f.t.is_cuda:
            offs[i] = o
            o += (f.span + 15) // 16 * 16
    host = torch.empty(o, dtype=torch.uint8, pin_memory=True)
    for i, f in enumerate(items):
        if offs[i] is not None:
            host[offs[i]:offs[i] + f.span] = f.t.reshape(-1)[:f.span]
    dbuf = torch.empty(o, dtype=torch.uint8, device=dev)
    addr = [dbuf.data_ptr() + offs[i] if offs[i] is not None else f.t.data_ptr() for i, f in enumerate(items)]
    base = min(addr)
    rows = (L.FrameRow * n)(*[L.FrameRow(a - base, f.h, f.w, f.pitch, 0) for a, f in zip(addr, items)])
    C.memmove(host.data_ptr(), rows, n * _ROW)
    dbuf.copy_(host, non_blocking=True)
    for f in items:
        if f.t.is_cuda:
            f.t.record_stream(torch.cuda.current_stream())
    return base, dbuf, [dbuf] + [f.t for f in items]


def preprocess_frames(frames, image_size=416, format="rgb", csc="bt601", rect=False, out=None, device=None):
    """:func:`letterbox` for a batch of frames in one launch, from RGB, BGR or NV12, with nothing read back.

    ``frames``: a list of uint8 arrays or tensors of any sizes - ``(H, W, 3)`` for ``format`` "rgb" / "bgr", ``(H * 3 / 2, W)`` for
    "nv12" (the luma rows, then the rows of interleaved U, V), or ``(buffer, h, w, pitch)`` for a surface whose rows are ``pitch``
    bytes apart - or ONE tensor ``(B, H, W, 3)`` / ``(B, H * 3 / 2, W)``. Host frames go through one pinned staging buffer and one
    non-blocking copy; device frames (a contiguous batch tensor, or the tensors of a list) are read where they are. ``csc`` ("bt601",
    "bt601-full", "bt709", "bt709-full": the matrix and range of the NV12 conversion) is ignored for RGB and BGR. ``rect`` and the
    canvas rule are :func:`letterbox`'s. Returns ``(x (B, 3, Hc, Wc) fp32, meta (B, 6) int32)``, both on the device: ``x`` holds the
    bits of ``letterbox`` on the frames converted to RGB (planes in R, G, B order); ``meta`` has its tuples as rows, for
    ``draw_boxes(meta=(meta, (Hc, Wc)))`` and :func:`boxes_to_frames`. ``out``: an ``x`` to write into. Every bad argument is a
    ``ValueError`` that names the frame, raised before any launch."""
    fmt, k = _kinds(format, csc)
    S = _image_size(image_size)
    items = _parse(frames, format)
    dev = _device(items, device)
    shapes = [(f.h, f.w) for f in items]
    canvas = _canvas(shapes, S, rect)
    _check_fits(shapes, S, canvas)
    n = len(items)
    _check_out("out", out, (n, 3) + canvas, torch.float32, dev)
    with torch.cuda.device(dev):
        base, table, keep = _upload(items, dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device()))
        x = torch.empty((n, 3) + canvas, dtype=torch.float32, device=table.device) if out is None else out
        meta = torch.empty((n, 6), dtype=torch.int32, device=table.device)
        L.check(L.lib().yolo_frames_letterbox(base, table.data_ptr(), n, fmt, k, S, canvas[0], canvas[1], x.data_ptr(), meta.data_ptr(),
                                              L.current_stream()), "yolo_frames_letterbox")
    del keep
    return x, meta


def frames_to_rgb(frames, format, csc="bt601", out=None, device=None):
    """The colour conversion alone: ``frames`` (as for :func:`preprocess_frames`, all of one size) as packed RGB ``(B, H, W, 3)``
    uint8 on the device, at source resolution - what :func:`draw_boxes` draws on when the source is NV12 or BGR."""
    fmt, k = _kinds(format, csc)
    items = _parse(frames, format)
    dev = _device(items, device)
    h, w = items[0].h, items[0].w
    for i, f in enumerate(items):
        if (f.h, f.w) != (h, w):
            raise ValueError(f"frame {i}: {f.h} x {f.w}, frame 0 is {h} x {w} (frames_to_rgb takes frames of one size)")
    if h > MAX_HW or w > MAX_HW:
        raise ValueError(f"frame 0: {h} x {w} exceeds {MAX_HW} pixels a side")
    n = len(items)
    _check_out("out", out, (n, h, w, 3), torch.uint8, dev)
    with torch.cuda.device(dev):
        base, table, keep = _upload(items, dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device()))
        rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=table.device) if out is None else out
        L.check(L.lib().yolo_frames_to_rgb(base, table.data_ptr(), n, h, w, fmt, k, rgb.data_ptr(), L.current_stream()), "yolo_frames_to_rgb")
    del keep
    return rgb


def boxes_to_frames(boxes, meta, canvas_hw, out=None):
    """``unletterbox_boxes(..., meta=)`` on the device: ``boxes`` (B, N, 6) fp32 rows ``[x, y, w, h, score, cls]`` normalised to the
    ``canvas_hw = (Hc, Wc)`` canvas become rows normalised to each original frame, by the ``meta`` (B, 6) int32 device table of
    :func:`preprocess_frames`. The Python expression in fp64 on the fp32 inputs, rounded once to fp32; columns 4 and 5 are copied.
    No read-back."""
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[2] != 6:
        raise ValueError("boxes must be a float32 (B, N, 6) tensor")
    B, N = int(boxes.shape[0]), int(boxes.shape[1])
    if not isinstance(meta, torch.Tensor) or meta.dtype != torch.int32 or tuple(meta.shape) != (B, 6):
        raise ValueError(f"meta must be an int32 tensor of shape {(B, 6)}")
    try:
        ch, cw = (int(v) for v in canvas_hw)
    except (TypeError, ValueError):
        raise ValueError("canvas_hw must be (canvas_h, canvas_w)") from None
    if ch < 1 or cw < 1 or B < 1:
        raise ValueError(f"canvas_hw {(ch, cw)} must be positive, and boxes must hold at least one frame")
    dev = boxes.device
    if dev.type != "cuda":
        raise RuntimeError("boxes_to_frames runs on MI355X only (no CPU fallback)")
    if meta.device != dev:
        raise ValueError(f"meta on {meta.device}, boxes on {dev}")
    _check_out("out", out, (B, N, 6), torch.float32, dev)
    with torch.cuda.device(dev):
        bx, mt = boxes.contiguous(), meta.contiguous()
        res = torch.empty_like(bx) if out is None else out
        L.check(L.lib().yolo_boxes_to_frames(bx.data_ptr(), B, N, mt.data_ptr(), ch, cw, res.data_ptr(), L.current_stream()),
                "yolo_boxes_to_frames")
    return res


def detect_frames(model, frames, scaled_anchors, image_size=416, format="rgb", csc="bt601", rect=False, iou_threshold=0.45,
                  obj_threshold=0.5, nms=None, device=None):
    """From frames to boxes on the frames: :func:`preprocess_frames`, :func:`detect_images` (centre-format boxes) and
    :func:`boxes_to_frames` on its boxes. Returns ``(boxes, keep, count, meta)``: ``boxes`` (B, N, 6) normalised to each ORIGINAL
    frame, ``keep`` / ``count`` as :func:`detect` returns them. One host synchronisation, that of ``detect_images``."""
    x, meta = preprocess_frames(frames, image_size, format, csc, rect, device=device)
    boxes, keep, count = detect_images(model, x, scaled_anchors, iou_threshold, obj_threshold, "center", nms=nms)
    return boxes_to_frames(boxes, meta, x.shape[2:]), keep, count, meta


class FrameStager:
    """The front end of a video loop: ``n`` frames of ``h x w`` per call, all buffers made once.

    It owns two pinned staging buffers, the device pool, the frame table, ``x`` and ``meta``. ``stage(frames)`` returns ``(x, meta)``
    - the same storage on every call - without allocating. A contiguous device tensor ``(n, H, W, 3)`` / ``(n, H * 3 / 2, W)`` is read
    where it is: one launch on the current stream, which a ``torch.cuda.graph`` captures (the replay reads the tensor's address, so
    new frames go into the same tensor). Host frames (a list, or one array) are copied into a pinned buffer and from there with one
    non-blocking copy; the two pinned buffers alternate, so the host waits only if the copy issued two calls earlier has not
    finished. A list of device tensors is gathered into the pool by device copies."""

    def __init__(self, n, h, w, format, image_size, rect=False, csc="bt601", device=None):
        self.format, self.csc = format, csc
        self._fmt, self._k = _kinds(format, csc)
        self.image_size = _image_size(image_size)
        n, h, w = int(n), int(h), int(w)
        if n < 1 or h < 1 or w < 1:
            raise ValueError(f"FrameStager needs at least one frame with pixels, got {n} x ({h} x {w})")
        if format == "nv12" and (h % 2 or w % 2):
            raise ValueError(f"frame 0: NV12 needs even sizes, got {h} x {w}")
        self.n, self.h, self.w = n, h, w
        rows, row, _ = _geometry(format, h, w)
        self._frame_shape = (rows, w) if format == "nv12" else (h, w, 3)
        self._frame_bytes = rows * row
        self.canvas = _canvas([(h, w)], self.image_size, rect)
        _check_fits([(h, w)], self.image_size, self.canvas)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("the frame front end runs on MI355X only (no CPU fallback)")
        with torch.cuda.device(dev):
            self.device = torch.device("cuda", torch.cuda.current_device())
            self._pinned = [torch.empty(n * self._frame_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._copied = [None, None]                       # the event behind each pinned buffer's last copy
            self._events = [torch.cuda.Event(), torch.cuda.Event()]
            self._slot = 0
            self._pool = torch.empty(n * self._frame_bytes, dtype=torch.uint8, device=self.device)
            rows_c = (L.FrameRow * n)(*[L.FrameRow(i * self._frame_bytes, h, w, row, 0) for i in range(n)])
            tab = torch.empty(n * _ROW, dtype=torch.uint8)
            C.memmove(tab.data_ptr(), rows_c, n * _ROW)
            self._table = tab.to(self.device)                # a tight batch anywhere has this table: offsets from its first byte
            self.x = torch.empty((n, 3) + self.canvas, dtype=torch.float32, device=self.device)
            self.meta = torch.empty((n, 6), dtype=torch.int32, device=self.device)

    def _batch(self, t, i=0):
        want = (self.n,) + self._frame_shape
        if t.dtype != torch.uint8:
            raise ValueError(f"frame {i}: dtype must be uint8, got {t.dtype}")
        if tuple(t.shape) != want:
            raise ValueError(f"frame {i}: this stager takes {self.format} batches of shape {want}, got {tuple(t.shape)}")
        return t

    def stage(self, frames):
        """``frames`` -> ``(x, meta)``, the stager's own tensors; see the class."""
        with torch.cuda.device(self.device):
            if isinstance(frames, torch.Tensor) and frames.is_cuda:
                self._batch(frames)
                if frames.device != self.device:
                    raise ValueError(f"frames are on different devices: {frames.device}, the stager is on {self.device}")
                if not frames.is_contiguous():
                    raise ValueError("a device batch must be one contiguous tensor")
                base = frames.data_ptr()
            else:
                if not isinstance(frames, (list, tuple)):
                    frames = self._batch(torch.as_tensor(frames))
                elif len(frames) != self.n:
                    raise ValueError(f"this stager takes {self.n} frames, got {len(frames)}")
                ts = []
                for i, f in enumerate(frames):
                    t = _as_u8(f, i)
                    if tuple(t.shape) != self._frame_shape:
                        raise ValueError(f"frame {i}: this stager takes {self.format} frames of shape {self._frame_shape}, got {tuple(t.shape)}")
                    ts.append(t)
                fb = self._frame_bytes
                if any(t.is_cuda for t in ts):
                    for i, t in enumerate(ts):
                        self._pool[i * fb:(i + 1) * fb].view(self._frame_shape).copy_(t, non_blocking=True)
                else:
                    s = self._slot
                    self._slot = 1 - s
                    if self._copied[s] is not None:
                        self._copied[s].synchronize()
                    pin = self._pinned[s]
                    for i, t in enumerate(ts):
                        pin[i * fb:(i + 1) * fb].view(self._frame_shape).copy_(t)
                    self._pool.copy_(pin, non_blocking=True)
                    self._events[s].record()
                    self._copied[s] = self._events[s]
                base = self._pool.data_ptr()
            L.check(L.lib().yolo_frames_letterbox(base, self._table.data_ptr(), self.n, self._fmt, self._k, self.image_size, self.canvas[0],
                                                  self.canvas[1], self.x.data_ptr(), self.meta.data_ptr(), L.current_stream()),
                    "yolo_frames_letterbox")
        return self.x, self.meta
