"""Training on tiles (csrc/crops.hip): the training-side counterpart of :func:`detect_tiled`. A pool of full-size
images is uploaded ONCE and stays on the device; every training batch is then cut from it - box-aware windows at a drawn scale, boxes
remapped and filtered by visibility, the augmentation chain of :func:`augment_batch` and the target builder behind them - with fresh
windows every step, no image crossing the bus again and no value read back. The reference tiled its dataset offline instead, which
fixes tile size, overlap and scale once and gives every epoch the same cuts. The contract of the windows, boxes and pixels is in
include/yolo_mi355x.h ("training on tiles"); parity with cv2 / albumentations is unpinned, as for the augmentation. Nothing here
computes pixels, and there is no CPU fallback."""
from __future__ import annotations

import math

import torch

from . import _lib as L
from .boxes import _anchors_to_device
from .data import AUG_NPARAM, augment_params, build_targets
from .extras import _extra_table
from .tiles import _level_hw, _overlap_px, _tile_hw, _tile_origins

__all__ = ["crop_params", "CropPool", "crop_batch", "train_crops"]

CROP_NPARAM = 5                       # YOLO_CROP_NPARAM: [u_pick, background, jx, jy, scale]
CROP_U_PICK, CROP_BACKGROUND, CROP_JX, CROP_JY, CROP_SCALE = range(5)
MAX_CROPS = 65535                     # crops per launch (the grid's second dimension)


def _scale_range(scale):
    try:
        lo, hi = (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError(f"scale must be a (lo, hi) pair of numbers, got {scale!r}") from None
    if not (0.0 < lo <= hi <= 8.0):                           # NaN too
        raise ValueError(f"scale must satisfy 0 < lo <= hi <= 8, got {scale!r}")
    return lo, hi


def crop_params(n, generator=None, scale=(1.0, 1.0), background=0.1):
    """The random draws of ``n`` crops as an (n, 5) float64 table ``[u_pick, background, jx, jy, scale]`` (``YOLO_CROP_*``):
    ``u_pick`` picks the box the window is placed on, ``background`` (1.0 with probability ``background``) makes the crop a
    uniformly placed window instead, ``jx, jy ~ U[0, 1)`` say where in the tile the picked centre falls (or where in the level a
    background window lies), ``scale ~ U[lo, hi]`` is the pyramid scale of the level the crop is cut from (``lo + (hi - lo) * u``:
    exactly ``lo`` when both are equal). All columns come from one ``torch.rand`` call, so a generator state gives one table."""
    lo, hi = _scale_range(scale)
    try:
        bg = float(background)
    except (TypeError, ValueError):
        bg = math.nan
    if not 0.0 <= bg <= 1.0:
        raise ValueError(f"background must be a probability in [0, 1], got {background!r}")
    if int(n) < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    u = torch.rand((int(n), CROP_NPARAM), generator=generator, dtype=torch.float64)
    p = u.clone()
    p[:, CROP_BACKGROUND] = (u[:, CROP_BACKGROUND] < bg).to(torch.float64)
    p[:, CROP_SCALE] = lo + (hi - lo) * u[:, CROP_SCALE]
    return p


_draw_crop_params = crop_params       # CropPool.batch has an argument of the function's name


def _table(name, t, shape, dtype):
    """A caller's table as a tensor of the given shape and dtype (host tables are converted, device tables must match)."""
    try:
        t = torch.as_tensor(t)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must be an array or tensor of shape {tuple(shape)}") from None
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.is_cuda:
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name}: a device table must be a contiguous {dtype} tensor, got {t.dtype}")
        return t
    if dtype == torch.int32 and (t.dtype.is_floating_point or t.dtype == torch.bool):
        raise ValueError(f"{name} must hold integers, got {t.dtype}")
    return t.to(dtype).contiguous()


class CropPool:
    """A device-resident pool of uint8 (H, W, 3) images of any sizes with their boxes, uploaded once: one pinned copy for host
    images, a device copy for device images. ``boxes``: one entry per image, ``[[x, y, w, h, class], ...]`` (normalised, the
    dataset's order), ``[]``, or ``None`` for an image without a label file (background crops only). The pool tensor, its byte
    ``offsets``, ``hw``, the float64 box table and ``nbox`` stay on the device; ``len(pool)`` is the number of images and
    ``pool.nbytes`` the size of the pixel pool."""

    def __init__(self, images, boxes, device=None):
        if isinstance(images, torch.Tensor) and images.dim() == 3 or not isinstance(images, (list, tuple)):
            images = [images]
        ts = []
        for i, im in enumerate(images):
            try:
                t = torch.as_tensor(im)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"image {i}: not an array or tensor ({type(im).__name__})") from None
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError(f"image {i}: images must be uint8 (H, W, 3), got {t.dtype} {tuple(t.shape)}")
            if t.numel() == 0:
                raise ValueError(f"image {i}: has no pixels ({t.shape[0]} x {t.shape[1]})")
            ts.append(t)
        n = len(ts)
        if n == 0:
            raise ValueError("images is empty: a pool needs at least one image")
        if boxes is None or len(boxes) != n:
            raise ValueError(f"boxes must have one entry (a list of rows, [] or None) per image: {n} images")
        rows = []
        for i, bl in enumerate(boxes):
            if bl is None:
                rows.append(None)
                continue
            r = torch.as_tensor(bl, dtype=torch.float64) if len(bl) else torch.zeros((0, 5), dtype=torch.float64)
            if r.dim() != 2 or r.shape[1] != 5:
                raise ValueError(f"image {i}: box rows are [x, y, w, h, class], got shape {tuple(r.shape)}")
            rows.append(r.cpu())
        devs = {t.device for t in ts if t.is_cuda}
        if len(devs) > 1:
            raise ValueError(f"images are on different devices: {sorted(str(d) for d in devs)}")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("training crops run on MI355X only (no CPU fallback)")
        if devs and (device is None or dev.index is None):
            dev = next(iter(devs))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._hw = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
        self._nbox = [-1 if r is None else int(r.shape[0]) for r in rows]
        self.max_boxes = max([1] + self._nbox)                # M of the output table, and max_in of the input one
        offs, o = [], 0
        for t in ts:
            offs.append(o)
            o += t.numel()
        # one pinned staging buffer for the small tables: float64 boxes, then int64 offsets, then int32 hw / nbox
        n_f = n * self.max_boxes * 5
        host = torch.empty(n_f + n + (3 * n + 1) // 2, dtype=torch.float64, pin_memory=True)
        bx = host[:n_f].view(n, self.max_boxes, 5)
        bx.zero_()
        for i, r in enumerate(rows):
            if r is not None and r.shape[0]:
                bx[i, :r.shape[0]] = r
        hi = host[n_f:].view(torch.int64)
        hi[:n] = torch.tensor(offs, dtype=torch.int64)
        h32 = hi[n:].view(torch.int32)
        h32[:2 * n] = torch.tensor([v for s in self._hw for v in s], dtype=torch.int32)
        h32[2 * n:3 * n] = torch.tensor(self._nbox, dtype=torch.int32)
        with torch.cuda.device(dev):
            tab = host.to(dev, non_blocking=True)
            if any(not t.is_cuda for t in ts):
                staged = torch.empty(o, dtype=torch.uint8, pin_memory=True)
                for t, at in zip(ts, offs):
                    if not t.is_cuda:
                        staged[at:at + t.numel()] = t.reshape(-1)
                pool = staged.to(dev, non_blocking=True)
            else:
                pool = torch.empty(o, dtype=torch.uint8, device=dev)
            for t, at in zip(ts, offs):
                if t.is_cuda:
                    pool[at:at + t.numel()].copy_(t.to(dev).reshape(-1))
                    t.record_stream(torch.cuda.current_stream())
        self.pool = pool
        self.boxes = tab[:n_f].view(n, self.max_boxes, 5)
        di = tab[n_f:].view(torch.int64)
        self.offsets = di[:n]
        d32 = di[n:].view(torch.int32)
        self.hw, self.nbox = d32[:2 * n].view(n, 2), d32[2 * n:3 * n]
        self._tab = tab
        self._staging = {}

    def __len__(self):
        return len(self._hw)

    @property
    def nbytes(self):
        return int(self.pool.numel())

    def _workspace(self, B, th, tw):
        key = (B, th, tw)
        if key not in self._staging:
            with torch.cuda.device(self.device):
                self._staging[key] = torch.empty(int(L.lib().yolo_augment_workspace_bytes(B, th, tw)), dtype=torch.uint8, device=self.device)
        return self._staging[key]

    def batch(self, B, tile=416, index=None, crop_params=None, params=None, generator=None, origins=None, scale=(1.0, 1.0),
              background=0.1, min_visibility=0.4, augment=True, out=None, extra=None):
        """``B`` crops of ``tile`` (t or (th, tw), multiples of 32) from the pool. ``index`` (B,) int32: the image of every crop;
        ``crop_params`` (B, 5): the table of :func:`crop_params`; ``params`` (B, 29): the table of :func:`augment_params`. Tables
        that are omitted are drawn from ``generator`` in this order: ``index`` (``torch.randint``), ``crop_params`` (with ``scale``
        and ``background``), then ``params``. ``origins`` (B, 2) int32 ``[y0, x0]``: explicit windows in pixels of each crop's level
        (any values; nothing is picked). ``augment=False``: no HSV / ShiftScaleRotate / flip, ``x`` is the level's pixels times
        1/255 (the bits of ``detect_tiled``'s gather). ``min_visibility``: a remapped box is kept iff the part of it inside the tile
        is at least this fraction of it (0.4: the reference's ``BboxParams``). A picked box larger than the tile can fall under it
        and be dropped; the crop then simply has fewer boxes, or none.

        Returns ``(x (B, 3, th, tw) fp32, boxes (B, M, 5) fp32, counts (B,) int32, windows (B, 6) int32)`` on the device, with
        ``M = pool.max_boxes`` and ``windows[b] = [image, y0, x0, level_h, level_w, picked row or -1]``. Host tables go through one
        pinned staging copy, device tensors (int32 / float64, contiguous) are used in place; there is no host synchronisation and
        nothing is read back, so a device ``index`` is not range-checked here: an entry outside the pool gives an empty crop. With
        every table a device tensor and ``out=`` (the four outputs of an earlier call) the call is capturable in a
        ``torch.cuda.graph``, and a replay follows the tables' current contents.

        ``extra`` (B, 24): the table of :func:`extras.extra_params` (rotation, vertical flip, MixUp, Cutout; needs ``augment``). A
        host table is validated, a device table is used in place; ``M`` is then ``2 * pool.max_boxes``, a crop's boxes followed by
        its MixUp partner's. ``None``: the call without the extras."""
        th, tw = _tile_hw(tile)
        B = int(B)
        if not 1 <= B <= MAX_CROPS:
            raise ValueError(f"B must be in [1, {MAX_CROPS}], got {B}")
        try:
            vis = float(min_visibility)
        except (TypeError, ValueError):
            vis = math.nan
        if not 0.0 <= vis <= 1.0:
            raise ValueError(f"min_visibility must be in [0, 1], got {min_visibility!r}")
        n = len(self)
        if not augment and params is not None:
            raise ValueError("params (the augmentation table) was given with augment=False")
        if not augment and extra is not None:
            raise ValueError("extra (the augmentation extras) was given with augment=False")
        if index is None:
            index = torch.randint(0, n, (B,), generator=generator)
        index = _table("index", index, (B,), torch.int32)
        if not index.is_cuda and B and (int(index.min()) < 0 or int(index.max()) >= n):
            raise ValueError(f"index must lie in [0, {n}) (the pool's images), got {int(index.min())} .. {int(index.max())}")
        if crop_params is None:
            crop_params = _draw_crop_params(B, generator, scale, background)
        cp = _table("crop_params", crop_params, (B, CROP_NPARAM), torch.float64)
        if not cp.is_cuda and not bool(((cp[:, CROP_SCALE] > 0.0) & (cp[:, CROP_SCALE] <= 8.0)).all()):
            raise ValueError("crop_params: the scale column must lie in (0, 8]")
        ap = None
        if augment:
            ap = _table("params", augment_params(B, generator) if params is None else params, (B, AUG_NPARAM), torch.float64)
        org = None if origins is None else _table("origins", origins, (B, 2), torch.int32)
        ex = None if extra is None else _extra_table(extra, B)
        dev = self.device
        for name, t in (("index", index), ("crop_params", cp), ("params", ap), ("origins", org), ("extra", ex)):
            if t is not None and t.is_cuda and t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the pool on {dev}")
        M = self.max_boxes if ex is None else 2 * self.max_boxes
        shapes = ((B, 3, th, tw), torch.float32), ((B, M, 5), torch.float32), ((B,), torch.int32), ((B, 6), torch.int32)
        if out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != 4:
                raise ValueError("out must be the four tensors (x, boxes, counts, windows) of an earlier call")
            for name, t, (shape, dtype) in zip(("x", "boxes", "counts", "windows"), out, shapes):
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"out: {name} must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        # one pinned staging buffer for the host tables: float64 crop / augmentation rows, then int32 index / origins
        host_f = [t for t in (cp, ap, ex) if t is not None and not t.is_cuda]
        host_i = [t for t in (index, org) if t is not None and not t.is_cuda]
        n_f, n_i = sum(t.numel() for t in host_f), sum(t.numel() for t in host_i)
        with torch.cuda.device(dev):
            if n_f + n_i:
                host = torch.empty(n_f + (n_i + 1) // 2, dtype=torch.float64, pin_memory=True)
                h32, at = host[n_f:].view(torch.int32), 0
                for t in host_f:
                    host[at:at + t.numel()] = t.reshape(-1)
                    at += t.numel()
                at = 0
                for t in host_i:
                    h32[at:at + t.numel()] = t.reshape(-1)
                    at += t.numel()
                tab = host.to(dev, non_blocking=True)
                d32, at_f, at_i = tab[n_f:].view(torch.int32), 0, 0

                def placed(t):
                    nonlocal at_f, at_i
                    if t is None or t.is_cuda:
                        return t
                    if t.dtype == torch.float64:
                        v = tab[at_f:at_f + t.numel()].view(t.shape)
                        at_f += t.numel()
                    else:
                        v = d32[at_i:at_i + t.numel()].view(t.shape)
                        at_i += t.numel()
                    return v
                cp, ap, ex = placed(cp), placed(ap), placed(ex)
                index, org = placed(index), placed(org)
            if out is None:
                out = tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in shapes)
            x, ob, ct, win = out
            staging = self._workspace(B, th, tw) if ap is not None else None
            stream = L.current_stream()
            lib = L.lib()
            if ex is not None:
                L.check(lib.yolo_crop_boxes_ex(self.boxes.data_ptr(), self.nbox.data_ptr(), self.max_boxes, self.hw.data_ptr(), n,
                                               index.data_ptr(), cp.data_ptr(), L.ptr(org), ap.data_ptr(), ex.data_ptr(), B, th, tw, vis,
                                               ob.data_ptr(), ct.data_ptr(), M, win.data_ptr(), stream), "yolo_crop_boxes_ex")
                L.check(lib.yolo_crop_images_ex(self.pool.data_ptr(), self.offsets.data_ptr(), self.hw.data_ptr(), n, win.data_ptr(),
                                                ap.data_ptr(), ex.data_ptr(), B, th, tw, staging.data_ptr(), x.data_ptr(), stream),
                        "yolo_crop_images_ex")
                return x, ob, ct, win
            L.check(lib.yolo_crop_boxes(self.boxes.data_ptr(), self.nbox.data_ptr(), M, self.hw.data_ptr(), n, index.data_ptr(),
                                        cp.data_ptr(), L.ptr(org), L.ptr(ap), B, th, tw, vis, ob.data_ptr(), ct.data_ptr(), M,
                                        win.data_ptr(), stream), "yolo_crop_boxes")
            L.check(lib.yolo_crop_images(self.pool.data_ptr(), self.offsets.data_ptr(), self.hw.data_ptr(), n, win.data_ptr(), L.ptr(ap),
                                         B, th, tw, L.ptr(staging), x.data_ptr(), stream), "yolo_crop_images")
        return x, ob, ct, win

    def train_batch(self, B, anchors, tile=416, **kw):
        """:meth:`batch` followed by :func:`build_targets` on its padded device table: the ``(x, targets)`` a training step
        (``GraphedTrainStep`` / ``YOLOLoss``) consumes, with no host synchronisation. ``kw`` goes to :meth:`batch`."""
        x, bt, ct, _ = self.batch(B, tile=tile, **kw)
        anc = _anchors_to_device(anchors, x.device, (9, 2))
        return x, build_targets(bt, anc, tile, counts=ct, device=x.device)

    def tile_origins(self, tile=416, overlap=0.2, scale=1.0):
        """``(index (T,) int32, origins (T, 2) int32)`` on the host: every :func:`tile_grid` tile of every image's level at
        ``scale``, in image then row-major order - the deterministic pass for validation on tiles:
        ``pool.batch(T, tile, index=index, origins=origins, scale=(scale, scale), augment=False)`` (in chunks of at most 65535)."""
        th, tw = _tile_hw(tile)
        oh, ow = _overlap_px(overlap, th, tw)
        _scale_range((scale, scale))
        idx, org = [], []
        for k, (h, w) in enumerate(self._hw):
            lh, lw = _level_hw(h, w, float(scale))
            o = _tile_origins(lh, lw, th, tw, oh, ow)
            org += o
            idx += [k] * (len(o) // 2)
        return torch.tensor(idx, dtype=torch.int32), torch.tensor(org, dtype=torch.int32).reshape(-1, 2)


def _one_shot(images, kw):
    n = len(images) if isinstance(images, (list, tuple)) else 1
    B = kw.pop("B", n)
    if "index" not in kw and B == n:
        kw["index"] = torch.arange(n, dtype=torch.int32)
    return B


def crop_batch(images, boxes, tile=416, device=None, **kw):
    """One-shot form: a :class:`CropPool` of ``images`` / ``boxes`` and one :meth:`CropPool.batch` from it. ``B`` defaults to
    ``len(images)`` and ``index`` to ``arange`` (one crop per image). Returns ``(x, boxes, counts, windows)``."""
    B = _one_shot(images, kw)
    return CropPool(images, boxes, device=device).batch(B, tile=tile, **kw)


def train_crops(images, boxes, anchors, tile=416, device=None, **kw):
    """One-shot form of :meth:`CropPool.train_batch`: ``(x, targets)`` of one crop per image (``B`` / ``index`` as for
    :func:`crop_batch`)."""
    B = _one_shot(images, kw)
    return CropPool(images, boxes, device=device).train_batch(B, anchors, tile=tile, **kw)
