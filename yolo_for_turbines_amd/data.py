"""A dataset's work on the device: targets (csrc/targets.hip), letterbox (csrc/preprocess.hip), augmentation (csrc/augment.hip)."""
import ctypes as C

import torch

from . import _lib as L
from .boxes import STRIDES, _anchors_to_device, _grid_hw


def build_targets(boxes, anchors, image_size, counts=None, ignore_iou_threshold=0.5, device=None):
    """Batched device version of the target loop of ``YOLODataset.__getitem__`` (dataset.py:119-161).

    ``boxes``: per-image lists ``[[x, y, w, h, class], ...]`` (normalised, the dataset's order) or a padded
    ``(B, max_boxes, 5)`` tensor with ``counts`` (B). ``anchors``: the 3x3x2 normalised anchor table
    (``config.ANCHORS``). ``image_size``: S or (H, W) (multiples of 32; per-axis grids, see ``yolo_build_targets_hw``).
    Returns the tuple of three ``(B, 3, gh, gw, 6)`` fp32 tensors the loss consumes."""
    if isinstance(boxes, torch.Tensor):
        if counts is None:
            raise ValueError("a padded box tensor needs `counts`")
        bt = boxes.to(dtype=torch.float32)
        dev = bt.device if device is None else torch.device(device)
        ct = torch.as_tensor(counts, dtype=torch.int32)
    else:
        B = len(boxes)
        mb = max(1, max((len(b) for b in boxes), default=1))
        host = torch.zeros((B, mb, 5), dtype=torch.float32)
        ct = torch.tensor([len(b) for b in boxes], dtype=torch.int32)
        for i, bl in enumerate(boxes):
            if len(bl):
                host[i, :len(bl)] = torch.as_tensor(bl, dtype=torch.float32).reshape(-1, 5)
        bt = host
        dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("build_targets runs on MI355X only (no CPU fallback)")
    bt = bt.to(dev).contiguous()
    ct = ct.to(dev).contiguous()
    anc = torch.as_tensor(anchors, dtype=torch.float32).reshape(9, 2).to(dev).contiguous()
    B, mb = bt.shape[0], bt.shape[1]
    H, W = _grid_hw(image_size)
    with torch.cuda.device(dev):
        outs = [torch.empty((B, 3, H // s, W // s, 6), dtype=torch.float32, device=dev) for s in STRIDES]
        L.check(L.lib().yolo_build_targets_hw(bt.data_ptr(), ct.data_ptr(), mb, anc.data_ptr(), B, H, W, float(ignore_iou_threshold),
                                              outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), L.current_stream()),
                "yolo_build_targets")
    return tuple(outs)


def letterbox(images, image_size=416, device=None, rect=False):
    """``config.set_only_image_transforms`` (config.py:101-113) on the device: each uint8 (H, W, 3) image (tensor or
    array) is resized so that its longer side is ``image_size`` (bilinear), centred on a zero canvas, scaled to [0,1]
    and laid out CHW. Returns ``(batch (B,3,Hc,Wc) fp32, meta)`` with ``meta[i] = (orig_h, orig_w, new_h, new_w,
    pad_top, pad_left)`` for :func:`unletterbox_boxes`. Parity with cv2 is unpinned (see csrc/preprocess.hip).
    ``rect=False``: the canvas is ``image_size`` square. ``rect=True``: (Hc, Wc) are the smallest multiples of 32 that hold
    every resized image of the batch (``yolo_letterbox_canvas``); resize arithmetic and the centring rule are the square
    path's, so the resized pixels are the same bits as the interior of the square letterbox."""
    if isinstance(images, (torch.Tensor,)) and images.dim() == 3 or not isinstance(images, (list, tuple)):
        images = [images]
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("letterbox runs on MI355X only (no CPU fallback)")
    S = int(image_size)
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("images must be uint8 (H, W, 3)")
        ts.append(t)
    hw = (C.c_int32 * max(2 * len(ts), 2))(*[int(v) for t in ts for v in t.shape[:2]])
    canvas = (C.c_int32 * 2)()
    L.check(L.lib().yolo_letterbox_canvas(hw, len(ts), S, int(bool(rect)), canvas), "yolo_letterbox_canvas")
    Hc, Wc = int(canvas[0]), int(canvas[1])
    with torch.cuda.device(dev):
        out = torch.empty((len(ts), 3, Hc, Wc), dtype=torch.float32, device=dev)
        meta = []
        for i, t in enumerate(ts):
            t = t.to(dev).contiguous()
            nhw, pad = (C.c_int * 2)(), (C.c_int * 2)()
            L.check(L.lib().yolo_letterbox_hw(t.data_ptr(), t.shape[0], t.shape[1], S, Hc, Wc, out[i].data_ptr(), nhw, pad,
                                              L.current_stream()), "yolo_letterbox")
            t.record_stream(torch.cuda.current_stream())
            meta.append((int(t.shape[0]), int(t.shape[1]), nhw[0], nhw[1], pad[0], pad[1]))
    return out, meta


def unletterbox_boxes(boxes, original_hw, resized_hw, meta=None):
    """Box mapping of ``plot_original`` (utils.py:475-501): normalised letterboxed ``[cx, cy, w, h, obj, cls]`` rows ->
    coordinates normalised to the ORIGINAL image. Same arithmetic (incl. its ``int(o * scale)`` size and ``// 2`` padding).
    ``resized_hw`` is the canvas (H, W). The reference's formula re-derives the resize from the canvas, which is only exact
    for a square canvas: on a rectangular one the short side can hold padding of its own (another image of the batch set the
    canvas, or the resized side was rounded up to 32), and ``min(r_w / o_w, r_h / o_h)`` then picks the wrong axis or is
    off by a rounding. ``meta`` (the tuple :func:`letterbox` returned for this image) uses the letterbox's own resized size
    and padding instead."""
    r_h, r_w = resized_hw
    if meta is not None:
        _, _, new_height, new_width, pad_height, pad_width = meta
    else:
        o_h, o_w = original_hw
        scale = min(r_w / o_w, r_h / o_h)
        new_width, new_height = int(o_w * scale), int(o_h * scale)
        pad_width, pad_height = (r_w - new_width) // 2, (r_h - new_height) // 2
    return [[(b[0] * r_w - pad_width) / new_width, (b[1] * r_h - pad_height) / new_height, (b[2] * r_w) / new_width,
             (b[3] * r_h) / new_height, b[4], b[5]] for b in boxes]


AUG_NPARAM = 29                       # YOLO_AUG_NPARAM: [do_hsv, hue, sat, val, do_ssr, scale, dx, dy, do_flip, (mx_k, my_k) k < 10]


def augment_params(n, generator=None, mosaic=False):
    """The random draws of ``config.set_train_transforms`` for ``n`` images as an (n, 29) float64 table: each transform
    on with p = 0.5; ``hue ~ U(-2, 2)``, ``sat ~ U(-50, 50)``, ``val ~ U(-40, 40)`` (HueSaturationValue(2, 50, 40)),
    ``scale ~ U(1, 1.5)``, ``dx, dy ~ U(-0.0625, 0.0625)`` (ShiftScaleRotate(scale_limit=(0, 0.5), rotate_limit=0)), and
    with ``mosaic`` the 10 cutout draws ``(x, y) ~ U(0.2, 0.3)`` of ``mosaic_augmentation``. The same generator state
    gives the same table (the draws are taken in one call whether or not ``mosaic`` is set)."""
    u = torch.rand((int(n), AUG_NPARAM), generator=generator, dtype=torch.float64)
    p = torch.zeros((int(n), AUG_NPARAM), dtype=torch.float64)
    for col in (0, 4, 8):
        p[:, col] = (u[:, col] < 0.5).to(torch.float64)
    p[:, 1] = -2.0 + 4.0 * u[:, 1]
    p[:, 2] = -50.0 + 100.0 * u[:, 2]
    p[:, 3] = -40.0 + 80.0 * u[:, 3]
    p[:, 5] = 1.0 + 0.5 * u[:, 5]
    p[:, 6] = -0.0625 + 0.125 * u[:, 6]
    p[:, 7] = -0.0625 + 0.125 * u[:, 7]
    if mosaic:
        p[:, 9:] = 0.2 + 0.1 * u[:, 9:]
    return p


def _resized_hw(h, w, size):
    scale = size / float(max(h, w))
    nh, nw = (int(round(h * scale)), int(round(w * scale))) if scale != 1.0 else (h, w)   # round(): half to even
    return max(nh, 1), max(nw, 1)


def augment_batch(images, boxes, image_size=416, params=None, generator=None, mosaic=None, device=None, extra=None):
    """``YOLODataset.apply_augmentations`` (dataset.py:75-111) for a whole batch on the device, with no host synchronisation.

    ``images``: list of uint8 (H, W, 3) tensors or arrays (CPU: staged with one pinned copy; or already on the device).
    ``boxes``: one entry per image, ``[[x, y, w, h, class], ...]`` (normalised, the dataset's order) or ``None`` for an image
    without a label file (letterbox only, count 0; dataset.py:162-165). ``image_size``: S or (H, W) (multiples of 32).
    ``mosaic``: ``None`` (output image b is the standard transform of ``images[b]``) or a (B, 4) index array into ``images``:
    row b is ``mosaic_augmentation`` of the four images followed by ``set_train_transforms(mosaic=True)``; a row
    ``[i, -1, -1, -1]`` is the standard transform of image i. ``params``: the (B, 29) table of :func:`augment_params`
    (drawn from ``generator`` when omitted). Returns ``(x (B, 3, H, W) fp32, boxes (B, M, 5) fp32, counts (B,) int32)``, all
    on the device: the padded box table is the input of :func:`build_targets`. Parity with cv2 / albumentations is unpinned
    (see csrc/augment.hip). ``extra``: the (B, 24) table of :func:`extras.extra_params` (rotation, vertical flip, MixUp, Cutout);
    ``M`` then holds a row's boxes plus its MixUp partner's (the exact sum for a host table, twice the largest row for a device
    table, which is used in place and not read). ``None``: the call without the extras."""
    x, out_boxes, counts, launch = _augment_prepare(images, boxes, image_size, params, generator, mosaic, device, extra)
    launch()
    return x, out_boxes, counts


def _augment_prepare(images, boxes, image_size, params, generator, mosaic, device, extra=None):
    """augment_batch up to the launches: validated tables uploaded, outputs allocated; ``launch()`` enqueues the kernels
    (tools/augment_bench.py times it alone)."""
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("augment_batch runs on MI355X only (no CPU fallback)")
    H, W = _grid_hw(image_size)
    ts = []
    for im in images:
        t = torch.as_tensor(im)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("images must be uint8 (H, W, 3)")
        ts.append(t)
    n = len(ts)
    if n == 0 or len(boxes) != n:
        raise ValueError("augment_batch needs at least one image and one box entry (or None) per image")
    if mosaic is None:
        src = [[i, -1, -1, -1] for i in range(n)]
    else:
        src = [[int(v) for v in row] for row in (mosaic.tolist() if hasattr(mosaic, "tolist") else mosaic)]
        if any(len(r) != 4 for r in src):
            raise ValueError("mosaic must be a (B, 4) index array")
        S = max(H, W)
        for r in src:
            if r[1] < 0:
                continue
            if H != W:
                raise ValueError(f"mosaic needs a square image_size (got {H}x{W}): rectangular mosaic is not built")
            if any(not 0 <= k < n for k in r):
                raise ValueError(f"mosaic row {r} indexes outside the {n} images")
            sizes = {_resized_hw(int(ts[k].shape[0]), int(ts[k].shape[1]), S) for k in r}
            if len(sizes) != 1:
                raise ValueError(f"mosaic row {r}: the four images resize to different sizes {sorted(sizes)} (the reference "
                                 "needs them equal)")
    B = len(src)
    if params is None:
        params = augment_params(B, generator, mosaic=mosaic is not None)
    params = torch.as_tensor(params)
    if tuple(params.shape) != (B, AUG_NPARAM):
        raise ValueError(f"params must be ({B}, {AUG_NPARAM})")
    # host tables: box rows per pool image (None -> -1), the pool layout, the source slots
    nbox = [-1 if b is None else len(b) for b in boxes]
    max_in = max([1] + nbox)
    own = [sum(max(nbox[k], 0) for k in r if k >= 0) for r in src]
    max_out = max(1, max(own))
    ex_host = False
    if extra is not None:
        from .extras import EXTRA_NPARAM, _extra_table, _host_partners
        extra = _extra_table(extra, B)
        ex_host = not extra.is_cuda
        on = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        if extra.is_cuda and extra.device != on:             # used in place: the kernels would read another device's memory
            raise ValueError(f"extra is on {extra.device}, the batch on {on}")
        if ex_host:
            max_out = max(1, max(o + (own[q] if q >= 0 else 0) for o, q in zip(own, _host_partners(extra, B))))
        else:
            max_out = 2 * max_out
    n_ex = B * EXTRA_NPARAM if ex_host else 0
    hw_l = [int(v) for t in ts for v in t.shape[:2]]
    src_l = [k for r in src for k in r]
    # one pinned staging buffer for every small table: float64 params + boxes, then int64 offsets, then int32 hw / src / nbox
    n_f = (0 if params.device.type == "cuda" else B * AUG_NPARAM) + n * max_in * 5 + n_ex
    n_i = n + (2 * n + 4 * B + n + 1) // 2
    host = torch.empty(n_f + n_i, dtype=torch.float64, pin_memory=True)
    hf = host[:n_f]
    off_p = 0
    if params.device.type != "cuda":
        hf[:B * AUG_NPARAM] = params.to(torch.float64).reshape(-1)
        off_p = B * AUG_NPARAM
    bx = hf[off_p:off_p + n * max_in * 5].view(n, max_in, 5)
    bx.zero_()
    for i, bl in enumerate(boxes):
        if bl is not None and len(bl):
            bx[i, :len(bl)] = torch.as_tensor(bl, dtype=torch.float64).reshape(-1, 5)
    if ex_host:
        hf[n_f - n_ex:] = extra.reshape(-1)
    hi = host[n_f:].view(torch.int64)
    cpu = [i for i, t in enumerate(ts) if t.device.type != "cuda"]
    offs, o = [0] * n, 0
    for i in cpu + [i for i in range(n) if i not in cpu]:
        offs[i] = o
        o += ts[i].numel()
    hi[:n] = torch.tensor(offs, dtype=torch.int64)
    h32 = hi[n:].view(torch.int32)
    h32[:2 * n] = torch.tensor(hw_l, dtype=torch.int32)
    h32[2 * n:2 * n + 4 * B] = torch.tensor(src_l, dtype=torch.int32)
    h32[2 * n + 4 * B:3 * n + 4 * B] = torch.tensor(nbox, dtype=torch.int32)
    n_cpu_bytes = sum(ts[i].numel() for i in cpu)
    if n_cpu_bytes:
        pool_host = torch.empty(n_cpu_bytes, dtype=torch.uint8, pin_memory=True)
        for i in cpu:
            pool_host[offs[i]:offs[i] + ts[i].numel()] = ts[i].reshape(-1)
    with torch.cuda.device(dev):
        dtab = host.to(dev, non_blocking=True)
        pool = torch.empty(max(o, 1), dtype=torch.uint8, device=dev)
        if n_cpu_bytes:
            pool[:n_cpu_bytes].copy_(pool_host, non_blocking=True)
        for i in range(n):
            if i not in cpu:
                pool[offs[i]:offs[i] + ts[i].numel()].copy_(ts[i].to(dev).reshape(-1))
                ts[i].record_stream(torch.cuda.current_stream())
        dp = params.to(dev, torch.float64).contiguous() if params.device.type == "cuda" else dtab[:B * AUG_NPARAM]
        dbox = dtab[off_p:n_f - n_ex]
        dex = None if extra is None else (dtab[n_f - n_ex:n_f] if ex_host else extra)
        di = dtab[n_f:].view(torch.int64)
        d32 = di[n:].view(torch.int32)
        dhw, dsrc, dnbox = d32[:2 * n], d32[2 * n:2 * n + 4 * B], d32[2 * n + 4 * B:3 * n + 4 * B]
        x = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        out_boxes = torch.empty((B, max_out, 5), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        sel = torch.empty((B,), dtype=torch.int32, device=dev)
        staging = torch.empty(int(L.lib().yolo_augment_workspace_bytes(B, H, W)), dtype=torch.uint8, device=dev)
        hw_c = (C.c_int32 * (2 * n))(*hw_l)
        src_c = (C.c_int32 * (4 * B))(*src_l)

    def launch():
        with torch.cuda.device(dev):
            stream = L.current_stream()
        if dex is not None:
            L.check(L.lib().yolo_augment_boxes_ex(dbox.data_ptr(), dnbox.data_ptr(), max_in, dhw.data_ptr(), dsrc.data_ptr(), hw_c, n,
                                                  src_c, dp.data_ptr(), dex.data_ptr(), B, H, W, out_boxes.data_ptr(), counts.data_ptr(),
                                                  max_out, sel.data_ptr(), stream), "yolo_augment_boxes_ex")
            L.check(L.lib().yolo_augment_images_ex(pool.data_ptr(), di.data_ptr(), dhw.data_ptr(), dsrc.data_ptr(), hw_c, n, src_c,
                                                   dp.data_ptr(), dex.data_ptr(), sel.data_ptr(), B, H, W, staging.data_ptr(),
                                                   x.data_ptr(), stream), "yolo_augment_images_ex")
            return
        L.check(L.lib().yolo_augment_boxes(dbox.data_ptr(), dnbox.data_ptr(), max_in, dhw.data_ptr(), dsrc.data_ptr(), hw_c, n, src_c,
                                           dp.data_ptr(), B, H, W, out_boxes.data_ptr(), counts.data_ptr(), max_out, sel.data_ptr(),
                                           stream), "yolo_augment_boxes")
        L.check(L.lib().yolo_augment_images(pool.data_ptr(), di.data_ptr(), dhw.data_ptr(), dsrc.data_ptr(), hw_c, n, src_c,
                                            dp.data_ptr(), sel.data_ptr(), B, H, W, staging.data_ptr(), x.data_ptr(), stream),
                "yolo_augment_images")
    return x, out_boxes, counts, launch


def train_batch(images, boxes, anchors, image_size=416, **kw):
    """:func:`augment_batch` followed by :func:`build_targets` on its padded device table: the ``(x, targets)`` a training
    step (``GraphedTrainStep`` / ``YOLOLoss``) consumes, with no host synchronisation. ``kw`` goes to :func:`augment_batch`."""
    x, bt, ct = augment_batch(images, boxes, image_size=image_size, **kw)
    anc = _anchors_to_device(anchors, x.device, (9, 2))
    return x, build_targets(bt, anc, image_size, counts=ct, device=x.device)
