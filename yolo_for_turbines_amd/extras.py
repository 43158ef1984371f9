"""Augmentation extras (csrc/augment.h): rotation, vertical flip, MixUp and Cutout on the device, for both
:func:`augment_batch` and :meth:`CropPool.batch`. The reference's transform list (HSV, shift-scale, horizontal flip, mosaic) was
chosen for ground-level photographs; drone shots of blades show damage at every orientation, and the rare class is small and sparse.
The draws live in a second table, ``(B, 24)`` float64 (``YOLO_AUGX_*`` in include/yolo_mi355x.h, which holds the contract), passed
as ``extra=``; ``extra=None`` is the call without it, bit for bit. The ``ellipse`` rotate method, shear and perspective are not
built. Parity with cv2 / albumentations is unpinned, as for the rest of the augmentation: the kernels follow the published
algorithms and are pinned to tests/augx_ref.py. Nothing here computes pixels, and there is no CPU fallback."""
from __future__ import annotations

import math

import torch

__all__ = ["extra_params", "EXTRA_NPARAM"]

EXTRA_NPARAM = 24                     # YOLO_AUGX_NPARAM
ROT_COS, ROT_SIN, DO_VFLIP, MIX_PARTNER, MIX_LAMBDA, CUT_N, CUT_COVER, CUT_FILL, CUT_RECT = range(9)
CUT_MAX = 4                           # rectangles per row: CUT_RECT + 4k .. + 4k + 3 = (x0, y0, x1, y1), k < 4
# columns of the one torch.rand call behind extra_params: angle, vflip, mix gate, partner, lambda, cutout gate, count, then
# (w, h, cx, cy) of every rectangle
_NDRAW = 7 + 4 * CUT_MAX


def _prob(name, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"{name} must be a probability in [0, 1], got {v!r}")
    return f


def _pair(name, v, lo_min, hi_max):
    try:
        lo, hi = (float(t) for t in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (lo, hi) pair of numbers, got {v!r}") from None
    if not (lo_min <= lo <= hi <= hi_max):                    # NaN too
        raise ValueError(f"{name} must satisfy {lo_min:g} <= lo <= hi <= {hi_max:g}, got {v!r}")
    return lo, hi


def extra_params(n, generator=None, degrees=0.0, flipud=0.0, mixup=0.0, mix_lambda=(0.4, 0.6), cutout=0.0, cut_max=4,
                 cut_size=(0.05, 0.25), cut_cover=0.6, cut_fill=0.0):
    """The random draws of the extras for ``n`` rows as an (n, 24) float64 table (``YOLO_AUGX_*``): the angle ``~ U(-degrees,
    degrees)`` stored as its cos and sin (float64; the kernels evaluate neither); a vertical flip with probability ``flipud``; with
    probability ``mixup`` (and ``n >= 2``) a partner ``(b + 1 + floor(u (n - 1))) mod n`` - any row but ``b`` - mixed in with
    ``lambda ~ U(mix_lambda)`` as the row's own weight; with probability ``cutout`` between 1 and ``cut_max`` (<= 4) erase
    rectangles with sides ``~ U(cut_size)`` of the canvas and centres uniform on it, filled with ``cut_fill``; a box is dropped when
    more than ``cut_cover`` of it lies inside one rectangle. All draws come from one ``torch.rand`` call, so a generator state gives
    one table. With the defaults the table is the neutral one (cos 1, sin 0, no flip, partner -1, no rectangle), with which every
    call gives the bits of the call without ``extra``."""
    n = int(n)
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    try:
        deg = float(degrees)
    except (TypeError, ValueError):
        deg = math.nan
    if not 0.0 <= deg <= 180.0:
        raise ValueError(f"degrees must be in [0, 180], got {degrees!r}")
    p_flip, p_mix, p_cut = _prob("flipud", flipud), _prob("mixup", mixup), _prob("cutout", cutout)
    l_lo, l_hi = _pair("mix_lambda", mix_lambda, 0.0, 1.0)
    s_lo, s_hi = _pair("cut_size", cut_size, 0.0, 1.0)
    cover = _prob("cut_cover", cut_cover)
    if isinstance(cut_max, bool) or not isinstance(cut_max, int) or not 1 <= cut_max <= CUT_MAX:
        raise ValueError(f"cut_max must be an integer in [1, {CUT_MAX}], got {cut_max!r}")
    fill = float(cut_fill)
    if not math.isfinite(fill):
        raise ValueError(f"cut_fill must be finite, got {cut_fill!r}")
    u = torch.rand((n, _NDRAW), generator=generator, dtype=torch.float64)
    p = torch.zeros((n, EXTRA_NPARAM), dtype=torch.float64)
    ang = torch.deg2rad(-deg + 2.0 * deg * u[:, 0])
    p[:, ROT_COS], p[:, ROT_SIN] = torch.cos(ang), torch.sin(ang)
    if deg == 0.0:                                            # exactly neutral: the rows take the two-corner box code
        p[:, ROT_COS], p[:, ROT_SIN] = 1.0, 0.0
    p[:, DO_VFLIP] = (u[:, 1] < p_flip).to(torch.float64)
    rows = torch.arange(n, dtype=torch.float64)
    partner = torch.remainder(rows + 1.0 + torch.floor(u[:, 3] * (n - 1)), max(n, 1))
    mixed = (u[:, 2] < p_mix) & (n >= 2)
    p[:, MIX_PARTNER] = torch.where(mixed, partner, torch.full_like(partner, -1.0))
    p[:, MIX_LAMBDA] = l_lo + (l_hi - l_lo) * u[:, 4]
    count = torch.clamp(1.0 + torch.floor(u[:, 6] * cut_max), max=float(cut_max))
    p[:, CUT_N] = torch.where(u[:, 5] < p_cut, count, torch.zeros_like(count))
    p[:, CUT_COVER], p[:, CUT_FILL] = cover, fill
    for k in range(CUT_MAX):
        w, h, cx, cy = (u[:, 7 + 4 * k + j] for j in range(4))
        w, h = s_lo + (s_hi - s_lo) * w, s_lo + (s_hi - s_lo) * h
        live = (p[:, CUT_N] > k).to(torch.float64)            # rectangles past CUT_N stay zero (they are not read)
        at = CUT_RECT + 4 * k
        p[:, at], p[:, at + 1] = (cx - w / 2) * live, (cy - h / 2) * live
        p[:, at + 2], p[:, at + 3] = (cx + w / 2) * live, (cy + h / 2) * live
    return p


def _extra_table(extra, B):
    """``extra=`` of a batch call as a tensor: a contiguous float64 device tensor is taken as it is, unchecked (its contents may
    change between the replays of a graph); a host table is validated."""
    try:
        t = torch.as_tensor(extra)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"extra must be an array or tensor of shape ({B}, {EXTRA_NPARAM})") from None
    if tuple(t.shape) != (B, EXTRA_NPARAM):
        raise ValueError(f"extra must have shape ({B}, {EXTRA_NPARAM}), got {tuple(t.shape)}")
    if t.is_cuda:
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"extra: a device table must be a contiguous torch.float64 tensor, got {t.dtype}")
        return t
    t = t.to(torch.float64).contiguous()
    if not bool(((t[:, ROT_COS] ** 2 + t[:, ROT_SIN] ** 2 - 1.0).abs() <= 1e-9).all()):      # NaN too
        raise ValueError("extra: ROT_COS, ROT_SIN must be the cos and sin of one angle (cos^2 + sin^2 = 1 to 1e-9)")
    if not bool(torch.isfinite(t[:, [DO_VFLIP, MIX_PARTNER, CUT_FILL]]).all()):
        raise ValueError("extra: DO_VFLIP, MIX_PARTNER and CUT_FILL must be finite")
    if not bool(((t[:, MIX_LAMBDA] >= 0.0) & (t[:, MIX_LAMBDA] <= 1.0)).all()):
        raise ValueError("extra: MIX_LAMBDA must lie in [0, 1]")
    if not bool(((t[:, CUT_COVER] >= 0.0) & (t[:, CUT_COVER] <= 1.0)).all()):
        raise ValueError("extra: CUT_COVER must lie in [0, 1]")
    cn = t[:, CUT_N]
    if not bool(((cn >= 0.0) & (cn <= float(CUT_MAX)) & (cn == torch.floor(cn))).all()):
        raise ValueError(f"extra: CUT_N must be an integer in 0 .. {CUT_MAX}")
    if not bool(torch.isfinite(t[:, CUT_RECT:]).all()):
        raise ValueError("extra: the CUT_RECT columns must be finite")
    return t


def _host_partners(t, B):
    """MIX_PARTNER of a validated host table as a list: the partner row, or -1 (the kernels' rule)."""
    out = []
    for b, v in enumerate(t[:, MIX_PARTNER].tolist()):
        ok = 0.0 <= v < B and v == math.floor(v) and int(v) != b
        out.append(int(v) if ok else -1)
    return out
