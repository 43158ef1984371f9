"""The shared small inputs of tests/test_augx_host.py and tests/test_gpu_augx.py (the augmentation extras). One pool of images per
canvas - 32 x 32, 64 x 96 and 96 x 64 - with landscape, portrait and exact-size images and one image without a label file, and a
list of cases: the (B, 29) augmentation table, the (B, 24) extras table, the source rows of ``augment_batch`` (``mosaic``) and the
``index`` / ``crop_params`` of ``CropPool.batch``. The host test checks on the restatement that no case compares empty box tables;
the GPU test runs every case through both calls. B is 4 throughout."""
import math

import numpy as np

from tests import augx_ref as xr

B = 4


def _img(seed, h, w):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)      # smooth-ish content plus noise
    big = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w].astype(np.int32)
    return np.clip(big + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


_CENTRE = [[0.5, 0.5, 0.5, 0.5, 1.0], [0.4, 0.45, 0.2, 0.3, 0.0], [0.93, 0.3, 0.2, 0.3, 1.0], [0.55, 0.6, 0.12, 0.1, 0.0],
           [0.08, 0.1, 0.14, 0.16, 1.0]]                     # the last sits in a corner: a turn of 45 degrees takes it off the canvas
_TWO = [[0.45, 0.5, 0.3, 0.4, 0.0], [0.1, 0.85, 0.3, 0.3, 1.0], [0.92, 0.9, 0.14, 0.16, 0.0]]

# canvas -> (sizes, boxes): image 0 .. 2 of every pool carry boxes; the last has no label file. (32, 32): images 0, 1, 3, 4 resize
# to 24 x 32 (one mosaic), 2 is a portrait, 5 has exactly the canvas' size.
_POOLS = {
    (32, 32): ([(24, 32), (48, 64), (40, 28), (36, 48), (12, 16), (32, 32), (30, 26)],
               [_CENTRE, _TWO, _CENTRE, _TWO, _CENTRE[:2], _CENTRE, None]),
    (64, 96): ([(20, 45), (64, 96), (30, 90), (33, 50)], [_CENTRE, _CENTRE, _TWO, None]),
    (96, 64): ([(45, 20), (96, 64), (90, 30), (50, 33)], [_CENTRE, _CENTRE, _TWO, None]),
}
POOLS = {k: ([_img(700 + 10 * i + j, h, w) for j, (h, w) in enumerate(sizes)], boxes)
         for i, (k, (sizes, boxes)) in enumerate(_POOLS.items())}

_DRAWS = [0.2 + 0.005 * k for k in range(20)]


def _p(hsv=False, ssr=False, scale=1.0, dx=0.0, dy=0.0, flip=False):
    return [float(hsv), 1.5, -30.0, 25.0, float(ssr), scale, dx, dy, float(flip)] + _DRAWS


def _e(deg=None, vflip=False, partner=-1.0, lam=0.5, cover=0.6, fill=0.0, rects=()):
    e = np.zeros(xr.NPARAM)
    if deg is None:
        e[xr.ROT_COS], e[xr.ROT_SIN] = 1.0, 0.0
    else:
        e[xr.ROT_COS], e[xr.ROT_SIN] = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    e[xr.DO_VFLIP], e[xr.MIX_PARTNER], e[xr.MIX_LAMBDA] = float(vflip), partner, lam
    e[xr.CUT_N], e[xr.CUT_COVER], e[xr.CUT_FILL] = len(rects), cover, fill
    for k, r in enumerate(rects):
        e[xr.CUT_RECT + 4 * k:xr.CUT_RECT + 4 * k + 4] = r
    return e


def _std(rows):
    return [[i, -1, -1, -1] for i in rows]


# crop rows: [u_pick, background, jx, jy, scale]
_CP = [[0.1, 0.0, 0.4, 0.6, 1.0], [0.6, 0.0, 0.5, 0.5, 1.0], [0.3, 0.0, 0.5, 0.4, 1.0], [0.2, 1.0, 0.3, 0.7, 1.0]]


def _case(name, kind, canvas, params, extra, mosaic, index, cp=_CP):
    assert len(params) == len(extra) == len(mosaic) == len(index) == len(cp) == B
    return dict(name=name, kind=kind, canvas=canvas, params=np.asarray(params, np.float64), extra=np.asarray(extra, np.float64),
                mosaic=np.asarray(mosaic, np.int32), index=list(index), cp=np.asarray(cp, np.float64))


_MOS = [[0, 1, 3, 4], [2, -1, -1, -1], [5, -1, -1, -1], [6, -1, -1, -1]]      # a mosaic row, a portrait, exact size, no label file
_SSR = dict(ssr=True, scale=1.3, dx=0.05, dy=-0.04)
_PLAIN = dict(ssr=True)                                      # ShiftScaleRotate on, scale 1, no shift: the rotation alone
_BIG = [0.05, 0.1, 0.62, 0.55]                               # erase rectangles
_RECTS4 = [[0.13, 0.21, 0.37, 0.48], [0.7, -0.2, 1.3, 0.33], [0.6, 0.5, 0.4, 0.9], [0.41, 0.77, 0.93, 0.99]]   # 2: hangs over, 3: empty

CASES = [
    # ---- neutral extras: a mosaic row; rows with and without ShiftScaleRotate
    _case("neutral_32", "neutral", (32, 32), [_p(True, **_SSR), _p(flip=True), _p(True, **_SSR, flip=True), _p(**_SSR)],
          [_e() for _ in range(B)], _MOS, [1, 2, 5, 6]),
    _case("neutral_64x96", "neutral", (64, 96), [_p(**_SSR), _p(True), _p(True, **_SSR, flip=True), _p()],
          [_e() for _ in range(B)], _std([0, 1, 2, 3]), [0, 1, 2, 3], [[0.1, 0.0, 0.4, 0.6, 2.0]] + _CP[1:]),
    # ---- rotation
    _case("rot_32_scaled", "rotation", (32, 32), [_p(True, **_SSR), _p(**_SSR, flip=True), _p(**_SSR), _p(**_SSR)],
          [_e(7), _e(-45, vflip=True), _e(90), _e(180)], [_MOS[0], _MOS[2], _MOS[1], _MOS[3]], [1, 5, 2, 0]),
    _case("rot_32_plain", "rotation", (32, 32), [_p(**_PLAIN), _p(**_PLAIN, flip=True), _p(**_PLAIN), _p(**_PLAIN)],
          [_e(-7), _e(45, vflip=True), _e(90), _e(-45)], _std([0, 5, 2, 1]), [1, 5, 2, 0]),
    _case("rot_64x96", "rotation", (64, 96), [_p(**_SSR), _p(**_PLAIN), _p(True, **_SSR, flip=True), _p(**_PLAIN)],
          [_e(7), _e(-7), _e(45, vflip=True), _e(180)], _std([0, 1, 2, 1]), [0, 1, 1, 2], [[0.1, 0.0, 0.4, 0.6, 2.0]] + _CP[1:]),
    _case("rot_96x64", "rotation", (96, 64), [_p(**_PLAIN), _p(**_SSR), _p(**_SSR, flip=True), _p(**_PLAIN)],
          [_e(45), _e(90), _e(7, vflip=True), _e(180)], _std([1, 1, 2, 0]), [1, 1, 2, 0]),
    # ---- MixUp. mutual: 0 <-> 1, row 0 with ShiftScaleRotate mixes in row 1 without it (never staged without the extras), and
    # row 3 mixes in row 2; lambda 0, 1 and interior
    _case("mix_mutual", "mixup", (32, 32), [_p(True, **_SSR), _p(True, flip=True), _p(), _p(**_SSR)],
          [_e(partner=1.0, lam=0.3), _e(partner=0.0, lam=1.0), _e(), _e(partner=2.0, lam=0.0)], _MOS[:3] + [[1, -1, -1, -1]],
          [1, 2, 5, 0]),
    # a chain 0 -> 1 -> 2 (not transitive), a partner without a label file (row 2 -> row 3)
    _case("mix_chain", "mixup", (32, 32), [_p(**_SSR), _p(flip=True), _p(True), _p(True, **_SSR)],
          [_e(partner=1.0, lam=0.7), _e(partner=2.0, lam=0.25, vflip=True), _e(partner=3.0, lam=0.6), _e()],
          _std([0, 2, 5, 6]), [1, 2, 5, 6]),
    # partners that all mean none: -1, the row itself, B, a non-integer
    _case("mix_none", "mixup", (32, 32), [_p(**_SSR), _p(), _p(True), _p(**_SSR)],
          [_e(partner=-1.0), _e(partner=1.0), _e(partner=float(B)), _e(partner=1.5)], _std([0, 2, 5, 1]), [1, 2, 5, 0]),
    _case("mix_64x96", "mixup", (64, 96), [_p(**_SSR), _p(), _p(True, flip=True), _p(**_SSR)],
          [_e(30, partner=1.0, lam=0.4), _e(partner=0.0, lam=0.55), _e(partner=3.0, lam=0.5), _e(partner=2.0, lam=0.5)],
          _std([0, 1, 2, 3]), [0, 1, 2, 3]),
    # ---- Cutout: 0, 1 and 4 rectangles, edges at non-integer pixels, one hanging over the edge, an empty one, a non-zero fill,
    # both flips on (rectangles are in output coordinates)
    _case("cut_32", "cutout", (32, 32), [_p(), _p(flip=True), _p(**_SSR, flip=True), _p(True)],
          [_e(), _e(rects=[_BIG], fill=0.5, vflip=True), _e(rects=_RECTS4, fill=0.25, vflip=True), _e(rects=[_BIG], cover=0.3)],
          _std([0, 2, 5, 1]), [1, 2, 5, 0]),
    # the strict threshold on the exact-size image (its box [0.25, 0.75]^2 is exact): the right half erased, kept at cover 0.5,
    # dropped just under it
    _case("cut_strict", "cutout", (32, 32), [_p(), _p(), _p(), _p()],
          [_e(rects=[[0.5, 0.0, 1.0, 1.0]], cover=0.5), _e(rects=[[0.5, 0.0, 1.0, 1.0]], cover=0.5 - 2.0 ** -30),
           _e(rects=[[0.0, 0.0, 1.0, 1.0]], fill=1.0), _e(rects=[[0.0, 0.5, 1.0, 1.0]], cover=0.5, fill=0.125)],
          _std([5, 5, 5, 5]), [5, 5, 5, 5], [[0.0, 1.0, 0.0, 0.0, 1.0]] * B),
    _case("cut_96x64", "cutout", (96, 64), [_p(**_SSR), _p(flip=True), _p(), _p(True)],
          [_e(rects=[_BIG]), _e(rects=_RECTS4, fill=0.5, vflip=True), _e(rects=[[0.3, 0.3, 0.31, 0.9]]), _e()],
          _std([0, 1, 2, 3]), [0, 1, 2, 3]),
    # ---- everything at once
    _case("all_32", "all", (32, 32), [_p(True, **_SSR), _p(True, flip=True), _p(**_SSR, flip=True), _p(**_PLAIN)],
          [_e(-20, partner=1.0, lam=0.45, rects=[[0.7, 0.6, 0.95, 0.9]], fill=0.5), _e(vflip=True, partner=2.0, lam=0.6),
           _e(90, vflip=True, rects=_RECTS4[:2]), _e(45, partner=0.0, lam=0.5, rects=[[0.0, 0.0, 0.2, 0.2]])],
          _MOS[:3] + [[1, -1, -1, -1]], [1, 2, 5, 0]),
    _case("all_64x96", "all", (64, 96), [_p(True, **_SSR), _p(flip=True), _p(**_SSR, flip=True), _p(**_PLAIN)],
          [_e(12, partner=1.0, lam=0.45, rects=[[0.7, 0.6, 0.95, 0.9]], fill=0.5), _e(vflip=True, partner=2.0, lam=0.6),
           _e(-30, vflip=True, rects=_RECTS4[:2]), _e(180, partner=3.0, lam=0.5)],
          _std([0, 1, 2, 3]), [0, 1, 2, 3], [[0.1, 0.0, 0.4, 0.6, 2.0]] + _CP[1:]),
]


def reference(case, user):
    """The restatement's (x, per-row boxes) of a case for ``user`` "augment" or "crop"; computed once per (case, user) and shared."""
    key = (case["name"], user)
    if key not in _REF:
        H, W = case["canvas"]
        images, boxes = POOLS[case["canvas"]]
        if user == "augment":
            _REF[key] = xr.augment(images, boxes, case["params"], case["extra"], H, W, case["mosaic"])
        else:
            _REF[key] = xr.crop(images, boxes, case["index"], case["cp"], case["params"], case["extra"], H, W)[:2]
    return _REF[key]


_REF = {}
