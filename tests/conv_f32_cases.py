"""Cases, fp64 reference and host-side restatements for the exact-fp32 convolution kernels: conv_igemm_f32 (tiles 1-4,
conv_f32.hip), conv_patch_f32 (tiles 5-7, conv_f32_v2.hip) and stem3x3_f32 (stem_f32.hip). Shared by
tests/test_conv_f32_cases_host.py (CPU: the bound stays sensitive, the geometry restatement equals yolo_conv_patch_plan, the
address audit of conv_patch_f32 is clean, the tables hold the edges they name) and tests/test_gpu_conv_f32_edges.py.

The bar is a per-element bound derived from the operands. With u = 2^-24, K = k*k*cin, S = conv64(|x|, |w|) and
ref = [r +] act(scale * conv64(x, w) + shift):

    bound = 2 * [ (K + 4) * u * (S * |scale| + |shift|) * L + 2u * |ref| ]  [+ eps_mish * |ref| for Mish]

(K + 4) u (S |scale| + |shift|) is the a-priori bound of a sequential fp32 chain of K products followed by the scale / shift
multiply-add; L (1 for none / leaky, 1.1 for Mish, whose slope reaches 1.09) carries it through the activation; 2u |ref| is the
activation's and the residual add's own rounding; the factor 2 is the margin. eps_mish is 4x the relative error of a plain
fp32 evaluation of the kernels' Mish formula (tests/train_kernels_ref.py), as tests/test_gpu_train_kernels.py takes it.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import train_kernels_ref as R

U = 2.0 ** -24
OUT_NHWC, OUT_UP, OUT_HEAD = 0, 1, 2
V2_LD, V2_NI, V2_PATCH_CAP = 36, 8, 256          # conv_f32_v2.hip
PATCH_TILES = (5, 6, 7)                          # BN 64 / 128 with two patch buffers, BN 64 with one
IGEMM_TILES = (1, 2, 3, 4)                       # 128x128, 128x64, 64x128, 64x64


def eps_mish():
    return 4.0 * _mish_rel()


@functools.lru_cache(maxsize=None)
def _mish_rel():
    return R.mish_fp32_formula_rel_error()


def _c(name, n, h, w, cin, cout, k, s, act=1, res=False, out=OUT_NHWC, x_ld=None, x_off=0, y_pad=0, y_off=0, r_pad=0, r_off=0, why=""):
    cp = (cin + 3) // 4 * 4
    return dict(name=name, n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, act=act, res=res, out=out, x_ld=cp if x_ld is None else x_ld,
                x_off=x_off, y_ld=cout + y_pad, y_off=y_off, r_ld=(cout + r_pad) if res else 0, r_off=r_off if res else 0, why=why)


# The y / residual views, out modes, activations and residual of both direct kernels: (suffix, keywords, the path it takes when
# cout % 4 == 0; with cout % 4 != 0 every one of them is stored element by element)
EPILOGUES = [
    ("vec4", dict(act=1, res=True, y_pad=8, y_off=4, r_pad=4, r_off=4), "all views multiples of 4: 16-byte stores and residual loads"),
    ("yoff2", dict(act=2, res=True, y_pad=6, y_off=2), "y_off 2, y_ld cout + 6: element by element"),
    ("yodd", dict(act=0, y_pad=3), "y_ld odd: element by element"),
    ("roff1", dict(act=1, res=True, r_pad=4, r_off=1), "aligned y, r_off 1: element by element"),
    ("up_vec", dict(act=1, out=OUT_UP, y_pad=64, y_off=64), "2x upsampling store into the second half of a concat buffer, 16 bytes"),
    ("up_odd", dict(act=2, out=OUT_UP, y_pad=6, y_off=2), "2x upsampling store, element by element"),
]


def _epilogue_cases(prefix, n, h, w, cin, k, s):
    return [_c(f"{prefix}_{suf}_c{cout}", n, h, w, cin, cout, k, s, why=why, **kw) for cout in (64, 66) for suf, kw, why in EPILOGUES]


# ---- A. conv_igemm_f32: forced tiles 1-4, and tile 0 where the heuristic routes here (1x1, stride 2, cin <= 4)
IGEMM_CASES = [
    _c("a_m25_kt1", 1, 5, 5, 32, 24, 1, 1, why="M = 25 < BM, cout 24 < BN, KT = 1: no prefetch step"),
    _c("a_m64_kt2", 1, 8, 8, 64, 64, 1, 1, act=0, why="M = 64 = BM of tiles 3 / 4, cout = 64 = BN, KT = 2"),
    _c("a_m65_kt3", 1, 5, 13, 96, 66, 1, 1, act=2, why="M = 65: one row into a second block; cout 66 (scalar stores); KT = 3"),
    _c("a_m129_c132", 1, 3, 43, 32, 132, 1, 1, res=True, why="M = 129 = 128 + 1, cout 132 = 128 + 4"),
    _c("a_straddle_kt9_c255", 3, 13, 13, 32, 255, 3, 1, why="M tiles straddle images (507 pixels), KT = 9, cout 255 in NHWC"),
    _c("a_kt27", 2, 7, 9, 96, 64, 3, 1, act=2, res=True, why="KT = 27: a K step changes tap every third step"),
    _c("a_s1_1x40", 1, 1, 40, 32, 64, 3, 1, why="3x3 on one row: kh = 0 and 2 are padding everywhere"),
    _c("a_s1_5x1", 2, 5, 1, 32, 24, 3, 1, act=0, why="3x3 on one column"),
    _c("a_s1_1x1", 3, 1, 1, 32, 64, 3, 1, why="3x3 on 1 x 1 maps: only the centre tap is real"),
    _c("a_s2_7x9", 3, 7, 9, 32, 66, 3, 2, why="3x3 stride 2, odd map: 4 x 5 outputs"),
    _c("a_s2_16x16", 2, 16, 16, 64, 64, 3, 2, act=2, why="3x3 stride 2, even map: the last tap column is never padding"),
    _c("a_s2_1x1", 2, 1, 1, 32, 24, 3, 2, why="3x3 stride 2 on 1 x 1 maps"),
    _c("a_k1s2_7x9", 2, 7, 9, 32, 64, 1, 2, act=0, why="1x1 stride 2 (pad 0): 4 x 5 outputs"),
    _c("a_xview", 2, 7, 9, 32, 64, 3, 2, x_ld=64, x_off=16, why="x_ld > cin, x_off 16"),
    _c("a_head21", 2, 5, 5, 32, 21, 1, 1, act=0, out=OUT_HEAD, why="head layout, nc5 = 7, M = 50 ragged"),
    _c("a_head255", 1, 5, 13, 64, 255, 1, 1, act=0, out=OUT_HEAD, why="head layout, nc5 = 85, M = 65 ragged"),
]
# SMALLC (cin <= 4: each 16-byte chunk of a K step is one tap): cin 1, 3, 4 with 3x3 stride 1, 3x3 stride 2, 1x1; x_ld 4 and 8
for _i, (_cin, (_k, _s)) in enumerate((ci, ks) for ci in (1, 3, 4) for ks in ((3, 1), (3, 2), (1, 1))):
    _wide = _i % 2 == 1
    IGEMM_CASES.append(_c(f"a_small_c{_cin}_k{_k}s{_s}", 2, 7, 9, _cin, (24, 64, 66)[_i % 3], _k, _s, act=_i % 3, x_ld=8 if _wide else 4,
                          x_off=4 if _wide and _i % 4 == 1 else 0, why="SMALLC: %d input channel(s), x_ld %d" % (_cin, 8 if _wide else 4)))
IGEMM_CASES += _epilogue_cases("a_epi", 3, 5, 5, 32, 1, 1)

# ---- B. conv_patch_f32: forced tiles 5-7, and tile 0 on the 3x3 cases (the heuristic picks 6 or 7 there)
PATCH_CASES = [
    _c("b_13x13", 2, 13, 13, 64, 128, 3, 1, res=True, why="two chunks (an even pair); tiles straddle the two images"),
    _c("b_7x9", 3, 7, 9, 96, 66, 3, 1, act=2, why="three chunks (an odd tail); cout 66: two n tiles at BN 64, scalar epilogue"),
    _c("b_1x40", 1, 1, 40, 32, 136, 3, 1, why="H = 1: every tile row is its own image; cout 136 = 128 + 8; one chunk"),
    _c("b_5x1", 2, 5, 1, 64, 24, 3, 1, act=0, why="W = 1: TW = 1, PC = 3"),
    _c("b_7x1x1", 7, 1, 1, 32, 64, 3, 1, act=0, why="seven 1 x 1 images in one tile: + 2 patch rows per image"),
    _c("b_5x2x3", 5, 2, 3, 96, 128, 3, 1, why="a tile crossing all five images"),
    _c("b_3x127", 2, 3, 127, 32, 64, 3, 1, why="W = 127 > 126, the widest TW"),
    _c("b_20x20", 1, 20, 20, 32, 64, 3, 1, res=True, why="32 x 4 tiles: a patch of 256 pixels, five tiles across"),
    _c("b_52x52", 1, 52, 52, 32, 24, 3, 1, why="more than 8 blocks, nblocks % 8 != 0: the XCD remap with q > 0"),
    _c("b1_m25_head255", 1, 5, 5, 32, 255, 1, 1, act=0, out=OUT_HEAD, why="1x1, M = 25, head layout (nc5 = 85)"),
    _c("b1_m129", 1, 3, 43, 96, 136, 1, 1, act=2, why="1x1, M = 129: a second tile of one pixel; three chunks"),
    _c("b1_m338", 2, 13, 13, 64, 66, 1, 1, res=True, why="1x1, M = 338: three tiles, the last ragged; two chunks"),
]
PATCH_CASES += _epilogue_cases("b_epi", 3, 7, 9, 32, 3, 1)

# ---- D. the shared epilogue under YOLO_FLAG_SPLIT_BF16 (tile 0) and YOLO_FLAG_SPLIT_K: one odd NHWC view, one odd upsample view
FLAGGED_CASES = [
    _c("d_nhwc_odd", 3, 7, 9, 96, 64, 3, 1, act=1, res=True, y_pad=6, y_off=2, r_pad=4, r_off=1, why="NHWC, y_off 2, r_off 1"),
    _c("d_up_odd", 2, 5, 5, 64, 64, 1, 1, act=2, out=OUT_UP, y_pad=6, y_off=2, why="2x upsampling store, y_off 2"),
]

# ---- E. stem3x3_f32: (N, H, W); 256 pixels per block, 64 per wave
STEM_SHAPES = [(1, 1, 1), (1, 1, 70), (2, 5, 3), (1, 16, 16), (3, 37, 45)]
STEM_LAYOUTS = [(32, 0), (48, 16)]               # y_ld == 32: the LDS-transposed store; else the direct one


def stem_case(shape, layout, act):
    n, h, w = shape
    return dict(name="e_%dx%dx%d_ld%d_act%d" % (n, h, w, layout[0], act), n=n, h=h, w=w, cin=3, cout=32, k=3, s=1, act=act, res=False,
                out=OUT_NHWC, x_ld=0, x_off=0, y_ld=layout[0], y_off=layout[1], r_ld=0, r_off=0, stem=True, why="")


STEM_CASES = [stem_case(sh, lay, act) for sh in STEM_SHAPES for lay in STEM_LAYOUTS for act in (0, 1, 2)]
ALL_CASES = {c["name"]: c for c in IGEMM_CASES + PATCH_CASES + FLAGGED_CASES + STEM_CASES}
assert len(ALL_CASES) == len(IGEMM_CASES) + len(PATCH_CASES) + len(FLAGGED_CASES) + len(STEM_CASES)


# ================================================================================================ data and reference
def out_hw(c):
    k, s = c["k"], c["s"]
    return (c["h"] + 2 * (k // 2) - k) // s + 1, (c["w"] + 2 * (k // 2) - k) // s + 1


def _key(c):
    return tuple((k, v) for k, v in sorted(c.items()) if k not in ("why", "name"))


def operands(c):
    """(x, w, scale, shift, r) on the host, seeded from the case tuple. x is the whole buffer (n, h, w, x_ld), every channel
    outside the view random too; a cin <= 4 view holds zeros in its pad channels, as the ABI states. The stem's x is NCHW."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(_key(c)).encode()))
    k, cin, cout = c["k"], c["cin"], c["cout"]
    ho, wo = out_hw(c)
    if c.get("stem"):
        x = torch.randn((c["n"], 3, c["h"], c["w"]), generator=g)
    else:
        x = torch.randn((c["n"], c["h"], c["w"], c["x_ld"]), generator=g)
        cp = (cin + 3) // 4 * 4
        x[..., c["x_off"] + cin:c["x_off"] + cp] = 0.0
    w = torch.randn((cout, cin, k, k), generator=g) * (1.0 / (k * k * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    r = torch.randn((c["n"], ho, wo, c["r_ld"]), generator=g) if c["res"] else None
    return x, w, scale, shift, r


def x_view_nchw(c, x):
    """The logical input (n, cin, h, w) of any dtype."""
    if c.get("stem"):
        return x
    return x[..., c["x_off"]:c["x_off"] + c["cin"]].permute(0, 3, 1, 2)


def conv64(c, xv, w):
    """fp64 convolution of an NCHW input, as (n, ho, wo, cout)."""
    return F.conv2d(xv.double(), w.double(), stride=c["s"], padding=c["k"] // 2).permute(0, 2, 3, 1)


def epilogue64(c, z, scale, shift, r):
    """[r +] act(scale * z + shift) in fp64 from the fp32 operands."""
    v = R.act_ref(z * scale.double() + shift.double(), c["act"])
    if r is not None:
        v = v + r[..., c["r_off"]:c["r_off"] + c["cout"]].double()
    return v


def bound_of(c, ops, ref):
    x, w, scale, shift, _ = ops
    K = c["k"] * c["k"] * c["cin"]
    S = conv64(c, x_view_nchw(c, x).abs(), w.abs())
    lip = 1.1 if c["act"] == R.ACT_MISH else 1.0
    b = 2.0 * ((K + 4) * U * (S * scale.double().abs() + shift.double().abs()) * lip + 2.0 * U * ref.abs())
    if c["act"] == R.ACT_MISH:
        b = b + eps_mish() * ref.abs()
    return b


@functools.lru_cache(maxsize=None)
def shared(name):
    """(case, operands, fp64 reference (n, ho, wo, cout), per-element bound): computed once, never modified."""
    c = ALL_CASES[name]
    ops = operands(c)
    x, w, scale, shift, r = ops
    ref = epilogue64(c, conv64(c, x_view_nchw(c, x), w), scale, shift, r)
    return c, ops, ref, bound_of(c, ops, ref)


def torch_fp32(c, ops):
    """torch's own fp32 CPU convolution with the same epilogue in fp32."""
    x, w, scale, shift, r = ops
    z = F.conv2d(x_view_nchw(c, x).contiguous(), w, stride=c["s"], padding=c["k"] // 2).permute(0, 2, 3, 1) * scale + shift
    if c["act"] == R.ACT_LEAKY:
        z = torch.where(z > 0, z, z * np.float32(R.LEAKY_SLOPE))
    elif c["act"] == R.ACT_MISH:
        z = F.mish(z)
    if r is not None:
        z = z + r[..., c["r_off"]:c["r_off"] + c["cout"]]
    return z


def _taps_of_pixel(c, xv, n, ho, wo):
    """(k*k, cin) fp64: what each tap of output pixel (n, ho, wo) reads, zeros where it is padding."""
    k, s, pad = c["k"], c["s"], c["k"] // 2
    t = torch.zeros((k * k, c["cin"]), dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            hi, wi = ho * s - pad + kh, wo * s - pad + kw
            if 0 <= hi < c["h"] and 0 <= wi < c["w"]:
                t[kh * k + kw] = xv[n, :, hi, wi].double()
    return t


def mutants(c, ops):
    """Three subtly wrong results, each as (label, fp64 output):
    tap   one border tap of one output pixel (the last pixel of image 0) reads what the next output pixel's same tap reads (the
          previous pixel's where there is no next; nothing where the output is a single pixel). The tap is the first border
          tap whose two reads differ; on a map where every border tap is padding for both, the centre tap.
    w0    one weight (last output channel, last input channel, centre tap) is zero.
    x4    x is read 4 elements further on in memory (x_off + 4; into the next pixel where the row ends, zeros past the end)."""
    x, w, scale, shift, r = ops
    xv = x_view_nchw(c, x)
    z = conv64(c, xv, w)
    k, cin, cout = c["k"], c["cin"], c["cout"]
    ho, wo = out_hw(c)
    # ---- tap
    m = ho * wo - 1
    total = c["n"] * ho * wo
    other = m + 1 if m + 1 < total else m - 1
    mine = _taps_of_pixel(c, xv, 0, m // wo, m % wo)
    theirs = torch.zeros_like(mine)
    if other >= 0:
        theirs = _taps_of_pixel(c, xv, other // (ho * wo), other % (ho * wo) // wo, other % wo)
    centre = (k // 2) * k + k // 2
    order = [t for t in range(k * k) if t != centre] + [centre]
    tap = next(t for t in order if not torch.equal(mine[t], theirs[t]))
    z_tap = z.clone()
    z_tap[0, m // wo, m % wo] += w.double().reshape(cout, cin, k * k)[:, :, tap] @ (theirs[tap] - mine[tap])
    # ---- w0
    w0 = w.clone()
    w0[cout - 1, cin - 1, k // 2, k // 2] = 0.0
    z_w0 = conv64(c, xv, w0)
    # ---- x4
    flat = torch.cat([x.reshape(-1), torch.zeros(4)])[4:]
    z_x4 = conv64(c, x_view_nchw(c, flat.reshape(x.shape)), w)
    return [(lab, epilogue64(c, zz, scale, shift, r)) for lab, zz in (("tap", z_tap), ("w0", z_w0), ("x4", z_x4))]


# ================================================================================================ conv_patch_f32 geometry
def _ceil_div(a, b):
    return (a + b - 1) // b


def _round_up(a, b):
    return _ceil_div(a, b) * b


def pick_patch_tile(H, W, ks):
    """(TH, TW, prmax) of pick_patch_tile in conv_f32_v2.hip: at most 128 pixels, the patch within V2_PATCH_CAP, the most useful
    MFMA rows."""
    if ks == 1:
        return 1, 128, 1
    best, th, tw, prmax = -1.0, 1, 1, 5
    for TW in range(1, min(W, 126) + 1):
        TH = 128 // TW
        while TH >= 1:
            cross = (TH + H - 1) // H
            if (TH + 2 + 2 * cross) * (TW + 2) <= V2_PATCH_CAP:
                break
            TH -= 1
        if TH < 1:
            continue
        eff = (float(W) / (_ceil_div(W, TW) * TW)) * (TH * TW / 128.0)
        if eff > best + 1e-9:
            best, th, tw, prmax = eff, TH, TW, TH + 2 + 2 * ((TH + H - 1) // H)
    return th, tw, prmax


def patch_plan(n, h, w, cin, cout, k, tile):
    """The launch numbers of conv_v2_launch for a stride-1 layer on tile 5, 6 or 7."""
    bn, single = (128 if tile == 6 else 64), tile == 7
    if k == 1:
        H, W, rows_total = 1, n * h * w, 1
        TH, TW, prmax = pick_patch_tile(1, W, 1)
        PC = 128
    else:
        H, W, rows_total = h, w, n * h
        TH, TW, prmax = pick_patch_tile(h, w, 3)
        PC = TW + 2
    patch_cap = max(_round_up(prmax * PC, 32), 128)
    if single:
        patch_cap = V2_PATCH_CAP
    assert patch_cap <= V2_PATCH_CAP
    tiles_w, tiles_r, tiles_n = _ceil_div(W, TW), _ceil_div(rows_total, TH), _ceil_div(cout, bn)
    return dict(H=H, W=W, rows_total=rows_total, TH=TH, TW=TW, PC=PC, prmax=prmax, patch_cap=patch_cap, tiles_w=tiles_w, tiles_r=tiles_r,
                tiles_n=tiles_n, nblocks=tiles_n * tiles_w * tiles_r, nchunks=cin // 32, KT=(cin // 32) * k * k, BN=bn, bufmask=0 if single else 1)


def direct_tile(c):
    """pick_direct_tile of conv_dispatch.hip: what tile 0 runs for a case that brings no workspace. (Tile 6 needs 640 blocks of
    128 channels on a 14 .. 26 row map, far beyond the sizes of these tables: every 3x3 stride-1 case here gets tile 7.)"""
    if c["s"] == 1 and c["cin"] % 32 == 0 and c["k"] == 3:
        blocks = patch_plan(c["n"], c["h"], c["w"], c["cin"], c["cout"], 3, 6)["nblocks"]
        return 6 if c["cout"] > 64 and 13 < c["h"] <= 26 and blocks >= 640 else 7
    return 4


def plan_out8(p):
    return [p[key] for key in ("TH", "TW", "PC", "prmax", "patch_cap", "tiles_w", "tiles_r", "nblocks")]


def packed_f32_floats(cout, cin, k):
    """(offset of the fragment-order section, its length) in floats inside the buffer of yolo_pack_weights (YOLO_F32)."""
    cp = _round_up(cin, 4)
    return _round_up(cout, 128) * _round_up(k * k * cp, 32), (_round_up(cout, 128) // 32) * (cin // 32) * k * k * 1024


def remap_block(bid, nblocks):
    """The XCD block remap of conv_patch_f32."""
    q, r, xcd = nblocks // 8, nblocks % 8, bid % 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + bid // 8


def audit_patch(c, tile, packed_floats):
    """Every address conv_patch_f32 forms for case c on `tile`, restated from the kernel text and asserted to lie inside its
    tensor (x, residual, y, scale, the packed weight buffer of `packed_floats` floats) or its LDS buffer. Also asserts that the
    patch a tile stages holds, for every tap of every output pixel of the tile, exactly the input pixel that tap reads (or a
    zero where it is padding), and that the tiles' output pixels partition the output. Returns what the edge assertions of
    the tables need: the largest number of images a tile crosses, and the largest PR."""
    p = patch_plan(c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"], tile)
    KS, H, W, TH, TW, PC, cap = c["k"], p["H"], p["W"], p["TH"], p["TW"], p["PC"], p["patch_cap"]
    BN, TN = p["BN"], p["BN"] // 64
    M = c["n"] * c["h"] * c["w"]
    x_elems = M * c["x_ld"]
    r_elems = M * c["r_ld"]
    ho, wo = c["h"], c["w"]
    y_elems = {OUT_NHWC: M * c["y_ld"], OUT_UP: 4 * M * c["y_ld"], OUT_HEAD: M * c["cout"]}[c["out"]]
    has_res = c["res"]
    vec_ok = c["out"] != OUT_HEAD and c["cout"] % 4 == 0 and (c["y_ld"] | c["y_off"]) & 3 == 0 and (not has_res or (c["r_ld"] | c["r_off"]) & 3 == 0)
    lds_floats = cap * V2_LD                                        # per buffer
    tid = np.arange(256)
    lane, wave = tid & 63, tid >> 6
    wm, wn, fh, frow = wave >> 1, wave & 1, lane >> 5, lane & 31
    Hp = H + 2

    def vrow(g):
        return g + 2 * (g // H) if KS == 3 else g

    seen = np.zeros(M, dtype=np.int64)
    stats = dict(max_cross=0, max_PR=0)
    assert sorted(remap_block(b, p["nblocks"]) for b in range(p["nblocks"])) == list(range(p["nblocks"])), "the block remap is a bijection"
    for sp in range(p["tiles_w"] * p["tiles_r"]):
        w_tile, r_tile = sp % p["tiles_w"], sp // p["tiles_w"]
        g0, c0 = r_tile * TH, w_tile * TW
        g_last = min(g0 + TH, p["rows_total"]) - 1
        v0 = vrow(g0)
        PR = vrow(g_last) + (3 if KS == 3 else 1) - v0
        assert PR <= p["prmax"], (c["name"], tile, sp, PR, p["prmax"])
        assert PR * PC <= cap and PR * PC <= 32 * V2_NI, "the whole patch is staged"
        stats["max_PR"] = max(stats["max_PR"], PR)
        stats["max_cross"] = max(stats["max_cross"], g_last // H - g0 // H + 1)
        # ---- pix[]: the incremental decode of the kernel, beside the direct one
        d_pr = 32 // PC
        d_pc = 32 - d_pr * PC
        pr = (tid >> 3) // PC
        pc = (tid >> 3) - pr * PC
        n0i = v0 // Hp if KS == 3 else 0
        pixmap = np.full(32 * V2_NI, -2, dtype=np.int64)            # patch pixel -> x pixel (-1: zero; -2: not staged)
        for i in range(V2_NI):
            pix = np.full(256, -1, dtype=np.int64)
            live = pr < PR
            if KS == 3:
                nn = np.full(256, n0i)
                yy = v0 + pr - n0i * Hp
                walk = live & (yy >= Hp)
                steps = 0
                while walk.any():                                   # while (yy >= Hp) { yy -= Hp; ++n; }
                    yy = np.where(walk, yy - Hp, yy)
                    nn = np.where(walk, nn + 1, nn)
                    walk = live & (yy >= Hp)
                    steps += 1
                    assert steps <= TH + 1
                hi, wi = yy - 1, c0 + pc - 1
                ok = live & (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
                pix = np.where(ok, (nn * H + hi) * W + wi, -1)
                # direct: virtual row v = v0 + pr -> image v // Hp, input row v % Hp - 1
                v = v0 + pr
                assert np.array_equal(np.where(ok, nn, 0), np.where(ok, v // Hp, 0)) and np.array_equal(np.where(ok, hi, 0), np.where(ok, v % Hp - 1, 0))
                assert (np.where(ok, nn, 0) < c["n"]).all()
            else:
                wi = c0 + pc
                pix = np.where(live & (wi < W), wi, -1)
            assert ((pix >= -1) & (pix < M)).all()
            idx = (tid >> 3) + 32 * i
            assert np.array_equal(np.where(live, pr * PC + pc, idx), idx), "patch pixel idx is (pr, pc)"
            stored = idx < cap
            assert (stored | ~live).all(), "a live patch pixel is not stored"
            pixmap[idx[stored]] = pix[stored]
            # global loads: the prologue's (pix >= 0 only) and the prefetch's (clamped to pixel 0), chunks 0 .. nchunks - 1
            px = np.maximum(pix, 0)
            top = px * c["x_ld"] + c["x_off"] + (p["nchunks"] - 1) * 32 + (tid & 7) * 4 + 3
            assert (top < x_elems).all() and (px * c["x_ld"] + c["x_off"] >= 0).all(), (c["name"], "x load outside the tensor")
            # LDS stores of the staged pixel
            dst = (tid >> 3) * V2_LD + (tid & 7) * 4 + 32 * i * V2_LD + 3
            assert (dst[stored] < lds_floats).all()
            pr = pr + d_pr
            pc = pc + d_pc
            wrap = pc >= PC
            pc = np.where(wrap, pc - PC, pc)
            pr = np.where(wrap, pr + 1, pr)
        # ---- a_off and the LDS reads behind it; what the patch holds under every tap of every output pixel
        for i in range(2):
            pp = wm * 64 + i * 32 + frow
            rr, cc = pp // TW, pp % TW
            g = g0 + rr
            ok = (pp < TH * TW) & (g <= g_last) & (c0 + cc < W)
            a_off = np.where(ok, ((vrow(g) - v0) * PC + cc) * V2_LD, 0) + 4 * fh
            far = a_off + ((KS - 1) * PC + (KS - 1)) * V2_LD + 3 * 8 + 3
            assert (far < lds_floats).all(), (c["name"], tile, "A fragment read outside the patch buffer")
            for kh in range(KS):
                for kw in range(KS):
                    at = (vrow(g) - v0 + kh) * PC + cc + kw
                    hi, wi = g % H + kh - KS // 2, c0 + cc + kw - KS // 2
                    want = np.where((hi >= 0) & (hi < H) & (wi >= 0) & (wi < W), ((g // H) * H + hi) * W + wi, -1)
                    assert np.array_equal(pixmap[at[ok]], want[ok]), (c["name"], tile, sp, kh, kw, "the patch does not hold the tap's pixel")
        # ---- mtab
        t = np.arange(128)
        rr, cc = t // TW, t % TW
        g = g0 + rr
        mok = (t < TH * TW) & (g <= g_last) & (c0 + cc < W)
        mtab = np.where(mok, g * W + c0 + cc, -1)
        assert ((mtab >= -1) & (mtab < M)).all()
        np.add.at(seen, mtab[mok], 1)
        # ---- per n tile: scale / shift, residual, y, B fragments
        for n_tile in range(p["tiles_n"]):
            for j in range(TN):
                ncol = n_tile * BN + wn * (BN // 2) + j * 32 + frow
                ncl = np.minimum(ncol, c["cout"] - 1)
                assert ((ncl >= 0) & (ncl < c["cout"])).all()
                nt = n_tile * (BN // 32) + wn * TN + j
                base = nt * p["KT"] * 1024 + lane * 4
                ktn = np.minimum(np.arange(p["KT"]) + 1, p["KT"] - 1)      # the one-step-ahead prefetch, clamped; step 0 in the prologue
                for kt in set(ktn.tolist()) | {0}:
                    assert (packed_floats[0] + base + (kt * 4 + 3) * 256 + 3 < packed_floats[0] + packed_floats[1]).all(), "B load outside the fragment section"
                    assert (packed_floats[0] + base + (kt * 4 + 3) * 256 + 3 < packed_floats[2]).all(), "B load outside the packed buffer"
                if vec_ok:
                    c4 = tid & 15
                    ncol4 = n_tile * BN + (c4 >> 3) * (BN // 2) + j * 32 + (c4 & 7) * 4
                    for it in range(8):
                        mrow = mtab[(tid >> 4) + 16 * it]
                        if has_res:
                            ridx = np.maximum(mrow, 0) * c["r_ld"] + c["r_off"] + np.where(ncol4 < c["cout"], ncol4, 0)
                            assert (ridx + 3 < r_elems).all() and (ridx % 4 == 0).all(), (c["name"], "residual load outside the tensor or misaligned")
                        st = (mrow >= 0) & (ncol4 < c["cout"])
                        top = _y_index(c, mrow[st], ncol4[st], ho, wo, last=True) + 3
                        assert (top < y_elems).all() and (_y_index(c, mrow[st], ncol4[st], ho, wo) % 4 == 0).all(), (c["name"], "vector store")
                else:
                    for it in range(32):
                        idx = tid + 256 * it
                        row, col = idx >> 6, idx & 63
                        m = mtab[row]
                        nc = n_tile * BN + (col >> 5) * (BN // 2) + j * 32 + (col & 31)
                        st = (m >= 0) & (nc < c["cout"])
                        if has_res:
                            assert (m[st] * c["r_ld"] + c["r_off"] + nc[st] < r_elems).all()
                        assert (_y_index(c, m[st], nc[st], ho, wo, last=True) < y_elems).all(), (c["name"], "scalar store")
    assert (seen == 1).all(), (c["name"], tile, "the tiles do not partition the output pixels")
    # the epilogue's staging tile [128][68] floats lies in the patch region
    assert 128 * 68 <= (p["bufmask"] + 1) * lds_floats
    return p, stats


def _y_index(c, m, ncol, ho, wo, last=False):
    """Element index of output pixel m, channel ncol in y (`last`: the last of the four pixels a 2x upsampling store writes)."""
    if c["out"] == OUT_NHWC:
        return m * c["y_ld"] + c["y_off"] + ncol
    img, rem = m // (ho * wo), m % (ho * wo)
    hh, ww = rem // wo, rem % wo
    if c["out"] == OUT_UP:
        W2 = 2 * wo
        d = ((img * 2 * ho + 2 * hh) * W2 + 2 * ww) * c["y_ld"] + c["y_off"] + ncol
        return d + (W2 + 1) * c["y_ld"] if last else d
    nc5 = c["cout"] // 3
    return (((img * 3 + ncol // nc5) * ho + hh) * wo + ww) * nc5 + ncol % nc5
