"""Cases, fp64 reference, bounds and host-side restatements for the two fp32 kernel families that tests/conv_f32_cases.py leaves
out: conv1_rs_f32 (tile 12, conv1_rs_f32.hip: 1x1 with the weights in registers) and Winograd F(2x2, 3x3) (tiles 13 / 14,
conv_wino_f32.hip: wino_pack_f32, wino_xform_f32, conv_wino_f32 / conv_wino2_f32), the latter also as the fp32 input gradient on
the filters of yolo_pack_weights_dgrad(flip = 1). Shared by tests/test_conv_wino_rs_cases_host.py (CPU) and
tests/test_gpu_conv_wino_rs_edges.py. No project code is used by the reference: plain torch on the CPU.

Two kinds of case.

INTEGER cases (every geometry case). x and the residual lie in +-{1..xmax}, the weights are integers in [-wmax, wmax], scale in
{0.5, 1, 2}, shift an integer, the activation none or LeakyReLU. The expected result is the fp64 reference BIT FOR BIT, with the
two epilogue roundings that are no matter of order (LeakyReLU's product with 0.1f, the residual add: `kernel_steps=True` of
tests/conv_h16_ref.py). For the 1x1 kernel every partial sum is an integer below 2^24. For F(2x2):

    Y = A^T [ (G g G^T) .* (B^T d B) ] A,   B^T, A^T hold 0 / +-1,   G holds 0 / +-1/2 / 1

U = G g G^T of an integer g is an exact multiple of 1/4 (wino_pack_f32 forms it in fp64 and rounds once: no rounding happens),
V = B^T d B is an integer, every product U V is a multiple of 1/4 and so is every partial sum over cin and every level of the
output transform. All of them are bounded in magnitude by the same algorithm run on absolute values,

    S^ = |A^T| [ (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A|      summed over cin,

so with 8 S^ < 2^24 (a multiple of 1/8 below 2^21 has 24 significant bits) every fp32 operation of any summation order is exact;
scale and shift keep that (halves, small integers). `exactness_margin` returns that figure per case; the host test proves it.
Signed zeros: no output zero's sign depends on the order. The accumulators start at +0 and x + (-x) = +0, the scale / shift step
ends in `+ shift` with shift either non-zero (then a zero result is an exact cancellation: +0) or +0 ((+-0) + (+0) = +0);
LeakyReLU keeps +0 and a residual is never zero. So everything, zeros included, is compared by bits; the host test asserts the
premises (no shift is -0, every scale is positive, no reference value is -0).

GAUSSIAN cases (a few per kernel, every activation, real scale / shift): a per-element bound. conv1_rs_f32: the bound of
tests/conv_f32_cases.py unchanged, K = cin. F(2x2), with u = 2^-24:

    bound = 2 * [ (cin + 7 + 4) * u * (S^ * |scale| + |shift|) * L + 2u * |ref| ]  [+ eps_mish * |ref|]

Every fp32 quantity of the algorithm is bounded by its part of S^, and each operation adds at most u times its result: cin for the
fmaf chain over the input channels (an f32 MFMA chain), 1 for U's rounding, 2 for the two add levels of B^T d B, 4 for the four
add levels of the output transform (conv_wino_f32: two for A^T M, two for (A^T M) A; conv_wino2_f32: one inside a pass, two for
the columns, one for adding the second pass), and 4, L, 2u |ref|, the outer 2 and eps_mish as in tests/conv_f32_cases.py (scale /
shift multiply-add, activation slope, activation and residual roundings, margin, Mish's formula). For the input gradient cin is
the launch's (the forward cout rounded up to 32).
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_f32_cases as K
from tests import conv_h16_ref as H

U = K.U
OUT_NHWC, OUT_UP = K.OUT_NHWC, K.OUT_UP
TILE_REG64, TILE_RS, TILE_WINO, TILE_WINO2, TILE_WINO4 = 4, 12, 13, 14, 15
WINO2_MAXPIX = 256                        # the unset value of YOLO_WINO2_MAXPIX


def _c(name, n, h, w, cin, cout, k, kind="int", act=1, res=False, out=OUT_NHWC, x_pad=0, x_off=0, y_pad=0, y_off=0, r_pad=0, r_off=0,
       xmax=8, wmax=1, fco=None, why=""):
    """One launch. An input-gradient case (fco: the forward layer's cout) is the launch it makes: cin = fco rounded up to 32 (the
    channels of dz), cout = the forward cin, weights (fco, cout, 3, 3) packed by yolo_pack_weights_dgrad(flip = 1), klim = fco."""
    assert fco is None or cin == (fco + 31) // 32 * 32
    return dict(name=name, kind=kind, n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=1, act=act, res=res, out=out, x_ld=cin + x_pad, x_off=x_off,
                y_ld=cout + y_pad, y_off=y_off, r_ld=(cout + r_pad) if res else 0, r_off=r_off if res else 0, xmax=xmax, wmax=wmax,
                klim=cin if fco is None else fco, dgrad=fco is not None, why=why)


# ---- R. conv1_rs_f32: K 256 / 384 / 512, cout a multiple of 128; tiles of 32 pixels, per = min(256 / ngroups, tiles) workgroups per
# channel group, workgroup f takes tiles f, f + per, ...; a ring of 3 slots (K <= 384) or 2 (K = 512), SLOTS - 1 tiles requested ahead
RS_CASES = [
    _c("r_m1", 1, 1, 1, 256, 128, 1, act=0, why="M = 1: every request of the only tile clamps to pixel 0; one workgroup, look-ahead from the zero page"),
    _c("r_m31", 1, 1, 31, 384, 128, 1, res=True, why="M = 31 < 32: the last row of the tile repeats pixel 30; K = 384"),
    _c("r_m32", 1, 4, 8, 512, 128, 1, act=0, res=True, why="M = 32: exactly one full tile; K = 512 (two slots)"),
    _c("r_m33", 1, 3, 11, 256, 128, 1, why="M = 33: a second tile of one pixel, 31 clamped rows; fewer tiles than `per`: one tile per workgroup"),
    _c("r_groups2", 3, 5, 5, 256, 256, 1, act=0, res=True, why="cout 256: two channel groups; 3 tiles < per: all look-ahead from the zero page; batch of 3"),
    _c("r_groups3", 2, 5, 7, 384, 384, 1, why="cout 384: three channel groups (per = 85), K = 384"),
    _c("r_up_13x13", 2, 13, 13, 256, 128, 1, out=OUT_UP, y_pad=256, y_off=128, why="tiles straddle the two 13 x 13 images; 2x upsampling store into a concat buffer"),
    _c("r_views4", 3, 3, 5, 256, 128, 1, res=True, x_pad=4, x_off=4, y_pad=12, y_off=4, r_pad=4, r_off=4,
       why="x_ld K + 4, x_off 4, y_off 4, r_off 4: multiples of 4 that are none of 8"),
    _c("r_per256_t257", 1, 7, 1171, 256, 128, 1, act=0, why="cout 128, per = 256, 257 tiles (8197 pixels): workgroup 0 gets a second, ragged tile"),
]
# cout 1024: 8 groups, per = 32; tiles = 32 s (s tiles per workgroup) and 32 s + 1 (workgroup 0 one more; the last tile ragged):
# s = slots and slots + 1
for _k, _ss in ((256, (3, 4)), (384, (3, 4)), (512, (2, 3))):
    for _s in _ss:
        RS_CASES.append(_c(f"r_wrap_k{_k}_t{32 * _s}", 1, 32, 32 * _s, _k, 1024, 1, act=_s % 2, xmax=4,
                           why=f"K = {_k}: {_s} tiles per workgroup on a ring of {3 if _k <= 384 else 2} slots"))
        RS_CASES.append(_c(f"r_wrap_k{_k}_t{32 * _s + 1}", 1, 1, 1024 * _s + 5, _k, 1024, 1, act=(_s + 1) % 2, res=_k == 512, xmax=4,
                           why=f"K = {_k}: workgroup 0 gets {_s + 1} tiles, the others {_s}; the last tile holds 5 pixels"))
# where tile 0 lands
RS_ROUTE_CASES = [
    _c("r_route_2048", 1, 1, 2048, 256, 128, 1, why="1 x 2048, cin 256, no residual: the heuristic's first map; tile 0 must equal tile 12"),
    _c("r_route_2047", 1, 1, 2047, 256, 128, 1, why="1 x 2047: one pixel short; tile 0 must equal tile 4"),
    _c("r_route_res", 1, 1, 2048, 256, 128, 1, res=True, why="1 x 2048 with a residual: tile 0 must equal tile 4"),
]
# The same three on real values. On the integer cases every tile stores the reference's bits, so comparing tiles there cannot tell
# one kernel from another; here conv_igemm_f32 (tile 4) and conv1_rs_f32 (tile 12) add in different orders and differ in bits.
RS_ROUTE_GAUSS = [dict(_rc, name="rg" + _rc["name"][1:], kind="gauss", why=_rc["why"] + " (real values: tiles 4 and 12 differ in bits)")
                  for _rc in RS_ROUTE_CASES]
RS_REFUSED = [
    _c("r_yoff2", 2, 5, 5, 256, 128, 1, y_pad=6, y_off=2, why="y_off 2: tile 12 refuses and writes nothing, tile 0 stores the reference"),
]
RS_GAUSS = [
    _c("rg_none_res", 3, 5, 5, 256, 128, 1, kind="gauss", act=0, res=True, why="M = 75 ragged, K = 256, no activation + residual; batch of 3"),
    _c("rg_leaky_res", 2, 5, 7, 384, 256, 1, kind="gauss", act=1, res=True, r_pad=4, r_off=4, why="K = 384, LeakyReLU + residual view; two groups; M = 70"),
    _c("rg_mish_res", 3, 3, 5, 512, 128, 1, kind="gauss", act=2, res=True, why="K = 512, Mish + residual"),
    _c("rg_mish_wrap", 1, 1, 3077, 256, 1024, 1, kind="gauss", act=2, why="97 tiles on 32 workgroups per group: the ring wraps on real values"),
    _c("rg_up", 2, 13, 13, 256, 128, 1, kind="gauss", act=1, out=OUT_UP, y_pad=128, y_off=128, why="upsampling store on real values"),
]

# ---- W. F(2x2): T = n ceil(h / 2) ceil(w / 2) tiles, blocks of 64 tiles x 64 channels; n_mt = ceil(T / 64) tile blocks over eight XCD
# lanes (grid = 8 n_nt ceil(n_mt / 8): lanes with mt >= n_mt leave), n_nt = ceil(cout / 64), cin / 4 ring stages, the transform in
# channel groups of 32
WINO_CASES = [
    _c("w_1x1", 3, 1, 1, 32, 64, 3, why="1 x 1 maps: T = 3, one pixel of each tile is written, eight of nine taps are padding; three images in one block"),
    _c("w_1x9", 13, 1, 9, 4, 4, 3, act=0, why="1 x 9: T = 65 (a second block of one tile); cin 4 (one stage, one lane of eight in the transform), cout 4"),
    _c("w_9x1", 2, 9, 1, 96, 60, 3, res=True, why="9 x 1; cin 96 (24 stages: six turns of the ring); cout 60 (one ragged channel block)"),
    _c("w_2x2", 3, 2, 2, 32, 68, 3, act=0, res=True, why="2 x 2: whole tiles, T = 3; cout 68: n_nt 2, the second holds one run"),
    _c("w_3x3_t64", 16, 3, 3, 32, 64, 3, why="3 x 3: T = 64 = exactly one block over 16 images; odd rows and columns"),
    _c("w_5x5_t63", 7, 5, 5, 32, 4, 3, act=0, why="T = 63: one tile short of a block; cout 4"),
    _c("w_4x5", 3, 4, 5, 160, 132, 3, res=True, why="4 x 5: even rows, odd columns; cin 160 (five channel groups in the transform), cout 132 (n_nt 3, last ragged)"),
    _c("w_13x13", 3, 13, 13, 64, 64, 3, res=True, why="13 x 13: T = 147, blocks straddle images; tile 0 with the workspace is tile 14"),
    _c("w_20x20", 1, 20, 20, 64, 64, 3, act=0, why="20 x 20 > wino2_maxpix and below F(4x4)'s 26 x 26: tile 0 with the workspace is tile 13"),
    _c("w_t512", 8, 16, 16, 32, 64, 3, why="T = 512: n_mt = 8, every lane of the block map has one tile block"),
    _c("w_46x46", 1, 46, 46, 32, 64, 3, act=0, why="one 46 x 46 image: T = 529, n_mt = 9: a second round in which seven lanes leave"),
    _c("w_views4", 3, 3, 5, 32, 68, 3, res=True, x_pad=4, x_off=4, y_pad=12, y_off=4, r_pad=8, r_off=4, why="x, y and residual views: multiples of 4, r_off 4"),
    _c("w_layer_13x13", 1, 13, 13, 512, 1024, 3, why="a real layer: 13 x 13, 512 -> 1024, n = 1 (128 stages, n_nt 16)"),
]
WINO_REFUSED = [
    _c("w_yoff2", 2, 5, 5, 64, 64, 3, y_pad=6, y_off=2, why="y_off 2: tile 13 refuses and writes nothing; tile 0 runs the direct kernel"),
]
WINO_GAUSS = [
    _c("wg_none", 1, 5, 6, 32, 132, 3, kind="gauss", act=0, res=True, why="no activation + residual, real scale / shift; n_nt 3"),
    _c("wg_leaky_res", 3, 13, 13, 64, 64, 3, kind="gauss", act=1, res=True, why="LeakyReLU + residual; tile 0 lands here; batch of 3"),
    _c("wg_mish_res", 3, 7, 9, 96, 68, 3, kind="gauss", act=2, res=True, r_pad=4, r_off=4, why="Mish + residual view; odd map"),
    _c("wg_20x20", 1, 20, 20, 64, 64, 3, kind="gauss", act=1, why="20 x 20 on real values, where tiles 13 and 14 differ in bits: tile 0 with the workspace is tile 13"),
]
# ---- G. the input gradient: dx = conv(dz, g'), g'[ci][co][p][q] = w[co][ci][2 - p][2 - q]; filter columns kk >= klim are zero
DGRAD_CASES = [
    _c("g_co84_ci64", 2, 6, 7, 96, 64, 3, act=0, fco=84, why="forward cout 84 (dz padded to 96: 12 garbage channels), forward cin 64"),
    _c("g_co33_ci96_acc", 3, 5, 5, 64, 96, 3, act=0, res=True, fco=33, why="forward cout 33 (padded to 64: 31 garbage channels), cin 96; accumulates into dx"),
    _c("gg_co84_ci96_acc", 2, 6, 6, 96, 96, 3, kind="gauss", act=0, res=True, fco=84, why="real values; accumulates into dx"),
]

FAMILIES = dict(R=RS_CASES + RS_ROUTE_CASES + RS_ROUTE_GAUSS + RS_GAUSS, W=WINO_CASES + WINO_GAUSS, G=DGRAD_CASES, X=RS_REFUSED + WINO_REFUSED)
ALL_CASES = {c["name"]: c for fam in FAMILIES.values() for c in fam}
assert len(ALL_CASES) == sum(len(f) for f in FAMILIES.values())


def names(cases):
    return [c["name"] for c in cases]


# ================================================================================================ geometry, restated from the launch code
def _ceil_div(a, b):
    return (a + b - 1) // b


def rs_geometry(c):
    """conv1_rs_launch and the tile walk of conv1_rs_f32."""
    M = c["n"] * c["h"] * c["w"]
    ngroups, tiles = _ceil_div(c["cout"], 128), _ceil_div(M, 32)
    per = min(max(256 // ngroups, 1), tiles)
    counts = [_ceil_div(tiles - f, per) for f in range(per)]           # tiles of workgroup `first` = f
    slots = 3 if c["cin"] <= 384 else 2
    # look-ahead requests beyond the last tile (tile >= tiles: the zero page), per workgroup: the prologue's and the loop's
    zero_page = [sum(1 for i in range(counts[f] + slots - 1) if f + i * per >= tiles) for f in range(per)]
    return dict(M=M, tiles=tiles, ngroups=ngroups, per=per, grid=per * ngroups, counts=counts, slots=slots, zero_page=zero_page,
                extra=[f for f in range(per) if counts[f] > min(counts)], last_pixels=M - 32 * (tiles - 1))


def wino_geometry(c):
    """conv_wino_launch."""
    th, tw = (c["h"] + 1) // 2, (c["w"] + 1) // 2
    T = c["n"] * th * tw
    n_mt, n_nt = _ceil_div(T, 64), _ceil_div(c["cout"], 64)
    grid = 8 * n_nt * _ceil_div(n_mt, 8)
    leaving = sum(1 for b in range(grid) if ((b >> 3) // n_nt) * 8 + (b & 7) >= n_mt)
    blocks_images = [len({t // (th * tw) for t in range(mt * 64, min(mt * 64 + 64, T))}) for mt in range(n_mt)]
    return dict(th=th, tw=tw, T=T, Tpad=64 * n_mt, n_mt=n_mt, n_nt=n_nt, stages=c["cin"] // 4, cgroups=_ceil_div(c["cin"] // 4, 8), grid=grid,
                leaving=leaving, rounds=_ceil_div(n_mt, 8), max_images_per_block=max(blocks_images),
                workspace_bytes=64 * n_mt * c["cin"] * 16 * 4)


def _views4(c):
    v = (c["x_ld"] | c["x_off"] | c["y_ld"] | c["y_off"]) & 3 == 0
    return v and (not c["res"] or (c["r_ld"] | c["r_off"]) & 3 == 0)


def tile0_lands(c, wino2_maxpix=WINO2_MAXPIX):
    """The tile id whose kernel runs a case at tile 0 when the caller brings the workspace yolo_conv_workspace_bytes asks for
    (f32_route of conv_dispatch.hip with no A/B switch set; no case here carries YOLO_FLAG_FILTERS_APPENDED)."""
    area = c["h"] * c["w"]
    if c["k"] == 1:
        rs = c["cin"] in (256, 384) and c["cout"] % 128 == 0 and area >= 2048 and not c["res"] and _views4(c) and c["out"] != 2
        return TILE_RS if rs else TILE_REG64
    if c["out"] == OUT_NHWC and c["cin"] % 4 == 0 and c["cout"] % 4 == 0 and _views4(c) and c["cin"] >= 64 and c["cout"] >= 64:
        padded = 16 * ((c["h"] + 3) // 4) * ((c["w"] + 3) // 4)
        if area >= 26 * 26 and 5 * padded <= 6 * area:
            return TILE_WINO4
        return TILE_WINO2 if area <= wino2_maxpix else TILE_WINO
    return K.direct_tile(c)


# ================================================================================================ data
def _key(c):
    return tuple((k, v) for k, v in sorted(c.items()) if k not in ("why", "name"))


def operands(c, garbage=0):
    """dict x, w, scale, shift, r (+ w_mem for the input gradient), seeded from the case. x and r are whole buffers of their ld, every
    channel outside the view filled like the view. w is the LOGICAL filter (cout, klim, k, k) of the launch's convolution. Input
    gradient: w_mem is what lies at the weight pointer, the forward weights (klim, cout, 3, 3) followed by as many floats again of
    finite non-zero garbage inside the same allocation; the channels [klim, cin) of x (dz) hold finite non-zero garbage too.
    `garbage` reseeds both and nothing else."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(_key(c)).encode()))
    gg = torch.Generator().manual_seed(zlib.crc32(repr((_key(c), "garbage", garbage)).encode()))
    n, h, w_, k, cin, cout, klim = c["n"], c["h"], c["w"], c["k"], c["cin"], c["cout"], c["klim"]
    wshape = (klim, cout, 3, 3) if c["dgrad"] else (cout, cin, k, k)
    if c["kind"] == "gauss":
        x = torch.randn((n, h, w_, c["x_ld"]), generator=g)
        wt = torch.randn(wshape, generator=g) * (1.0 / (k * k * klim)) ** 0.5
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        r = torch.randn((n, h, w_, c["r_ld"]), generator=g) if c["res"] else None
        junk = lambda shape: torch.randn(shape, generator=gg) + 3.0 * torch.sign(torch.randn(shape, generator=gg))
    else:
        x = H.ints((n, h, w_, c["x_ld"]), g, c["xmax"])
        wt = torch.randint(-c["wmax"], c["wmax"] + 1, wshape, generator=g).float()
        scale = torch.tensor([1.0, 2.0, 0.5])[torch.randint(0, 3, (cout,), generator=g)]
        shift = torch.randint(-16, 17, (cout,), generator=g).float()
        r = H.ints((n, h, w_, c["r_ld"]), g, c["xmax"]) if c["res"] else None
        junk = lambda shape: H.ints(shape, gg, c["xmax"])
    ops = dict(x=x, scale=scale, shift=shift, r=r)
    if c["dgrad"]:
        ops["scale"], ops["shift"] = torch.ones(cout), torch.zeros(cout)          # a gradient: identity epilogue
        x[..., klim:cin] = junk((n, h, w_, cin - klim))
        assert bool((x[..., klim:cin] != 0).all())
        ops["w_mem"] = torch.cat([wt.reshape(-1), junk((wt.numel(),))])
        ops["w"] = dgrad_filters(c, ops["w_mem"], klim)[:, :klim].contiguous()
    else:
        ops["w"] = wt
    return ops


def dgrad_filters(c, w_mem, limit):
    """(cout, cin, 3, 3): the filters wino_pack_f32 forms in its dgrad mode with `klim` = limit, read from the floats at the weight
    pointer: column kk of row co is w_mem[(kk * cout + co) * 9 ..] flipped, zero for kk >= limit."""
    cin, cout = c["cin"], c["cout"]
    g = w_mem[:cin * cout * 9].reshape(cin, cout, 3, 3).flip(2, 3).transpose(0, 1).clone()
    g[:, limit:] = 0.0
    return g


def x_view(c, x, channels=None):
    """the logical input (n, channels, h, w): the klim real channels unless told otherwise"""
    ch = c["klim"] if channels is None else channels
    return x[..., c["x_off"]:c["x_off"] + ch].permute(0, 3, 1, 2)


def _res(c, r):
    return None if r is None else r[..., c["r_off"]:c["r_off"] + c["cout"]]


def reference(c, ops):
    """fp64, (n, h, w, cout). Integer cases: with the epilogue's two fp32 roundings; the result is an fp32 value."""
    z = F.conv2d(x_view(c, ops["x"]).double(), ops["w"].double(), padding=c["k"] // 2).permute(0, 2, 3, 1)
    if c["kind"] == "gauss":
        return K.epilogue64(c, z, ops["scale"], ops["shift"], ops["r"])
    v = H.act_ref(z * ops["scale"].double() + ops["shift"].double(), c["act"], kernel_steps=True)
    if ops["r"] is not None:
        v = (v + _res(c, ops["r"]).double()).float().double()
    return v


# ================================================================================================ F(2x2), restated in plain torch
G_MAT = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def input_tiles(c, xv):
    """(n, C, th, tw, 4, 4): the 4x4 input tile of every 2x2 output tile (stride 2, zero padding 1)"""
    h, w = c["h"], c["w"]
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = F.pad(xv, (1, 2 * tw + 1 - w, 1, 2 * th + 1 - h))
    return xp.unfold(2, 4, 2).unfold(3, 4, 2).contiguous()


def _bt(d, dim, absolute):
    """B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1] along `dim`"""
    d0, d1, d2, d3 = d.unbind(dim)
    rows = [d0 + d2, d1 + d2, d2 + d1, d1 + d3] if absolute else [d0 - d2, d1 + d2, d2 - d1, d1 - d3]
    return torch.stack(rows, dim)


def _at(m, dim, absolute):
    """A^T = [1 1 1 0; 0 1 -1 -1] along `dim`"""
    m0, m1, m2, m3 = m.unbind(dim)
    rows = [m0 + m1 + m2, m1 + m2 + m3] if absolute else [m0 + m1 + m2, m1 - m2 - m3]
    return torch.stack(rows, dim)


def wino_grid(c, d, g, dtype, absolute=False):
    """Y on the whole tile grid, (n, 2 th, 2 tw, cout) in `dtype`, from input tiles d (n, C, th, tw, 4, 4) and filters g (cout, C, 3, 3):
    U = G g G^T in fp64 rounded once to `dtype`, V = B^T d B, a sum over C per transform point, the output transform."""
    gm = G_MAT.abs() if absolute else G_MAT
    gg = g.double().abs() if absolute else g.double()
    u = torch.einsum("ap,ocpq,bq->aboc", gm, gg, gm).to(dtype)
    v = _bt(_bt(d.to(dtype), 4, absolute), 5, absolute)
    m = torch.einsum("abok,nktsab->notsab", u, v)
    y = _at(_at(m, 4, absolute), 5, absolute)                          # (n, o, th, tw, 2, 2)
    n, o, th, tw = y.shape[:4]
    return y.permute(0, 2, 4, 3, 5, 1).reshape(n, 2 * th, 2 * tw, o)


def _act32(v, act):
    if act == H.ACT_LEAKY:
        return torch.maximum(v, v * np.float32(0.1))
    return F.mish(v) if act == H.ACT_MISH else v


VARIANTS = ("tap", "col", "klim")


def has_edge(c, variant):
    """does the case have the edge the wrong variant gets wrong?"""
    if c["k"] != 3:
        return False
    if variant == "col":            # an odd width, and a pixel behind the last column of some row (the stray store lands inside y)
        return c["w"] % 2 == 1 and c["n"] * c["h"] > 1
    if variant.startswith("klim"):
        return c["dgrad"] and c["klim"] < c["cin"]
    return True                     # every map has a border


def fp32_value(c, ops, variant=None):
    """An fp32 evaluation in plain torch of what the kernel family of c computes: torch's convolution for the 1x1 cases, the F(2x2)
    restatement above for the others. `variant` makes F(2x2) subtly wrong:
      tap     one padding tap kept: row -1, column 0 of tile (0, 0) of image 0 holds pixel (0, 0) instead of zero (what the
              transform's clamped load returns when the select behind it is lost)
      col     the last tile column is written for odd W: those stores land on the first pixel of the next row
      klim    the gradient filters' columns kk >= klim are not zeroed (klim-1, klim+1: klim shifted by one)"""
    x, scale, shift, r = ops["x"], ops["scale"], ops["shift"], ops["r"]
    n, h, w, cout = c["n"], c["h"], c["w"], c["cout"]
    if c["k"] == 1:
        assert variant is None
        z = F.conv2d(x_view(c, x).contiguous(), ops["w"]).permute(0, 2, 3, 1)
        v = _act32(z * scale + shift, c["act"])
        return v + _res(c, r) if r is not None else v
    if variant and variant.startswith("klim"):
        limit = {"klim": c["cin"], "klim-1": c["klim"] - 1, "klim+1": c["klim"] + 1}[variant]
        g, xv = dgrad_filters(c, ops["w_mem"], limit), x_view(c, x, c["cin"])
    else:
        g, xv = ops["w"], x_view(c, x)
    d = input_tiles(c, xv)
    if variant == "tap":
        d[0, :, 0, 0, 0, 1] = xv[0, :, 0, 0]
    grid = _act32(wino_grid(c, d, g, torch.float32) * scale + shift, c["act"])
    v = grid[:, :h, :w].contiguous()
    if variant == "col":
        rows = torch.arange(n * h)
        dest = (rows * w + w).clamp(max=n * h * w - 1)                 # pixel w of a row = pixel 0 of the next
        stray = grid[:, :h, w].reshape(n * h, cout)
        inside = rows * w + w < n * h * w
        v.view(-1, cout)[dest[inside]] = stray[inside]
    return v + _res(c, r) if r is not None else v


def s_hat(c, ops):
    """S^ of the module text, (n, h, w, cout) in fp64"""
    d = input_tiles(c, x_view(c, ops["x"]).double().abs())
    return wino_grid(c, d, ops["w"], torch.float64, absolute=True)[:, :c["h"], :c["w"]]


def bound_of(c, ops, ref):
    if c["k"] == 1:
        return K.bound_of(c, (ops["x"], ops["w"], ops["scale"], ops["shift"], ops["r"]), ref)
    lip = 1.1 if c["act"] == H.ACT_MISH else 1.0
    b = 2.0 * ((c["cin"] + 7 + 4) * U * (s_hat(c, ops) * ops["scale"].double().abs() + ops["shift"].double().abs()) * lip + 2.0 * U * ref.abs())
    if c["act"] == H.ACT_MISH:
        b = b + K.eps_mish() * ref.abs()
    return b


def exactness_margin(c, ops):
    """8 * (the largest magnitude any intermediate of an integer case can reach) / 2^24: below 1, every fp32 operation is exact"""
    if c["k"] == 3:
        s = s_hat(c, ops)
    else:
        s = F.conv2d(x_view(c, ops["x"]).double().abs(), ops["w"].double().abs()).permute(0, 2, 3, 1)
    top = s * ops["scale"].double().abs() + ops["shift"].double().abs()
    if ops["r"] is not None:
        top = top + _res(c, ops["r"]).double().abs()
    return 8.0 * float(torch.maximum(s, top).max()) / 2.0 ** 24


@functools.lru_cache(maxsize=None)
def shared(name):
    """(case, operands, reference, bound): computed once, never modified. Integer cases: the reference as the fp32 tensor it is
    exactly, no bound. Gaussian cases: the fp64 reference and the per-element bound."""
    c = ALL_CASES[name]
    ops = operands(c)
    ref = reference(c, ops)
    if c["kind"] == "int":
        assert torch.equal(ref.float().double(), ref), name
        return c, ops, ref.float(), None
    return c, ops, ref, bound_of(c, ops, ref)
