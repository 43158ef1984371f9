"""Case tables of tests/test_gpu_conv_dma_h16.py: the 16-bit kernels that carry the default path, at the edges of their
launch geometry, with the reference and the integer operands of tests/conv_h16_ref.py.

  A  conv1_dma_h16, 1x1 (tile 8)                cin >= 128 and cout >= 128: 128 pixels x 128 channels per block, KT = cin / 32
                                                K steps through a 5-slot ring, four of them peeled; the scale / shift table
                                                parks in ring slot KT % 5
  B  conv1_dma_h16, gathered rows (tile 13)     3x3 stride 2 with cout >= 128 as a GEMM, KT = 9 cin / 32
  C  conv1_dma_h16, gather mode 2               yolo_conv_dgrad_s2 with 32 / 64 dx channels: the four parity classes as one
                                                GEMM over the dz pixels, KT = 4 (dz channels) / 32
  D  conv3_dma_h16 (tiles 8 and 10)             3x3 stride 1 with more than 64 output channels
  E  conv3_ws_h16 (tile 14)                     3x3 with at most 64 channels: min(tiles, 512) persistent workgroups walk
                                                8 x 16-pixel tiles, alternating two patch buffers

The routing rules of conv_h16.hip are restated below (dma_ok, dma1_ok, s2_ok, ws_eligible, s2g_ok);
tests/test_conv_dma_h16_ref_host.py proves that every case lands where its table says, that the edges a comment names
really occur, and for every case what the GPU test relies on when it asks for bit equality (see conv_h16_ref.py). xmax
is chosen per case so that the reference alone meets the sharpness condition of that test: large K wants thinner
activations, and the fused statistics want (pixels per partial row) x max z^2 below 2^24.
"""
import torch

from tests import conv_h16_ref as R
from tests.conv_h16_ref import ACT_LEAKY, ACT_MISH, ACT_NONE, OUT_HEAD, OUT_NHWC, OUT_UPSAMPLE2X, _c

TILE_DMA, TILE_DMA_IDENT_QUADS, TILE_S2_GEMM, TILE_WS = 8, 10, 13, 14
UP = OUT_UPSAMPLE2X
WS_TH, WS_TW, WS_GRID = 8, 16, 512
RING_SLOTS = 5


# ------------------------------------------------------------------------------------------------- where a case is routed
def _rows16(c):
    return c.y_ld % 8 == 0 and c.y_off % 8 == 0 and (not c.res or (c.r_ld % 8 == 0 and c.r_off % 8 == 0))


def dma_ok(c):
    return (c.kind == "fwd" and c.k == 3 and c.stride == 1 and c.cout > 64 and c.cin <= 2048 and c.cout % 8 == 0 and c.out != OUT_HEAD
            and _rows16(c))


def dma1_ok(c):
    return (c.kind == "fwd" and c.k == 1 and c.stride == 1 and c.cout >= 128 and c.cin >= 128 and c.cout % 8 == 0 and c.out != OUT_HEAD
            and _rows16(c))


def s2_ok(c):
    return (c.kind == "fwd" and c.k == 3 and c.stride == 2 and c.cout >= 128 and c.cout % 8 == 0 and c.out == OUT_NHWC and _rows16(c)
            and c.cin * 9 // 32 >= 4)


def ws_eligible(c):
    if c.kind != "fwd" or c.k != 3 or c.out != OUT_NHWC:
        return False
    shape = ((c.stride == 1 and ((c.cin == 32 and 32 < c.cout <= 64) or (c.cin == 64 and c.cout <= 32)))
             or (c.stride == 2 and c.cin == 32 and 32 < c.cout <= 64))
    return shape and c.cout % 8 == 0 and c.x_ld % 8 == 0 and c.x_off % 8 == 0 and _rows16(c) and not (c.stride == 2 and (c.H % 2 or c.W % 2))


def s2g_ok(c):
    """the fused stride-2 input gradient; cin = dx channels, cout = dz channels"""
    return c.kind == "dgrad" and c.cin in (32, 64) and c.cout % 32 == 0 and c.cout >= 32 and _rows16(c)


def default_kernel(c):
    """the kernel of the default dispatch (tile 0, no A/B switch set), in the order conv_h16.hip asks"""
    if c.kind == "dgrad":
        return "conv1_dma_h16/2" if s2g_ok(c) else "conv_patch_h16"
    if ws_eligible(c):
        return "conv3_ws_h16"
    if dma1_ok(c):
        return "conv1_dma_h16/0"
    if s2_ok(c):
        return "conv1_dma_h16/1"
    return "conv3_dma_h16" if dma_ok(c) else "conv_patch_h16"


def forced_ok(c):
    """does the tile the case forces accept it? (else: YOLO_ERR_UNSUPPORTED and nothing is written)"""
    return {TILE_DMA: dma_ok(c) or dma1_ok(c), TILE_S2_GEMM: s2_ok(c), TILE_WS: ws_eligible(c)}[c.tile]


def kt(c):
    """K steps of 32 channels"""
    return 4 * c.cout // 32 if c.kind == "dgrad" else c.cin // 32 * c.k * c.k


def gemm_blocks(c):
    """conv1_dma_h16: (pixel tiles of 128, channel tiles of 128, pixels in the last pixel tile)"""
    m = c.B * c.H * c.W if c.kind == "dgrad" else c.B * R.res_hw(c)[0] * R.res_hw(c)[1]
    n = 4 * c.cin if c.kind == "dgrad" else c.cout
    return -(-m // 128), -(-n // 128), (m - 1) % 128 + 1


def ws_tiles(c):
    """conv3_ws_h16: (tiles, iterations of the busiest workgroup, workgroups in the last round)"""
    ho, wo = R.res_hw(c)
    t = c.B * -(-ho // WS_TH) * -(-wo // WS_TW)
    return t, -(-t // WS_GRID), (t - 1) % WS_GRID + 1


def stats_ok(c):
    """yolo_conv_fwd_stats takes the case: identity epilogue, no residual, NHWC, and a kernel with fused statistics"""
    return c.kind == "fwd" and c.act == ACT_NONE and not c.res and c.out == OUT_NHWC and forced_ok(c)


def stats_row_pixels(c):
    """most pixels one partial row sums: a wave's 64 pixels of a block (DMA kernels), 32 pixels of every tile of a workgroup"""
    return 32 * ws_tiles(c)[1] if c.tile == TILE_WS else 64


def stats_value(c, ops, dtype=torch.float64):
    """z of yolo_conv_fwd_stats: the raw convolution, no scale / shift"""
    n = R.n_out(c)
    return R.value(c, dict(ops, scale=torch.ones(n), shift=torch.zeros(n)), dtype)


# ------------------------------------------------------------------------------------------------------------ the cases
def _a(name, B, H, W, cin, cout, **kw):
    return _c("A-" + name, B, H, W, cin, cout, tile=TILE_DMA, default=True, **kw)


INT_A = [
    # KT = 4: only the four peeled steps; 5: one steady step; 9: the write slot wraps. KT % 5 = 4, 0, 1, 2, 3, 4: the table's slot
    _a("kt4", 2, 5, 7, 128, 128),
    _a("kt5", 2, 5, 7, 160, 128),
    _a("kt6", 2, 5, 7, 192, 128),
    _a("kt7", 2, 5, 7, 224, 128),
    _a("kt8", 2, 5, 7, 256, 128),
    _a("kt9", 2, 5, 7, 288, 128),
    _a("one-pixel", 1, 1, 1, 128, 128),                                           # every lane clamps to pixel M - 1 = 0
    # blocks 1 (above), 2, 7, 8, 9, 17: the XCD remap with (q, r) = (0, n), (1, 0), (1, 1), (2, 1)
    _a("2-blocks", 1, 3, 43, 128, 128),                                           # 129 pixels: the last tile holds one
    _a("7-blocks", 1, 29, 29, 128, 128, xmax=4),
    _a("8-blocks", 1, 30, 30, 128, 128, xmax=4),
    _a("9-blocks", 1, 25, 41, 128, 128, xmax=4),                                  # 1025 pixels: the last tile holds one
    _a("17-blocks", 1, 33, 65, 128, 128, xmax=4),
    _a("cout136-res-view", 2, 5, 7, 128, 136, res=1, r_ld=144, r_off=8),          # the residual load's ch < Cout ? ch : 0
    _a("cout200", 2, 5, 7, 160, 200),
    _a("slices", 3, 5, 5, 128, 256, x_ld=512, x_off=64, y_ld=768, y_off=256),
    _a("up2x-two-images", 2, 5, 6, 128, 128, out=UP, y_ld=192, y_off=64),         # the offset's division by Ho * Wo
    _a("leaky-res", 3, 5, 5, 128, 128, act=ACT_LEAKY, res=1),                     # both fp32 roundings of kernel_steps
    _a("fallback-y_ld132", 2, 5, 7, 128, 128, y_ld=132),                          # tile 8 refuses; tile 0 is the patch kernel
]


def _b(name, B, H, W, cin, cout, **kw):
    return _c("B-" + name, B, H, W, cin, cout, k=3, stride=2, tile=TILE_S2_GEMM, default=True, **kw)


INT_B = [
    _b("kt9-one-output", 3, 2, 2, 32, 128),                                       # every top and left tap reads the zero page
    _b("kt18-straddle", 3, 10, 10, 64, 128),                                      # 25 outputs per image
    _b("kt27-ragged", 2, 26, 26, 96, 128, xmax=4),                                # 338 outputs: three tiles, the last ragged
    _b("rect", 1, 6, 44, 32, 128),                                                # TW = 22, PC = 66
    _b("cout136-res-view", 2, 10, 10, 32, 136, res=1, r_ld=144, r_off=8, y_ld=160, y_off=16),
    _b("x-slice", 2, 6, 8, 32, 128, x_ld=96, x_off=32),                           # the tap offset multiplies by x_ld
    _b("leaky", 2, 6, 8, 64, 128, act=ACT_LEAKY),
]


def _g(name, B, H, W, dx, dz, **kw):
    return _c("C-" + name, B, H, W, dx, dz, kind="dgrad", **kw)


INT_C = [  # H, W of dz; 32 dx channels: one n tile with all four parity classes, 64: two n tiles
    _g("kt4-1x1", 1, 1, 1, 32, 32),                                               # both neighbours outside
    _g("kt8-3x5", 1, 3, 5, 32, 64),
    _g("kt12-straddle", 3, 5, 5, 64, 96),
    _g("kt20-ragged", 2, 13, 13, 32, 160),                                        # 338 dz pixels
    _g("accumulate", 2, 3, 5, 64, 32, res=2),
    _g("res-view", 1, 3, 5, 32, 64, res=1, r_ld=48, r_off=8),
    _g("dz-slice-dx-view", 1, 3, 5, 64, 128, x_ld=192, x_off=32, y_ld=96, y_off=32),
    _g("fallback-dx_ld36", 2, 3, 5, 32, 64, y_ld=36),                             # the four per-class launches
]


def _d(name, B, H, W, cin, cout, **kw):
    return _c("D-" + name, B, H, W, cin, cout, k=3, tile=TILE_DMA, default=True, **kw)


INT_D = [
    _d("1-chunk-all-halo", 1, 1, 1, 32, 72),                                      # never a next patch to prefetch; one ragged n tile
    _d("2-chunks-column", 1, 40, 1, 64, 128),
    _d("3-chunks-row130", 1, 1, 130, 96, 136),                                    # two column tiles past the 126 cap
    _d("8-chunks-19x19", 1, 19, 19, 256, 128, xmax=1),
    _d("image-crossing", 5, 7, 7, 32, 256),                                       # a tile over three images
    _d("2x13x13-res-view", 2, 13, 13, 64, 136, res=1, r_ld=144, r_off=8, y_ld=160, y_off=16),
    _d("9x33-up2x", 1, 9, 33, 32, 128, out=UP),
    _d("52x52", 1, 52, 52, 32, 128, xmax=4),                                      # the 32 x 4 tile: tiles 8 and 10 permute quads differently
    _d("leaky-x-slice", 2, 6, 5, 64, 72, act=ACT_LEAKY, x_ld=96, x_off=32),
    _d("fallback-y_ld132", 2, 6, 6, 32, 128, y_ld=132),
]


def _e(name, B, H, W, cin, cout, **kw):
    return _c("E-" + name, B, H, W, cin, cout, k=3, tile=TILE_WS, default=True, **kw)


INT_E = [
    _e("32-40-1x1", 1, 1, 1, 32, 40),
    _e("32-48-one-tile", 1, 8, 16, 32, 48),
    _e("32-56-9x17", 1, 9, 17, 32, 56),                                           # four tiles, each ragged by one pixel
    _e("32-64-leaky-res", 2, 9, 17, 32, 64, act=ACT_LEAKY, res=1),
    _e("64-8-9x17", 1, 9, 17, 64, 8, xmax=4),
    _e("64-24-one-tile", 1, 8, 16, 64, 24, xmax=4),
    _e("64-32-1x1", 1, 1, 1, 64, 32),
    _e("s2-32-40-2x2", 1, 2, 2, 32, 40, stride=2),
    _e("s2-32-64-9x17", 2, 18, 34, 32, 64, stride=2),
    # the persistent loop: 513 tiles = one workgroup runs twice (patch buffer 1); more than 1024 with a ragged last round =
    # three iterations (buffer 0 again). Many small images, 3 / 8 / 4 tiles each. Every instantiation adds a residual in its
    # second iteration once, and sums its statistics over two or three iterations.
    _e("32-64-513-tiles-res", 171, 8, 33, 32, 64, xmax=4, res=1),
    _e("32-40-1032-tiles", 129, 9, 49, 32, 40, xmax=4),
    _e("64-32-513-tiles", 171, 8, 33, 64, 32, xmax=4),
    _e("64-32-513-tiles-res", 171, 8, 33, 64, 32, xmax=4, res=1),
    _e("64-24-1032-tiles-view", 129, 9, 49, 64, 24, xmax=4, y_ld=40, y_off=8),
    _e("s2-32-64-513-tiles-res", 171, 16, 66, 32, 64, stride=2, xmax=4, res=1),
    _e("s2-32-40-1028-tiles", 257, 18, 34, 32, 40, stride=2, xmax=4),
]

INT_FWD = INT_A + INT_B + INT_D + INT_E
INT_CASES = INT_FWD + INT_C
STATS_CASES = [c for c in INT_FWD if stats_ok(c)]
NAN_CASES = [INT_A[1], INT_B[1], INT_D[4], INT_E[2]]

GAUSS_CASES = [  # Mish, real scale / shift and a residual, one per kernel mode (the gradient has no activation)
    _c("gauss-A", 3, 5, 5, 160, 136, act=ACT_MISH, res=1, tile=TILE_DMA, default=True),
    _c("gauss-B", 2, 10, 10, 64, 136, k=3, stride=2, act=ACT_MISH, res=1, tile=TILE_S2_GEMM, default=True),
    _c("gauss-C", 2, 5, 5, 64, 96, kind="dgrad", res=1),
    _c("gauss-D", 2, 13, 13, 96, 136, k=3, act=ACT_MISH, res=1, tile=TILE_DMA, default=True),
    _c("gauss-E", 2, 9, 17, 32, 64, k=3, act=ACT_MISH, res=1, tile=TILE_WS, default=True),
]
