"""fp64 restatement of what the 16-bit convolution entry points compute (conv_patch_h16.hip and its siblings), and the
case tables of tests/test_gpu_conv_patch_h16.py.

  yolo_conv_fwd (YOLO_BF16 / YOLO_F16)   y = act(scale[c] * conv(x, w)[c] + shift[c]) [+ residual], of the operands as rounded
                                         to the 16-bit type, written as NHWC into an ld / off view, as the 2x-replicated
                                         store, or as the fp32 head layout (B, 3, H, W, nc5) with channel = a * nc5 + k
  yolo_conv_dgrad_s2                     dx = conv_transpose2d(dz, w, stride 2, padding 1, output_padding 1) [+ residual]

Plain torch on the CPU, no project code. Every input is taken as stored (already rounded to its dtype) and promoted;
activations are NHWC, weights OIHW. ``tests/test_conv_h16_ref_host.py`` ties these functions to torch.nn.functional and to
oracle.net.cnn_block, and proves for every integer case below what the GPU test relies on: that the fp32 value ahead of the
store does not depend on the order of accumulation, and that most of those values need no rounding at the store.

Integer cases: activations and residual in +-{1..xmax} (xmax = 8 unless the case says otherwise: tests/conv_dma_h16_ref.py
thins the activations of its large-K cases), weights in {-1, 0, +1}, integer shift, scale in {1, 2, 0.5}. All
partial sums are integers (or halves) far below 2^24, so any fp32 evaluation gives the same bits and the expected output is
``torch.Tensor.to(dtype)`` of it. LeakyReLU stays exact in that sense: the kernels compute fmaxf(v, v * 0.1f), one fp32
rounding of a product, and add the residual in fp32, a second one; ``kernel_steps=True`` states those two roundings.
"""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_LEAKY, ACT_MISH = 0, 1, 2
OUT_NHWC, OUT_UPSAMPLE2X, OUT_HEAD = 0, 1, 2
LEAKY_SLOPE_F32 = float(np.float32(0.1))          # the kernels' 0.1f
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------------------------------------------ the operations
def _nchw(t, dtype):
    return t.to(dtype).permute(0, 3, 1, 2)


def act_ref(v, act, kernel_steps=False):
    if act == ACT_NONE:
        return v
    if act == ACT_LEAKY:
        if not kernel_steps:
            return torch.where(v > 0, v, 0.1 * v)
        lk = v * LEAKY_SLOPE_F32                   # fp32: rounded by the multiplication itself
        if v.dtype == torch.float64:
            lk = lk.float().double()               # fp64: the exact 48-bit product, rounded to fp32 once
        return torch.maximum(v, lk)
    if act == ACT_MISH:
        return v * torch.tanh(torch.logaddexp(v, torch.zeros_like(v)))
    raise ValueError(act)


def conv_fwd_ref(x, w, scale, shift, act, stride=1, residual=None, dtype=torch.float64, kernel_steps=False):
    """act(scale * conv(x, w) + shift) + residual as (B, Ho, Wo, cout) in `dtype`. x (B, H, W, cin) and residual
    (B, Ho, Wo, cout) as stored, w (cout, cin, k, k) holding the rounded weights, padding k // 2.
    kernel_steps: the fp32 roundings of the kernels' epilogue that are not a matter of order (see the module text)."""
    k = w.shape[-1]
    v = F.conv2d(_nchw(x, dtype), w.to(dtype), stride=stride, padding=k // 2)
    v = v * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    v = act_ref(v, act, kernel_steps).permute(0, 2, 3, 1)
    if residual is not None:
        v = v + residual.to(dtype)
        if kernel_steps and dtype == torch.float64:
            v = v.float().double()
    return v.contiguous()


def dgrad_s2_ref(dz, w, residual=None, dtype=torch.float64):
    """Input gradient of a 3x3 stride-2 convolution: dz (B, ho, wo, cout), w (cout, cin, 3, 3) -> (B, 2 ho, 2 wo, cin)."""
    v = F.conv_transpose2d(_nchw(dz, dtype), w.to(dtype), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    if residual is not None:
        v = v + residual.to(dtype)
    return v.contiguous()


def upsample2x(v):
    """(B, H, W, c) -> (B, 2H, 2W, c), every value at its 2x2 destination pixels"""
    return v.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def head_layout(v, nc5):
    """(B, H, W, 3 nc5) with channel = a * nc5 + k -> (B, 3, H, W, nc5)"""
    b, h, w, c = v.shape
    assert c == 3 * nc5
    return v.reshape(b, h, w, 3, nc5).permute(0, 3, 1, 2, 4).contiguous()


def place(buf, v, off):
    """`buf` (..., ld) with v (..., c) in channels [off, off + c)"""
    out = buf.clone()
    out[..., off:off + v.shape[-1]] = v.to(buf.dtype)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
# kind "fwd": x (B, H, W, cin) -> cout channels. kind "dgrad": dz (B, H, W, cout) -> dx (B, 2H, 2W, cin); x_* is the view of
# dz, y_* of dx. res: 0 none, 1 a buffer of its own (r_ld, r_off), 2 the output buffer itself (dgrad: accumulate in place).
# default: tile 0 runs the kernel the table is about (here conv_patch_h16) and must store the bits of the forced tile.
# xmax: integer activations and residual lie in +-{1..xmax}. tile: the tile id a table forces (0: the test's own choice).
# The last two fields came later: a case that leaves them at (8, 0) is seeded from the fields before them, as it always was.
Case = collections.namedtuple("Case", "kind name B H W cin cout k stride out act x_ld x_off y_ld y_off res r_ld r_off default xmax tile")
SEED_FIELDS = 19


def _c(name, B, H, W, cin, cout, k=1, stride=1, out=OUT_NHWC, act=ACT_NONE, x_ld=None, x_off=0, y_ld=None, y_off=0, res=0,
       r_ld=None, r_off=0, default=False, kind="fwd", xmax=8, tile=0):
    n, kin = (cin, cout) if kind == "dgrad" else (cout, cin)
    y_ld = y_ld or n
    if res == 2:
        r_ld, r_off = y_ld, y_off
    return Case(kind, name, B, H, W, cin, cout, k, stride, out, act, x_ld or kin, x_off, y_ld, y_off, res, r_ld or n, r_off, default, xmax, tile)


UP, HEAD = OUT_UPSAMPLE2X, OUT_HEAD

# 1x1: h_kstep_1x1 runs three chunks unrolled, loads two chunks ahead, then a remainder of 0 / 1 / 2 chunks.
# Blocks = pixel tiles of 128 x channel tiles of BN (64 at tile 5, 128 at tile 6): 1, 2, 4, 6, 7, 8 and 9 occur.
INT_1X1 = [
    _c("1x1-one-chunk", 2, 5, 7, 32, 64, default=True),                                  # every look-ahead clamps to chunk 0; one ragged tile
    _c("1x1-two-chunks-slices", 3, 9, 9, 64, 32, x_ld=96, x_off=32, y_ld=64, y_off=16, res=1, r_ld=40, r_off=8, default=True),
    _c("1x1-one-trio", 1, 3, 43, 96, 72, default=True),                                   # 129 pixels: the last tile holds one; 8-wide channel tile
    _c("1x1-four-chunks-up2x", 2, 5, 6, 128, 64, out=UP, y_ld=192, y_off=128, default=True),
    _c("1x1-five-chunks-ragged-n", 1, 13, 13, 160, 136),                                  # 136 = 128 + 8; the default is the DMA kernel
    _c("1x1-seven-chunks", 2, 4, 4, 224, 40, default=True),
    _c("1x1-7-blocks", 1, 29, 29, 32, 64, default=True),                                  # 841 pixels
    _c("1x1-8-blocks", 1, 30, 30, 32, 64, default=True),                                  # 900 pixels
    _c("1x1-9-blocks", 1, 33, 32, 32, 64, default=True),                                  # 1056 pixels: the XCD remap with q = 1, r = 1
    _c("1x1-scalar-21", 2, 5, 7, 64, 21, default=True),
    _c("1x1-scalar-21-res", 2, 5, 7, 64, 21, res=1, default=True),
    _c("1x1-scalar-20-up2x", 2, 5, 7, 64, 20, out=UP, y_ld=28, y_off=4, default=True),
    _c("1x1-leaky-res", 3, 9, 9, 64, 32, act=ACT_LEAKY, res=1, default=True),             # both fp32 roundings of kernel_steps
]
# views whose rows are not on 16 bytes: the element-wise epilogue although cout % 8 == 0
INT_UNALIGNED = [
    _c("1x1-y_ld36", 2, 5, 7, 64, 32, y_ld=36, default=True),
    _c("1x1-y_ld40-off4", 2, 5, 7, 64, 32, y_ld=40, y_off=4, default=True),
    _c("1x1-r_ld36", 2, 5, 7, 64, 32, res=1, r_ld=36, default=True),
    _c("1x1-up2x-y_ld36", 2, 5, 7, 64, 32, out=UP, y_ld=36, res=1, r_ld=34, r_off=2, default=True),
    _c("3x3-y_ld68", 2, 6, 6, 64, 64, k=3, y_ld=68, y_off=2, default=True),
]
INT_HEAD = [
    _c("head-nc5-7", 3, 5, 7, 64, 21, out=HEAD, default=True),                            # three images inside one pixel tile
    _c("head-nc5-85", 3, 7, 7, 256, 255, out=HEAD, default=True),                         # images straddle the tile boundary; ragged channel tile
    _c("head-smallest", 1, 1, 1, 32, 18, out=HEAD, default=True),
]
INT_3X3_S1 = [
    _c("3x3-all-halo", 1, 1, 1, 32, 8, k=3, default=True),
    _c("3x3-two-column-tiles", 1, 2, 130, 32, 64, k=3),                                   # wider than the 126-pixel tile cap
    _c("3x3-image-crossing", 5, 7, 7, 64, 64, k=3, default=True),
    _c("3x3-three-chunks-ragged-n", 2, 13, 13, 96, 136, k=3, res=1, y_ld=160, y_off=16),
    _c("3x3-scalar-21", 2, 6, 5, 32, 21, k=3, default=True),
    _c("3x3-up2x", 2, 6, 6, 64, 64, k=3, out=UP, default=True),
    _c("3x3-leaky", 2, 6, 5, 64, 64, k=3, act=ACT_LEAKY, default=True),
]
INT_3X3_S2 = [
    _c("s2-one-pixel", 1, 2, 2, 32, 32, k=3, stride=2, default=True),
    _c("s2-64-64", 2, 8, 12, 64, 64, k=3, stride=2, default=True),
    _c("s2-three-chunks-straddle", 3, 10, 10, 96, 136, k=3, stride=2),
    _c("s2-two-column-tiles", 1, 2, 256, 32, 64, k=3, stride=2),                          # 128 output columns
]
# stride-2 input gradient, one launch per parity class (dx channels other than 32 / 64): nchunks = dz channels / 32, three
# unrolled; BN = 128 unless ho > 52. H, W are those of dz.
INT_DGRAD = [
    _c("dgrad-1-chunk", 2, 3, 5, 96, 32, kind="dgrad"),
    _c("dgrad-2-chunks", 1, 4, 4, 96, 64, kind="dgrad"),
    _c("dgrad-3-chunks-accumulate-slice", 2, 5, 3, 128, 96, kind="dgrad", y_ld=160, y_off=32, res=2),
    _c("dgrad-4-chunks", 1, 3, 3, 160, 128, kind="dgrad"),
    _c("dgrad-5-chunks-dz-slice", 1, 2, 6, 96, 160, kind="dgrad", x_ld=192, x_off=32),
    _c("dgrad-bn64", 1, 53, 2, 96, 32, kind="dgrad"),
    _c("dgrad-dx_ld100", 2, 3, 5, 96, 32, kind="dgrad", y_ld=100),
    _c("dgrad-dx_ld104-r_ld100", 1, 4, 4, 96, 64, kind="dgrad", y_ld=104, y_off=4, res=1, r_ld=100, r_off=2),
]
INT_FWD = INT_1X1 + INT_UNALIGNED + INT_HEAD + INT_3X3_S1 + INT_3X3_S2
INT_CASES = INT_FWD + INT_DGRAD

GAUSS_CASES = [  # Mish, LeakyReLU on real values, scale / shift that are no powers of two
    _c("gauss-1x1-mish", 3, 9, 9, 64, 32, act=ACT_MISH, x_ld=96, x_off=32, y_ld=64, y_off=16, res=1, r_ld=40, r_off=8, default=True),
    _c("gauss-head", 3, 7, 7, 256, 255, out=HEAD, default=True),
    _c("gauss-3x3-mish", 5, 7, 7, 64, 64, k=3, act=ACT_MISH, res=1, default=True),
    _c("gauss-s2-leaky", 2, 8, 12, 64, 64, k=3, stride=2, act=ACT_LEAKY, default=True),
]
GAUSS_TOL = {"bf16": 1e-2, "fp16": 2e-3}      # max error over max |reference|, one rounding at the store (test_dma_conv_kernels_edge_shapes)
GAUSS_TOL_HEAD = 2e-5                          # fp32 output: accumulation order only (test_wgrad_16bit_kernel_vs_fp64)
NAN_CASES = [INT_1X1[1], INT_HEAD[0], INT_3X3_S1[2]]


def out_hw(c):
    """spatial size of the stored output"""
    if c.kind == "dgrad":
        return 2 * c.H, 2 * c.W
    ho, wo = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    return (2 * ho, 2 * wo) if c.out == OUT_UPSAMPLE2X else (ho, wo)


def res_hw(c):
    return (2 * c.H, 2 * c.W) if c.kind == "dgrad" else ((c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1)


def n_out(c):
    """channels the launch writes"""
    return c.cin if c.kind == "dgrad" else c.cout


def k_terms(c):
    """an upper bound of the products per output value"""
    return c.cout * 9 if c.kind == "dgrad" else c.cin * c.k * c.k


def _gen(c, dtype, what):
    key = tuple(c) if (c.xmax, c.tile) != (8, 0) else tuple(c)[:SEED_FIELDS]
    return torch.Generator().manual_seed(zlib.crc32(repr((key, dtype, what)).encode()))


def _ints(shape, g, xmax=8):
    v = torch.randint(-xmax, xmax, shape, generator=g)
    return torch.where(v >= 0, v + 1, v).float()            # +-{1..xmax}


ints = _ints                                                 # (the name other case modules use)


def operands(c, dtype, gauss=False):
    """The data of a case, seeded from it: x / w / scale / shift / residual as the launch gets them (x and residual whole
    buffers of their ld, rounded to the dtype; w fp32 OIHW holding values the dtype represents exactly)."""
    tdt = TDT[dtype]
    g = _gen(c, dtype, "gauss" if gauss else "int")
    n, kin = n_out(c), (c.cout if c.kind == "dgrad" else c.cin)
    rh, rw = res_hw(c)
    wshape = (c.cout, c.cin, c.k, c.k) if c.kind == "fwd" else (c.cout, c.cin, 3, 3)
    if gauss:
        x = torch.randn((c.B, c.H, c.W, c.x_ld), generator=g).to(tdt)
        w = (torch.randn(wshape, generator=g) * (1.0 / k_terms(c)) ** 0.5).to(tdt).float()
        scale, shift = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.1
        r = torch.randn((c.B, rh, rw, c.r_ld), generator=g).to(tdt)
    else:
        x = _ints((c.B, c.H, c.W, c.x_ld), g, c.xmax).to(tdt)
        w = torch.randint(-1, 2, wshape, generator=g).float()
        scale = torch.tensor([1.0, 2.0, 0.5])[torch.randint(0, 3, (n,), generator=g)]
        shift = torch.randint(-16, 17, (n,), generator=g).float()
        r = _ints((c.B, rh, rw, c.r_ld), g, c.xmax).to(tdt)
    if c.out == OUT_HEAD:
        scale = torch.ones(n)                                # a bare convolution: scale = 1, shift = bias
    return dict(x=x, w=w, scale=scale, shift=shift, r=r if c.res else None)


def value(c, ops, dtype=torch.float64, kernel_steps=False):
    """the value ahead of the store, (B, h, w, n_out) before any upsampling or head permutation, in `dtype`"""
    r = None if ops["r"] is None else ops["r"][..., c.r_off:c.r_off + n_out(c)]
    if c.kind == "dgrad":
        return dgrad_s2_ref(ops["x"][..., c.x_off:c.x_off + c.cout], ops["w"], r, dtype)
    return conv_fwd_ref(ops["x"][..., c.x_off:c.x_off + c.cin], ops["w"], ops["scale"], ops["shift"], c.act, c.stride, r, dtype, kernel_steps)


def stored(c, v):
    """`v` = value(...) as the output tensor holds it: (B, 3, H, W, nc5) for a head, else (B, ho, wo, n_out)"""
    if c.out == OUT_HEAD:
        return head_layout(v, c.cout // 3)
    return upsample2x(v) if c.out == OUT_UPSAMPLE2X else v
