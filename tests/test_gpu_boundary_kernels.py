"""GPU tests (``-m gpu``) of the boundary kernels (layout.hip and the two movers of calls.hip), called through the C ABI:

  entry point                               kernels                               cases
  yolo_nchw_to_nhwc                         nchw_to_nhwc_small                    c_pad <= 8 fp32; 2,097,929 pixels: past 8192 blocks
                                            nchw_to_nhwc_small_h16                c_pad = 8 16-bit; 4,195,081 pixels: past 16384 blocks
                                            nchw_to_nhwc_tiled                    c and h w across 32, padding across a tile
  yolo_nhwc_to_nchw                         nhwc_to_nchw_tiled                    a channel slice (x_ld, x_off) of a wider buffer
  yolo_bn_fold                              bn_fold_kernel                        c around one block; gamma = NULL
  yolo_pack_weights / yolo_unpack_weights   pack_weights_f32, unpack_weights_f32  padded and unpadded cin and cout, 1x1 and 3x3
  yolo_fill_zero                            fill_zero_kernel / memset             1 byte to past 2048 blocks, aligned or not
  yolo_copy_d2d                             copy_kernel (16-byte and byte path)   the same sizes, either pointer unaligned

The movers are bit-exact: fp32 is a pure move, a 16-bit output is ``torch.Tensor.to`` of the value (round to nearest even),
checked with +-0, +-inf, subnormals, overflow and exact ties planted. Every output is pre-filled with a sentinel (or NaN
where a read of an unwritten element must show) and followed by 256 bytes of 0xA5 that must come back unchanged. Data is
seeded from the case tuple; the multi-megabyte cases are generated and compared on the device. Measured maxima are printed
(run with -s).
"""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -12288.0                       # exact in fp32, fp16 and bf16
GUARD = 256
EPS = float(np.float32(1e-5))
DTYPES = ["fp32", "bf16", "fp16"]


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _dt(L, dtype):
    return {"fp32": (L.F32, torch.float32), "bf16": (L.BF16, torch.bfloat16), "fp16": (L.F16, torch.float16)}[dtype]


def _gen(*case):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(case).encode()))


def _sync():
    torch.cuda.synchronize()


class Out:
    """`numel` elements of `tdt` filled with `fill`, `front` bytes into an allocation, 0xA5 in front of and behind them"""

    def __init__(self, numel, tdt, fill=SENT, front=0):
        size = torch.empty((), dtype=tdt).element_size()
        self.raw = torch.full((front + numel * size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.front, self.end = front, front + numel * size
        self.t = self.raw[front:self.end].view(tdt) if front % size == 0 else None
        if self.t is not None:
            self.t.fill_(fill)

    def ptr(self):
        return self.raw.data_ptr() + self.front

    def guards_ok(self):
        return bool((self.raw[:self.front] == 0xA5).all()) and bool((self.raw[self.end:] == 0xA5).all())


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# fp32 values whose 16-bit conversion is decided by the rounding rule, the range or the sign of zero
SPECIALS = [0.0, -0.0, float("inf"), -float("inf"), 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,      # bf16 ties
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 2048 + 1.0, 2048 + 3.0,                     # fp16 ties
            65504.0, 65519.996, 65520.0, -65520.0, 1e30, 3.4e38, -3.4e38,                                                # fp16 overflow, bf16 top
            2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -14 - 2.0 ** -25, 6e-8, -6e-8,           # fp16 subnormals
            2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -127]                                                         # bf16 subnormals


def _input(n, c, h, w, *case):
    """Gaussian (n, c, h, w) with SPECIALS spread over it (as many as fit in a quarter of it, the whole of a tiny one)"""
    x = torch.randn((n, c, h, w), generator=_gen("nchw", n, c, h, w, *case), device="cuda")
    flat = x.view(-1)
    k = min(len(SPECIALS), max(1, flat.numel() // 4)) if flat.numel() >= 8 else 0
    if k:
        pos = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(n * c * h * w))[:k].cuda()
        flat[pos] = torch.tensor(SPECIALS[:k], device="cuda")
    return x


def _nhwc_want(x, c_pad, tdt):
    n, c, h, w = x.shape
    want = torch.zeros((n, h, w, c_pad), dtype=tdt, device=x.device)
    want[..., :c] = x.permute(0, 2, 3, 1).to(tdt)
    return want


def _to_nhwc(L, x, c_pad, dtype, flag=None):
    code, tdt = _dt(L, dtype)
    n, c, h, w = x.shape
    out = Out(n * h * w * c_pad, tdt)
    L.check(L.lib().yolo_nchw_to_nhwc(x.data_ptr(), out.ptr(), n, c, h, w, c_pad, code, L.ptr(flag), L.current_stream()), "yolo_nchw_to_nhwc")
    _sync()
    assert out.guards_ok(), "nchw_to_nhwc wrote past its output"
    return out.t.view(n, h, w, c_pad)


# =============================================================================================== yolo_nchw_to_nhwc
NHWC_CASES = [(2, 3, 5, 7, 4, "fp32"), (1, 1, 1, 1, 8, "fp32"),                                               # small
              (2, 3, 5, 7, 8, "bf16"), (2, 3, 5, 7, 8, "fp16"), (1, 8, 3, 3, 8, "fp16"),                      # small_h16
              (2, 33, 3, 11, 40, "fp32"), (2, 33, 3, 11, 40, "bf16"), (2, 33, 3, 11, 40, "fp16"),             # tiled: c, h w and c_pad
              (1, 9, 1, 1, 16, "fp32"), (1, 3, 5, 7, 16, "bf16")]                                             # across 32; c_pad > 8
NHWC_IDS = ["n%d-c%d-%dx%d-pad%d-%s" % c for c in NHWC_CASES]


def test_special_values_convert_as_the_tables_say():
    """what the planted values are for, on the host: ties go to even, 65520 is the first fp16 infinity, zeros keep their sign"""
    x = torch.tensor(SPECIALS)
    bf, hf = x.to(torch.bfloat16).float(), x.to(torch.float16).float()
    at = lambda v: SPECIALS.index(v)
    assert bf[at(1 + 2.0 ** -8)] == 1.0 and bf[at(1 + 3 * 2.0 ** -8)] == 1 + 2.0 ** -6 and bf[at(1 + 2.0 ** -8 + 2.0 ** -23)] == 1 + 2.0 ** -7
    assert hf[at(1 + 2.0 ** -11)] == 1.0 and hf[at(1 + 3 * 2.0 ** -11)] == 1 + 2.0 ** -9 and hf[at(2049.0)] == 2048 and hf[at(2051.0)] == 2052
    assert hf[at(65519.996)] == 65504 and torch.isinf(hf[at(65520.0)]) and hf[at(2.0 ** -25)] == 0 and hf[at(3 * 2.0 ** -25)] == 2.0 ** -23
    assert bf[at(2.0 ** -134)] == 0 and bf[at(3 * 2.0 ** -134)] == 2.0 ** -132 and bf[at(2.0 ** -133)] == 2.0 ** -133
    assert SPECIALS[1] == 0 and torch.signbit(hf[1]) and torch.signbit(bf[1]) and not torch.signbit(bf[0]) and torch.signbit(hf[at(-6e-8)])


@pytest.mark.parametrize("case", NHWC_CASES, ids=NHWC_IDS)
def test_nchw_to_nhwc_is_bit_exact(L, case):
    """every element where it belongs, the padding channels [c, c_pad) +0, no NaN seen: the flag stays 0"""
    n, c, h, w, c_pad, dtype = case
    x = _input(n, c, h, w, c_pad, dtype)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _to_nhwc(L, x, c_pad, dtype, flag)
    want = _nhwc_want(x.cpu(), c_pad, _dt(L, dtype)[1])
    assert _same_bits(got.cpu(), want)
    assert int(flag) == 0


@pytest.mark.parametrize("case", NHWC_CASES, ids=NHWC_IDS)
def test_nchw_to_nhwc_nan_flag(L, case):
    """one NaN at the first, the last and a middle element sets the flag to 1 (and arrives as a NaN where it belongs, all
    else unchanged); a preset 1 stays without a NaN; a null flag pointer is accepted with and without a NaN"""
    n, c, h, w, c_pad, dtype = case
    tdt = _dt(L, dtype)[1]
    x0 = _input(n, c, h, w, c_pad, dtype)
    clean = _nhwc_want(x0, c_pad, tdt)
    numel = x0.numel()
    for pos in sorted({0, numel // 2, numel - 1}):
        x = x0.clone()
        x.view(-1)[pos] = float("nan")
        for flag in (torch.zeros(1, dtype=torch.int32, device="cuda"), None):
            got = _to_nhwc(L, x, c_pad, dtype, flag)
            assert flag is None or int(flag) == 1
            nan_at = torch.isnan(got.float())
            assert torch.equal(nan_at, torch.isnan(_nhwc_want(x, c_pad, tdt).float())) and int(nan_at.sum()) == 1
            assert torch.equal(_bits(got)[~nan_at], _bits(clean)[~nan_at])
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    assert _same_bits(_to_nhwc(L, x0, c_pad, dtype, flag), clean) and int(flag) == 1
    assert _same_bits(_to_nhwc(L, x0, c_pad, dtype, None), clean)


@pytest.mark.parametrize("n,h,w,c_pad,dtype", [(41, 1, 51169, 4, "fp32"), (11, 1, 381371, 8, "bf16"), (11, 1, 381371, 8, "fp16")],
                         ids=["small-8192-blocks", "small_h16-16384-blocks-bf16", "small_h16-16384-blocks-fp16"])
def test_nchw_to_nhwc_past_the_grid_caps(L, n, h, w, c_pad, dtype):
    """n h w = 2,097,152 + 777 (fp32: 8192 blocks of 256 pixels) and 4,194,304 + 777 (16-bit: 16384 blocks): the first 777
    pixels are a second trip of the grid-stride loop, in an image other than the first. On the device throughout."""
    assert n * h * w == {4: 8192, 8: 16384}[c_pad] * 256 + 777
    x = _input(n, 3, h, w, "cap", dtype)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _to_nhwc(L, x, c_pad, dtype, flag)
    assert _same_bits(got, _nhwc_want(x, c_pad, _dt(L, dtype)[1])) and int(flag) == 0
    x[n - 1, 2, 0, w - 1] = float("nan")                                  # the last element: seen by the second trip of block 776
    x[0, 0, 0, 776] = float("nan")
    _to_nhwc(L, x, c_pad, dtype, flag)
    assert int(flag) == 1


# =============================================================================================== yolo_nhwc_to_nchw
def _slice_input(n, c, hw, x_ld, x_off, tdt, *case):
    """flat NHWC buffer of n hw x_ld + x_off elements, NaN everywhere but the c channels at x_off of every pixel (with
    x_off + c > x_ld the slice of a pixel ends in the next row, as the kernel's flat index pixel * x_ld + x_off + channel does)"""
    buf = torch.full((n * hw * x_ld + x_off,), float("nan"), dtype=tdt, device="cuda")
    idx = (torch.arange(n * hw, device="cuda").view(-1, 1) * x_ld + x_off + torch.arange(c, device="cuda").view(1, -1))
    vals = torch.randn((n * hw, c), generator=_gen("nhwc", n, c, hw, x_ld, x_off, *case), device="cuda").to(tdt)
    k = min(len(SPECIALS), vals.numel())
    vals.view(-1)[:k] = torch.tensor(SPECIALS, device="cuda")[:k].to(tdt)
    buf[idx.view(-1)] = vals.view(-1)                       # c <= x_ld: the slices of two pixels never overlap
    return buf, vals.view(n, hw, c)


def _to_nchw(L, buf, n, c, h, w, x_ld, x_off, dtype):
    out = Out(n * c * h * w, torch.float32)
    L.check(L.lib().yolo_nhwc_to_nchw(buf.data_ptr(), out.ptr(), n, c, h, w, x_ld, x_off, _dt(L, dtype)[0], L.current_stream()),
            "yolo_nhwc_to_nchw")
    _sync()
    assert out.guards_ok(), "nhwc_to_nchw wrote past its output"
    return out.t.view(n, c, h, w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,x_ld,x_off", [((2, 33, 3, 11), 33, 0), ((2, 33, 3, 11), 33, 7), ((2, 33, 3, 11), 64, 0),
                                              ((2, 33, 3, 11), 64, 7), ((1, 1, 1, 1), 1, 0), ((1, 1, 1, 1), 5, 3)])
def test_nhwc_to_nchw_is_bit_exact(L, dtype, shape, x_ld, x_off):
    """33 channels and 33 pixels: both tile loops straddle 32. Every element of the buffer outside the slice is NaN and
    none may appear; 16-bit values widen exactly (subnormals and infinities included)."""
    n, c, h, w = shape
    tdt = _dt(L, dtype)[1]
    buf, vals = _slice_input(n, c, h * w, x_ld, x_off, tdt)
    got = _to_nchw(L, buf, n, c, h, w, x_ld, x_off, dtype)
    want = vals.float().permute(0, 2, 1).reshape(n, c, h, w)
    assert not bool(torch.isnan(got).any()), "an element from outside the channel slice"
    assert _same_bits(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,c_pad", [((2, 33, 3, 11), 40), ((2, 3, 5, 7), 8), ((1, 1, 1, 1), 8)])
def test_round_trip_through_both_movers(L, dtype, shape, c_pad):
    n, c, h, w = shape
    x = _input(n, c, h, w, "round-trip", dtype)
    mid = _to_nhwc(L, x, c_pad, dtype)
    back = _to_nchw(L, mid, n, c, h, w, c_pad, 0, dtype)
    assert _same_bits(back, x.to(_dt(L, dtype)[1]).float())


# =============================================================================================== yolo_bn_fold
FOLD_C = [1, 255, 256, 257]


def _fold_inputs(c):
    g = _gen("bn_fold", c)
    u = lambda: torch.rand(c, generator=g, device="cuda")
    gamma = (0.5 + u()) * torch.where(u() < 0.25, -1.0, 1.0)
    beta, mean = torch.randn(c, generator=g, device="cuda"), torch.randn(c, generator=g, device="cuda") * 3
    var = torch.exp(np.log(1e-8) + u() * (np.log(1e4) - np.log(1e-8)))
    var[0], var[-1] = 1e-8, 1e4
    return [t.float().cpu() for t in (gamma, beta, mean, var)]


def _fold64(gamma, beta, mean, var):
    s = gamma.double() / torch.sqrt(var.double() + EPS)
    return s, beta.double() - mean.double() * s


@pytest.fixture(scope="module")
def fold_fp32_error():
    """Relative error of a numpy fp32 evaluation (one rounding per operation) of scale = gamma / sqrt(var + eps) and
    shift = beta - mean * scale against fp64, the shift relative to |beta| + |mean scale|: the largest over the inputs of all
    four channel counts (a single channel alone can round luckily and say nothing about the formula)."""
    e_scale = e_shift = 0.0
    for c in FOLD_C:
        gamma, beta, mean, var = [t.numpy() for t in _fold_inputs(c)]
        s32 = (gamma / np.sqrt(var + np.float32(EPS))).astype(np.float32)
        h32 = (beta - (mean * s32).astype(np.float32)).astype(np.float32)
        s64, h64 = _fold64(*[torch.from_numpy(a) for a in (gamma, beta, mean, var)])
        e_scale = max(e_scale, float(((torch.from_numpy(s32).double() - s64).abs() / s64.abs()).max()))
        e_shift = max(e_shift, float(((torch.from_numpy(h32).double() - h64).abs() / (torch.from_numpy(beta).double().abs() + (torch.from_numpy(mean).double() * s64).abs())).max()))
    print(f"bn_fold: numpy fp32 against fp64: scale rel err {e_scale:.3e}, shift err / (|beta| + |mean scale|) {e_shift:.3e}")
    assert 2.0 ** -26 < e_scale < 2.0 ** -21 and 2.0 ** -26 < e_shift < 2.0 ** -21      # a few roundings of 2^-24
    return e_scale, e_shift


def _fold(L, c, gamma, beta, mean, var):
    scale, shift = Out(c + 8, torch.float32), Out(c + 8, torch.float32)
    dev = [None if t is None else t.cuda() for t in (gamma, beta, mean, var)]
    L.check(L.lib().yolo_bn_fold(*[L.ptr(t) for t in dev], EPS, scale.ptr(), shift.ptr(), c, L.current_stream()), "yolo_bn_fold")
    _sync()
    for o in (scale, shift):
        assert o.guards_ok() and bool((o.t[c:] == SENT).all()), "bn_fold wrote past channel c"
    return scale.t[:c].cpu(), shift.t[:c].cpu()


@pytest.mark.parametrize("c", FOLD_C)
def test_bn_fold_vs_fp64(L, fold_fp32_error, c):
    """variances from 1e-8 (below eps) to 1e4; within 4x the fp32 formula's own error (the factor is the suite's allowance
    for the device's sqrt and divide and a contracted multiply-add)"""
    gamma, beta, mean, var = _fold_inputs(c)
    scale, shift = _fold(L, c, gamma, beta, mean, var)
    s64, h64 = _fold64(gamma, beta, mean, var)
    e_s = float(((scale.double() - s64).abs() / s64.abs()).max())
    e_h = float(((shift.double() - h64).abs() / (beta.double().abs() + (mean.double() * s64).abs())).max())
    print(f"bn_fold c {c}: scale rel err {e_s:.3e} (bound {4 * fold_fp32_error[0]:.3e}), shift {e_h:.3e} (bound {4 * fold_fp32_error[1]:.3e})")
    assert e_s <= 4 * fold_fp32_error[0] and e_h <= 4 * fold_fp32_error[1]


@pytest.mark.parametrize("c", FOLD_C)
def test_bn_fold_without_gamma(L, c):
    """a bare convolution: scale exactly 1; shift exactly the bias, or 0 without one. mean and var are not read."""
    _, beta, _, _ = _fold_inputs(c)
    scale, shift = _fold(L, c, None, beta, None, None)
    assert bool((scale == 1.0).all()) and _same_bits(shift, beta)
    scale, shift = _fold(L, c, None, None, None, None)
    assert bool((scale == 1.0).all()) and _same_bits(shift, torch.zeros(c))


# =============================================================================================== pack / unpack (fp32)
@pytest.mark.parametrize("cout,cin,k", [(1, 1, 1), (21, 3, 3), (255, 96, 1), (33, 40, 3), (64, 64, 3)])
def test_pack_unpack_round_trip(L, cout, cin, k):
    """OIHW -> packed -> OIHW gives the bits back. The packed buffer starts as NaN: a read of an element the packer left
    unwritten shows; its size is what yolo_packed_weight_bytes says, and the bytes behind it stay."""
    lib = L.lib()
    w = torch.randn((cout, cin, k, k), generator=_gen("pack", cout, cin, k), device="cuda")
    k8 = min(w.numel(), 6)
    w.view(-1)[:k8] = torch.tensor([-0.0, 0.0, 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126], device="cuda")[:k8]   # a move keeps them
    nbytes = lib.yolo_packed_weight_bytes(cout, cin, k, L.F32)
    assert nbytes >= w.numel() * 4 and nbytes % 4 == 0 and nbytes == 4 * lib.yolo_packed_weight_elems(cout, cin, k)
    packed = Out(nbytes // 4, torch.float32, fill=float("nan"))
    L.check(lib.yolo_pack_weights(w.data_ptr(), packed.ptr(), cout, cin, k, L.F32, L.current_stream()), "yolo_pack_weights")
    back = Out(w.numel(), torch.float32)
    L.check(lib.yolo_unpack_weights(packed.ptr(), back.ptr(), cout, cin, k, L.F32, L.current_stream()), "yolo_unpack_weights")
    _sync()
    assert packed.guards_ok() and back.guards_ok()
    assert _same_bits(back.t.view(w.shape), w)


# =============================================================================================== fill_zero / copy_d2d
SIZES = [1, 15, 16, 17, 4101, 2048 * 256 * 16 + 19]                         # the last: 2048 blocks of 256 x 16 bytes and a tail
FRONT = 64                                                                  # sentinel bytes in front, keeps 16-byte alignment


def _bytes(nbytes, *case):
    return torch.randint(0, 256, (nbytes,), generator=_gen("bytes", nbytes, *case), device="cuda", dtype=torch.int16).to(torch.uint8)


@pytest.mark.parametrize("off", [0, 1, 8])
@pytest.mark.parametrize("nbytes", SIZES)
def test_fill_zero(L, nbytes, off):
    """aligned start: the kernel (16-byte stores, a byte tail by block 0, a grid-stride loop past 2048 blocks); a start 1 or 8
    bytes off: the runtime's memset. The range is zero and the bytes around it are as they were."""
    buf = Out(nbytes, torch.uint8, fill=0xA5, front=FRONT + off)
    buf.raw[buf.front:buf.end] = _bytes(nbytes, "fill", off) | 1               # nothing is zero beforehand
    assert (buf.ptr() % 16 == 0) == (off == 0)
    L.check(L.lib().yolo_fill_zero(buf.ptr(), nbytes, L.current_stream()), "yolo_fill_zero")
    _sync()
    assert not bool(buf.raw[buf.front:buf.end].any()) and buf.guards_ok()


@pytest.mark.parametrize("d_off,s_off", [(0, 0), (1, 0), (0, 1), (8, 8), (1, 8)])
@pytest.mark.parametrize("nbytes", SIZES)
def test_copy_d2d(L, nbytes, d_off, s_off):
    """both pointers aligned: 16-byte moves and a byte tail; either one off: the byte path (its grid capped at 2048 blocks
    too). The destination equals the source, the source and the bytes around the destination are as they were."""
    src = Out(nbytes, torch.uint8, fill=0xA5, front=FRONT + s_off)
    data = _bytes(nbytes, "copy", d_off, s_off)
    src.raw[src.front:src.end] = data
    dst = Out(nbytes, torch.uint8, fill=0xA5, front=FRONT + d_off)
    dst.raw[dst.front:dst.end] = ~data
    L.check(L.lib().yolo_copy_d2d(dst.ptr(), src.ptr(), nbytes, L.current_stream()), "yolo_copy_d2d")
    _sync()
    assert torch.equal(dst.raw[dst.front:dst.end], data) and dst.guards_ok()
    assert torch.equal(src.raw[src.front:src.end], data) and src.guards_ok()
