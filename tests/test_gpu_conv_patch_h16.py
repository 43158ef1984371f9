"""GPU tests (``-m gpu``) of conv_patch_h16.hip, the register-staged bf16 / fp16 convolution, called through the C ABI at the
edges of its launch geometry (the case tables and their reasons: tests/conv_h16_ref.py):

  yolo_conv_fwd, tile 5 / 6 (64 / 128 channels per block) and tile 0 where the default dispatch lands in this kernel
      1x1            h_kstep_1x1: 1 .. 7 chunks (every remainder of the three-chunk unroll), 1 / 2 / 4 / 6 / 7 / 8 / 9 blocks,
                     ragged pixel and channel tiles, ld / off views, the 2x-upsampling store, the element-wise epilogue
      heads          YOLO_OUT_HEAD, fp32 (B, 3, H, W, nc5): images inside and across pixel tiles, anchors across channel passes
      3x3 stride 1   the double-buffered patch: all halo, two column tiles, tiles across two and three images
      3x3 stride 2   the single patch buffer
      unaligned      y / residual views whose rows are not on 16 bytes although cout % 8 == 0: the element-wise epilogue
  yolo_conv_dgrad_s2, dx channels other than 32 / 64: the four tap-subset launches, 1 .. 5 chunks, BN 128 and 64

Integer cases ask for BIT equality with the fp64 reference: tests/test_conv_h16_ref_host.py proves that their fp32 value ahead
of the store does not depend on the order of accumulation. Gaussian cases (Mish, real scale / shift) are held to the error of
one rounding at the store. Every output lies in a sentinel-filled buffer (heads: NaN-filled) between 0xA5 guard bytes; channels
outside [off, off + cout) must come back unchanged. Data is seeded from the case tuple. Measured maxima are printed (-s).
"""
import pytest
import torch

from tests import conv_h16_ref as R
from tests.conv_h16_launch import Launch, bits as _bits, reference as _reference, same_bits as _same_bits

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp16"]
TILE_BN64, TILE_BN128 = 5, 6


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _tiles(c):
    """(forced tiles, the forced tile the default dispatch must equal or None); the gradient has no tile argument"""
    if c.kind == "dgrad":
        return (0,), None
    auto = TILE_BN128 if (c.k == 3 and c.cout > 64) else TILE_BN64
    return (TILE_BN64, TILE_BN128) + ((0,) if c.default else ()), (auto if c.default else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.INT_CASES, ids=lambda c: c.name)
def test_integer_cases_are_bit_exact(L, case, dtype):
    """every forced tile (and tile 0 where it lands here) stores the bits of the fp64 reference; the default dispatch stores
    the bits of the forced tile its own rule picks"""
    c = case
    ops, ref = _reference(c, dtype, False)
    want = ref.float() if c.out == R.OUT_HEAD else ref.float().to(R.TDT[dtype])
    run = Launch(L, c, dtype, ops)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    tiles, auto = _tiles(c)
    outs = {}
    for tile in tiles:
        got, untouched = run.split(run.run(tile, flag=flag))
        wrong = _bits(got) != _bits(want)
        assert not bool(wrong.any()), "%s %s tile %d: %d of %d values differ, first at %s: got %s, want %s" % (
            c.name, dtype, tile, int(wrong.sum()), wrong.numel(), tuple(wrong.nonzero()[0].tolist()),
            got[wrong][:4].tolist(), want[wrong][:4].tolist())
        assert untouched, "%s tile %d: channels outside [off, off + cout) changed" % (c.name, tile)
        assert int(flag) == 0
        outs[tile] = got
    if auto is not None:
        assert _same_bits(outs[0], outs[auto])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.GAUSS_CASES, ids=lambda c: c.name)
def test_gaussian_cases_within_one_rounding(L, case, dtype):
    """Mish, LeakyReLU and real scale / shift against fp64 of the same rounded operands. Measured on an MI355X, error over
    max |reference|: bf16 2.8e-3 / 2.3e-3 / 1.6e-3 (1x1, 3x3, stride 2), fp16 2.9e-4 / 3.5e-4 / 2.9e-4, heads 1.5e-7 / 2.1e-7"""
    c = case
    ops, ref = _reference(c, dtype, True)
    tol = R.GAUSS_TOL_HEAD if c.out == R.OUT_HEAD else R.GAUSS_TOL[dtype]
    run = Launch(L, c, dtype, ops)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    tiles, auto = _tiles(c)
    outs = {}
    for tile in tiles:
        got, untouched = run.split(run.run(tile, flag=flag))
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print("%s %s tile %d: max error / max |reference| = %.3g (tolerance %g)" % (c.name, dtype, tile, err, tol))
        assert bool(torch.isfinite(got.float()).all()) and err <= tol, (c.name, dtype, tile, err)
        assert untouched and int(flag) == 0
        outs[tile] = got
    assert _same_bits(outs[0], outs[auto])              # the default dispatch is the kernel this file tests


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.NAN_CASES, ids=lambda c: c.name)
def test_nan_flag(L, case, dtype):
    """clean data leaves the flag alone; one NaN activation sets bit 1 (the other bits stay) and turns exactly the outputs
    whose window holds it into NaN, in every channel; without YOLO_FLAG_NANCHECK the flag is not written"""
    c = case
    ops, ref = _reference(c, dtype, False)
    want = ref.float() if c.out == R.OUT_HEAD else ref.float().to(R.TDT[dtype])
    run = Launch(L, c, dtype, ops)
    xn = run.x.clone()
    xn[c.B - 1, c.H // 2, c.W // 2, c.x_off + 3] = float("nan")
    bad = dict(ops, x=xn.cpu())
    nan_at = torch.isnan(R.stored(c, R.value(c, bad, torch.float64)))
    pixels = 1 if c.k == 1 else min(3, c.H) * min(3, c.W)
    assert int(nan_at.sum()) == pixels * c.cout
    for tile in (TILE_BN64, TILE_BN128):
        flag = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        assert _same_bits(run.split(run.run(tile, flag=flag))[0], want) and int(flag) == 4
        got = run.split(run.run(tile, x=xn, flag=flag))[0]
        assert int(flag) == 6
        assert torch.equal(torch.isnan(got.float()), nan_at) and torch.equal(_bits(got)[~nan_at], _bits(want)[~nan_at])
        flag.fill_(4)
        run.run(tile, x=xn, flag=flag, nancheck=False)
        assert int(flag) == 4
        run.run(tile, x=xn, flag=None, nancheck=False)
