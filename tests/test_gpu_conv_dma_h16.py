"""GPU tests (``-m gpu``) of the 16-bit kernels of the default path, called through the C ABI at the edges of their launch
geometry (the case tables and their reasons: tests/conv_dma_h16_ref.py):

  A  conv1_dma_h16, 1x1, tile 8             KT 4 .. 9 (peeled steps only, one steady step, the ring's wrap, every slot of the
                                            scale / shift table), one pixel, 1 / 2 / 7 / 8 / 9 / 17 blocks, ragged channel tiles
  B  conv1_dma_h16, gathered rows, tile 13  3x3 stride 2: zero-page taps, tiles across rows and images, rectangular inputs
  C  conv1_dma_h16, gather mode 2           yolo_conv_dgrad_s2 with 32 / 64 dx channels: one GEMM for the four parity classes
  D  conv3_dma_h16, tiles 8 and 10          1 / 2 / 3 / 8 chunks, all halo, column, row, image-crossing and 32 x 4 tiles
  E  conv3_ws_h16, tile 14                  all three instantiations, one to 1032 tiles: the second and third iteration of the
                                            persistent loop, both patch buffers, the ragged last round

Integer cases ask for BIT equality with the fp64 reference (tests/test_conv_dma_h16_ref_host.py proves that the fp32 value
ahead of the store does not depend on the order of accumulation), from every forced tile and, unless an A/B switch of the
library is set, from the default dispatch, which must pick the same kernel. A view that a forced tile cannot take
("fallback") must be refused with nothing written while tile 0 still stores the reference bits. The fused statistics must
add up to the fp64 sums of the stored z and z^2 exactly. Every output lies in a sentinel-filled buffer between 0xA5 guard
bytes; channels outside [off, off + cout) must come back unchanged. Measured maxima are printed (-s).
"""
import pytest
import torch

from tests import conv_dma_h16_ref as D
from tests import conv_h16_ref as R
from tests.conv_h16_launch import ERR_UNSUPPORTED, Launch, bits, reference, same_bits, switches

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _switched_off(L, c):
    """the A/B switches in force that take the default dispatch of this case away from the kernel its table names"""
    watch = {"A": ("YOLO_NO_DMA",), "B": ("YOLO_NO_DMA", "YOLO_NO_S2_DMA"), "C": ("YOLO_NO_DMA", "YOLO_NO_S2G"), "D": ("YOLO_NO_DMA",),
             "E": ("YOLO_NO_CONV3_WS",)}[c.name.split("-")[-1 if c.name.startswith("gauss") else 0]]
    sw = switches(L)
    assert all(k in sw for k in watch)
    return [k for k in watch if sw[k]]


def _forced(c):
    if c.kind == "dgrad":
        return ()                                                      # the gradient has no tile argument
    return (D.TILE_DMA, D.TILE_DMA_IDENT_QUADS) if (c.tile == D.TILE_DMA and c.k == 3) else (c.tile,)


def _assert_bits(c, dtype, tile, got, want, what=""):
    wrong = bits(got) != bits(want)
    assert not bool(wrong.any()), "%s %s tile %d%s: %d of %d values differ, first at %s: got %s, want %s" % (
        c.name, dtype, tile, what, int(wrong.sum()), wrong.numel(), tuple(wrong.nonzero()[0].tolist()),
        got[wrong][:4].tolist(), want[wrong][:4].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", D.INT_CASES, ids=lambda c: c.name)
def test_integer_cases_are_bit_exact(L, case, dtype):
    """every forced tile stores the bits of the fp64 reference, or refuses the view and writes nothing; the default dispatch
    stores the same bits (where it is the patch kernel too: the fallback cases)"""
    c = case
    ops, ref = reference(c, dtype, False)
    want = ref.float().to(R.TDT[dtype])
    run = Launch(L, c, dtype, ops)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = {}
    for tile in _forced(c):
        rc, whole = run.launch(tile, flag=flag)
        if not D.forced_ok(c):
            assert rc == ERR_UNSUPPORTED and bool((whole == whole.flatten()[0]).all()) and int(flag) == 0, (c.name, tile, rc)
            continue
        L.check(rc, "yolo_conv_fwd")
        got, untouched = run.split(whole)
        _assert_bits(c, dtype, tile, got, want)
        assert untouched, "%s tile %d: channels outside [off, off + cout) changed" % (c.name, tile)
        assert int(flag) == 0
        outs[tile] = got
    off = _switched_off(L, c)
    if off and "fallback" not in c.name:
        pytest.skip("the default dispatch of %s is switched away from its kernel by %s" % (c.name, ", ".join(off)))
    got, untouched = run.split(run.run(0, flag=flag))
    _assert_bits(c, dtype, 0, got, want)
    assert untouched and int(flag) == 0
    assert all(same_bits(got, o) for o in outs.values())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", D.STATS_CASES, ids=lambda c: c.name)
def test_fused_statistics_are_exact_sums(L, case, dtype):
    """yolo_conv_fwd_stats: z carries the reference bits of the raw convolution, and the partial rows, added per channel in
    fp64, EQUAL the fp64 sums of the stored z and z^2 (integer sums below 2^24: the host test). A clamped pixel of a ragged
    tile counted twice, or a tile's sums lost between iterations of the persistent loop, cannot hide in a tolerance."""
    c = case
    ops, _ = reference(c, dtype, False)
    want = D.stats_value(c, ops).float().to(R.TDT[dtype])
    run = Launch(L, c, dtype, ops)
    off = _switched_off(L, c)
    for tile in _forced(c) + (() if off else (0,)):
        whole, part = run.run_stats(tile)
        z, untouched = run.split(whole)
        _assert_bits(c, dtype, tile, z, want, " (statistics)")
        assert untouched
        rows = part[:, :, :c.cout].double()
        assert bool(torch.isfinite(rows).all()), "%s tile %d: a partial row was not written" % (c.name, tile)
        z64 = z.double().reshape(-1, c.cout)
        got, sums = rows.sum(0), torch.stack([z64.sum(0), (z64 * z64).sum(0)])
        assert torch.equal(got, sums), "%s %s tile %d: channel sums differ at %s: got %s, want %s" % (
            c.name, dtype, tile, (got != sums).nonzero()[:4].tolist(), got[got != sums][:4].tolist(), sums[got != sums][:4].tolist())
    if off:
        pytest.skip("the default dispatch of %s is switched away from its kernel by %s" % (c.name, ", ".join(off)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", D.NAN_CASES, ids=lambda c: c.name)
def test_nan_flag(L, case, dtype):
    """clean data leaves the flag alone; one NaN activation sets bit 1 (the other bits stay) and turns exactly the outputs
    whose window holds it into NaN, in every channel; without YOLO_FLAG_NANCHECK the flag is not written"""
    c = case
    ops, ref = reference(c, dtype, False)
    want = ref.float().to(R.TDT[dtype])
    run = Launch(L, c, dtype, ops)
    xn = run.x.clone()
    h, w = c.H // 2, c.W // 2
    xn[c.B - 1, h, w, c.x_off + 3] = float("nan")
    nan_at = torch.isnan(R.stored(c, R.value(c, dict(ops, x=xn.cpu()), torch.float64)))
    ho, wo = R.res_hw(c)
    holding = lambda i, n: sum(1 for o in range(n) if abs(o * c.stride - i) <= c.k // 2)      # windows along one axis that hold index i
    assert int(nan_at.sum()) == holding(h, ho) * holding(w, wo) * c.cout > 0
    for tile in _forced(c):
        flag = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        assert same_bits(run.split(run.run(tile, flag=flag))[0], want) and int(flag) == 4
        got = run.split(run.run(tile, x=xn, flag=flag))[0]
        assert int(flag) == 6
        assert torch.equal(torch.isnan(got.float()), nan_at) and torch.equal(bits(got)[~nan_at], bits(want)[~nan_at])
        flag.fill_(4)
        run.run(tile, x=xn, flag=flag, nancheck=False)
        assert int(flag) == 4
        run.run(tile, x=xn, flag=None, nancheck=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", D.GAUSS_CASES, ids=lambda c: c.name)
def test_gaussian_cases_within_one_rounding(L, case, dtype):
    """Mish, real scale / shift and a residual against fp64 of the same rounded operands, held to R.GAUSS_TOL (1e-2 bf16,
    2e-3 fp16 of max |reference|). Measured on an MI355X, error over max |reference|, A / B / C / D / E:
    bf16 2.5e-3 / 2.4e-3 / 2.8e-3 / 2.4e-3 / 2.5e-3, fp16 2.9e-4 / 2.9e-4 / 3.6e-4 / 2.8e-4 / 2.7e-4 (every tile the same)"""
    c = case
    ops, ref = reference(c, dtype, True)
    tol = R.GAUSS_TOL[dtype]
    run = Launch(L, c, dtype, ops)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    off = _switched_off(L, c)
    outs = {}
    for tile in _forced(c) + (() if off and c.kind == "fwd" else (0,)):
        got, untouched = run.split(run.run(tile, flag=flag))
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print("%s %s tile %d: max error / max |reference| = %.3g (tolerance %g)" % (c.name, dtype, tile, err, tol))
        assert bool(torch.isfinite(got.float()).all()) and err <= tol, (c.name, dtype, tile, err)
        assert untouched and int(flag) == 0
        outs[tile] = got
    if off:
        pytest.skip("the default dispatch of %s is switched away from its kernel by %s" % (c.name, ", ".join(off)))
    assert all(same_bits(outs[0], o) for o in outs.values())
