"""GPU tests (``-m gpu``) of conv1_rs_f32 (tile 12) and of Winograd F(2x2, 3x3) (wino_pack_f32, wino_xform_f32, conv_wino_f32 = tile
13, conv_wino2_f32 = tile 14; also as the fp32 input gradient on yolo_pack_weights_dgrad(flip = 1)) against an fp64 convolution of
the same fp32 operands, through the C ABI only, at the smallest shapes that reach every branch of their launch geometry. Cases,
what each is there for (`why`), the reference and both bars are in tests/conv_wino_rs_cases.py; tests/test_conv_wino_rs_cases_host.py
shows on the CPU that the reference alone meets the bars, that three subtly wrong kernels do not, and that the tables hold the
geometry they name.

  integer cases   bit equality with the fp64 reference (every geometry case): any error, however small against the largest
                  output, in any single element fails
  Gaussian cases  the per-element bound, every activation, real scale / shift

  R  conv1_rs_f32      M = 1 / 31 / 32 / 33; fewer tiles than workgroups (look-ahead from the zero page); 1, 2, 3 and 8 channel groups;
                       cout 1024 with exactly `slots` and `slots + 1` tiles per workgroup on the 3-slot (K 256 / 384) and the 2-slot
                       ring (K 512), and with one more, ragged tile for workgroup 0; 257 tiles on 256 workgroups; tiles straddling
                       images with the 2x upsampling store; views that are multiples of 4 and not of 8; where tile 0 lands (1 x 2048:
                       here; 1 x 2047 or a residual: tile 4); y_off 2: refused, nothing written, tile 0 stores the reference
  W  F(2x2)            tiles 13 and 14, and tile 0 with the workspace where yolo_conv_pick_tile says 13 (bits of tile 14 up to
                       YOLO_WINO2_MAXPIX pixels, of tile 13 beyond): 1x1, 1x9, 9x1, 2x2, 3x3, 4x5, 13x13 maps; T = 3 / 63 / 64 / 65 with the
                       tiles of a block in different images; n_mt 1 / 8 / 9; cin 4 / 32 / 96 / 160; cout 4 / 60 / 64 / 68 / 132; views;
                       the 13 x 13 512 -> 1024 layer; y_off 2: refused by 13 / 14, run directly by tile 0
  G  input gradient    forward cout 84 and 33 with finite non-zero garbage in the padded dz channels and behind the weight tensor (the
                       result does not change with it), forward cin 64 and 96, accumulation into dx in place

Every launch: the output in a sentinel-filled buffer with 256 guard bytes of 0xA5, channels outside [y_off, y_off + cout) unchanged,
the four pixels of an upsampling store equal; the workspace exactly yolo_conv_workspace_bytes, pre-filled with 0x7F, guard bytes
behind it; the packed weights in a guarded buffer; x, residual and packed weights bit-unchanged; NaN flag 0. Per case two runs give
the same bits, and image 1 of a batch of 3 equals that image run alone.

Special values (LeakyReLU, finite data elsewhere; an Inf, then a NaN, at x pixel 0 channel 0, at the last pixel of an image, at the
last pixel of the ragged last tile, in residual row 0). conv1_rs_f32: exactly that pixel's outputs are non-finite, all others keep
the bits of the clean run. F(2x2): every output whose 3x3 window holds the pixel is non-finite, every output outside the 2x2 tiles
whose 4x4 input tile holds it keeps its bits; flag bit 2 is set if and only if a NaN was stored. What the rest of those tiles holds
is not asserted, only recorded (below).

Measured on an MI355X, the first run (printed by every test and by the last one; run with -s). A record, not a bar.
Every integer case: the bits of the fp64 reference on tiles 12, 13, 14 and on tile 0 wherever it was compared.
Worst err / bound over the Gaussian cases: conv1_rs_f32 0.009; F(2x2) tile 13 0.003, tile 14 0.003, tile 0 0.002; input gradient tile 13
0.001, tile 14 0.001. (The bound is an a-priori one and grows with K; the error of a chain of 256 to 512 roundings grows with its root.)
Where tile 0 lands is observed on the Gaussian cases only: there the two candidate tiles are first asserted to differ in bits (on an
integer case every tile stores the reference's bits, so the comparison could not tell them apart). Observed: rg_route_2048 stored the
bits of tile 12 and not of tile 4, rg_route_2047 and rg_route_res those of tile 4 and not of tile 12; with the workspace wg_leaky_res,
wg_mish_res and gg_co84_ci96_acc stored those of tile 14 and not of tile 13, wg_20x20 those of tile 13 and not of tile 14. Worst err /
bound of the three 1x1 route cases: tile 4 0.009, tile 12 0.010.
Special values, tiles 13 and 14 alike: an Inf in x makes NaN of 254 of the 256 outputs that depend on pixel 0, 146 of 256 at an image's
last pixel, 447 of 576 at an inner pixel (the output transform subtracts infinities; conv1_rs_f32 keeps all of them Inf), and sets the
flag. In the rest of the 2x2 tiles whose input tile holds the pixel (320 and 448 outputs) NOTHING was non-finite: the rows of A^T
and B^T are such that a transform point holding input row i enters output row a only for i in a .. a + 2, so the non-finite
outputs are exactly the 3x3 dependence, as in the direct kernels; only Inf against NaN differs.
"""
import functools

import pytest
import torch

from tests import conv_wino_rs_cases as W
from tests.conv_f32_launch import GUARD, SENT, bits, same_bits, sentinel_buffer, values, y_shape
from tests.conv_h16_launch import ERR_UNSUPPORTED, switches

pytestmark = pytest.mark.gpu

WORST = {}
REST = {}
ROUTES = []


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _guarded(nbytes, fill):
    """`nbytes` of `fill` with GUARD bytes of 0xA5 behind them"""
    raw = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    raw[nbytes:] = 0xA5
    return raw


class Dev:
    """A case's operands on the device, the weights packed into a guarded buffer, with copies to compare against after every launch."""

    def __init__(self, L, c, ops):
        lib, st = L.lib(), L.current_stream()
        self.c = c
        self.x, self.scale, self.shift = ops["x"].cuda(), ops["scale"].cuda(), ops["shift"].cuda()
        self.r = ops["r"].cuda() if ops["r"] is not None else None
        if c["dgrad"]:
            wd = ops["w_mem"].cuda()                                   # the weights with garbage behind them, one allocation
            self.nwp = lib.yolo_packed_dgrad_bytes(c["klim"], c["cout"], 3, 1, L.F32)
            self.wp = _guarded(self.nwp, 0)
            L.check(lib.yolo_pack_weights_dgrad(wd.data_ptr(), self.wp.data_ptr(), c["klim"], c["cout"], 3, 1, L.F32, st), "pack dgrad")
        else:
            wd = ops["w"].cuda().contiguous()
            self.nwp = lib.yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], L.F32)
            self.wp = _guarded(self.nwp, 0)
            L.check(lib.yolo_pack_weights(wd.data_ptr(), self.wp.data_ptr(), c["cout"], c["cin"], c["k"], L.F32, st), "pack")
        torch.cuda.synchronize()
        assert self.nwp > 0 and bool((self.wp[self.nwp:] == 0xA5).all()), (c["name"], "the pack wrote past its stated size")
        self.x0, self.wp0 = self.x.clone(), self.wp.clone()
        self.r0 = self.r.clone() if self.r is not None else None

    def inputs_unchanged(self, inplace):
        return same_bits(self.x, self.x0) and torch.equal(self.wp, self.wp0) and (self.r is None or inplace or same_bits(self.r, self.r0))


@functools.lru_cache(maxsize=None)
def _dev(L, name):
    c, ops, _, _ = W.shared(name)
    return Dev(L, c, ops)


def _desc(L, c, tile, flags):
    return L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=1, x_ld=c["x_ld"], x_off=c["x_off"],
                      y_ld=c["y_ld"], y_off=c["y_off"], r_ld=c["r_ld"], r_off=c["r_off"], act=c["act"], out_mode=c["out"], dtype=L.F32,
                      flags=(L.FLAG_RESIDUAL if c["res"] else 0) | flags, tile=tile)


def _launch(L, dev, tile, flags=None, expect_rc=0):
    """One yolo_conv_fwd_ws of dev's case with the workspace yolo_conv_workspace_bytes states (none where it states 0). Asserts the
    return code, the guards and that the inputs are bit-unchanged; returns ((n, h, w, cout) on the host after the untouched-channel
    and upsample checks, the NaN flag). A refused launch (expect_rc) must have written nothing: returns (None, flag).
    An accumulating input gradient runs in place: the output buffer holds dx and is the residual."""
    lib, st, c = L.lib(), L.current_stream(), dev.c
    raw, y = sentinel_buffer(y_shape(c))
    inplace = c["dgrad"] and c["res"]
    if inplace:
        assert y.shape == dev.r.shape
        y.copy_(dev.r)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    d = _desc(L, c, tile, L.FLAG_NANCHECK if flags is None else flags)
    need = lib.yolo_conv_workspace_bytes(d)
    wsb = _guarded(need, 0x7F) if need else None
    rptr = y.data_ptr() if inplace else L.ptr(dev.r)
    rc = lib.yolo_conv_fwd_ws(d, dev.x.data_ptr(), dev.wp.data_ptr(), dev.scale.data_ptr(), dev.shift.data_ptr(), rptr, y.data_ptr(),
                              wsb.data_ptr() if need else 0, need, flag.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == expect_rc, (c["name"], tile, rc, lib.yolo_last_error())
    assert bool((raw[-GUARD:] == 0xA5).all()), (c["name"], tile, "wrote past the output buffer")
    assert wsb is None or bool((wsb[need:] == 0xA5).all()), (c["name"], tile, "wrote past the stated workspace")
    assert dev.inputs_unchanged(inplace), (c["name"], tile, "an input changed")
    if rc != 0:
        assert bool((y == SENT).all()) and int(flag.item()) == 0, (c["name"], tile, "a refused call wrote something")
        return None, int(flag.item())
    return values(c, y.cpu(), tile), int(flag.item())


def _check(name, got, tile, fam):
    """the case's bar: the bits of the reference, or the per-element bound"""
    c, _, ref, bound = W.shared(name)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if c["kind"] == "int":
        wrong = bits(got) != bits(ref)
        assert not bool(wrong.any()), (name, tile, "%d of %d elements differ from the reference, the first at %s"
                                       % (int(wrong.sum()), wrong.numel(), wrong.nonzero()[0].tolist()))
        return
    assert not bool((got == SENT).any()), (name, tile, "an output element was not written")
    ratio = float(((got.double() - ref).abs() / bound).max())
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    print(f"{name} tile {tile}: err/bound {ratio:.3f}")
    assert ratio <= 1.0, (name, tile, ratio)


def _alone(L, c, ops):
    """Image 1 of a batch, as a case and device operands of its own."""
    one = dict(ops, x=ops["x"][1:2].contiguous(), r=ops["r"][1:2].contiguous() if ops["r"] is not None else None)
    return Dev(L, dict(c, n=1), one)


def _run(L, name, tiles, fam):
    """Every tile of `tiles` on one case: the bar, the NaN flag, determinism, batch independence."""
    c, ops, _, _ = W.shared(name)
    dev = _dev(L, name)
    out = {}
    for tile in tiles:
        out[tile], flag = _launch(L, dev, tile)
        assert flag == 0, (name, tile, "NaN flag on clean data")
        _check(name, out[tile], tile, "%s tile %d" % (fam, tile))
    for tile in tiles:
        again, _ = _launch(L, dev, tile)
        assert same_bits(again, out[tile]), (name, tile, "two runs differ")
    if c["n"] == 3:
        alone = _alone(L, c, ops)
        for tile in tiles:
            y1, _ = _launch(L, alone, tile)
            assert same_bits(y1, out[tile][1:2]), (name, tile, "image 1 depends on its batch")
    return out


def _observe_route(name, y0, out, candidates, expect):
    """Which of the forced tiles `candidates` stored the bits tile 0 stored, and whether that is `expect`. On a Gaussian case the
    candidates must differ from each other in bits, so the answer is an observation and goes into ROUTES; on an integer case every
    tile stores the reference's bits and the comparison only says that tile 0 did too."""
    c = W.ALL_CASES[name]
    if c["kind"] == "gauss":
        a, b = candidates
        assert not same_bits(out[a], out[b]), (name, f"tiles {a} and {b} store the same bits: the comparison cannot tell them apart")
    seen = [t for t in candidates if same_bits(y0, out[t])]
    if c["kind"] == "gauss":
        ROUTES.append(f"{name}: tile 0 stored the bits of tile {seen}")
        print(ROUTES[-1])
        assert seen == [expect], (name, f"tile 0 stored the bits of {seen}, the routing rule says tile {expect}")
    else:
        assert expect in seen, (name, f"tile 0 does not store the bits of tile {expect}")


def _tile0_with_workspace(L, name, out):
    """Tile 0 with the workspace where yolo_conv_pick_tile says 13: the bits of tile 14 up to wino2_maxpix pixels, of tile 13 beyond
    (the switch as yolo_switches_describe reports it)."""
    c = W.ALL_CASES[name]
    picked = L.lib().yolo_conv_pick_tile(_desc(L, c, 0, 0))
    if picked != W.TILE_WINO:
        assert W.tile0_lands(c) not in (W.TILE_WINO, W.TILE_WINO2) or switches(L)["YOLO_NO_WINOGRAD"], (name, picked)
        return
    y0, flag = _launch(L, _dev(L, name), 0)
    assert flag == 0
    _check(name, y0, 0, "F(2x2) tile 0")
    expect = W.TILE_WINO2 if c["h"] * c["w"] <= switches(L)["YOLO_WINO2_MAXPIX"] else W.TILE_WINO
    _observe_route(name, y0, out, (W.TILE_WINO, W.TILE_WINO2), expect)


# ====================================================================================== R. conv1_rs_f32
@pytest.mark.parametrize("name", W.names(W.RS_CASES + W.RS_GAUSS))
def test_conv1_rs_against_fp64(L, name):
    _run(L, name, (W.TILE_RS,), "conv1_rs_f32")


@pytest.mark.parametrize("name", W.names(W.RS_ROUTE_CASES + W.RS_ROUTE_GAUSS))
def test_conv1_rs_where_tile0_lands(L, name):
    """The integer cases hold the three tiles to the reference's bits on these shapes; the Gaussian copies, on which tiles 4 and 12
    differ in bits, show which of the two tile 0 ran."""
    c = W.ALL_CASES[name]
    out = _run(L, name, (W.TILE_REG64, 0, W.TILE_RS), "1x1 route")
    lands = W.tile0_lands(c)
    if lands == W.TILE_RS and switches(L)["YOLO_NO_CONV1_RS"]:
        return                                                          # the A/B switch takes the default away from this kernel
    _observe_route(name, out[0], out, (W.TILE_REG64, W.TILE_RS), lands)


@pytest.mark.parametrize("name", W.names(W.RS_REFUSED))
def test_conv1_rs_refuses_a_view_that_is_no_multiple_of_4(L, name):
    dev = _dev(L, name)
    _launch(L, dev, W.TILE_RS, expect_rc=ERR_UNSUPPORTED)
    y0, flag = _launch(L, dev, 0)
    assert flag == 0
    _check(name, y0, 0, "direct")


# ====================================================================================== W. F(2x2)
@pytest.mark.parametrize("name", W.names(W.WINO_CASES + W.WINO_GAUSS))
def test_winograd_f2x2_against_fp64(L, name):
    out = _run(L, name, (W.TILE_WINO, W.TILE_WINO2), "F(2x2)")
    _tile0_with_workspace(L, name, out)


@pytest.mark.parametrize("name", W.names(W.WINO_REFUSED))
def test_winograd_f2x2_refuses_a_view_that_is_no_multiple_of_4(L, name):
    dev = _dev(L, name)
    for tile in (W.TILE_WINO, W.TILE_WINO2):
        _launch(L, dev, tile, expect_rc=ERR_UNSUPPORTED)
    y0, flag = _launch(L, dev, 0)
    assert flag == 0
    _check(name, y0, 0, "direct")


# ====================================================================================== G. the input gradient
@pytest.mark.parametrize("name", W.names(W.DGRAD_CASES))
def test_winograd_input_gradient_against_fp64(L, name):
    """dz's padded channels and the floats behind the weight tensor hold finite non-zero garbage: with klim right both meet zeros
    only. A second fill of both must give the same bits."""
    c, ops, _, _ = W.shared(name)
    out = _run(L, name, (W.TILE_WINO, W.TILE_WINO2), "dgrad")
    _tile0_with_workspace(L, name, out)
    other = W.operands(c, garbage=1)
    nw, klim = c["klim"] * c["cout"] * 9, c["klim"]
    assert torch.equal(other["x"][..., :klim], ops["x"][..., :klim]) and torch.equal(other["w_mem"][:nw], ops["w_mem"][:nw])
    assert not bool((other["x"][..., klim:] == ops["x"][..., klim:]).all()) and not bool((other["w_mem"][nw:] == ops["w_mem"][nw:]).all())
    dev = Dev(L, c, other)
    assert torch.equal(dev.wp, _dev(L, name).wp), (name, "the packed gradient filters depend on what lies behind the weights")
    for tile in (W.TILE_WINO, W.TILE_WINO2):
        got, flag = _launch(L, dev, tile)
        assert flag == 0 and same_bits(got, out[tile]), (name, tile, "the result depends on the garbage")


# ====================================================================================== special values
def _plant_and_compare(L, name, tile, plants, fam):
    c, ops, _, _ = W.shared(name)
    clean, flag = _launch(L, _dev(L, name), tile)
    assert flag == 0 and bool(torch.isfinite(clean).all())
    for label, which, idx, must, may in plants:
        for value in (float("inf"), float("nan")):
            mod = dict(ops)
            mod[which] = ops[which].clone()
            mod[which][idx] = value
            got, flag = _launch(L, Dev(L, c, mod), tile)
            bad = ~torch.isfinite(got)
            assert bool(bad[must].all()), (name, tile, label, value, "an output that depends on the value is finite")
            assert not bool(bad[~may].any()) and torch.equal(bits(got)[~may], bits(clean)[~may]), (name, tile, label, value, "an independent output changed")
            has_nan = bool(torch.isnan(got).any())
            assert flag == (2 if has_nan else 0), (name, tile, label, value, flag)
            if value != value:
                assert has_nan
            rest = may & ~must
            key = f"{fam} tile {tile}, {'NaN' if value != value else 'Inf'} at {label}"
            REST[key] = "%d dependent outputs, %d of them NaN" % (int(must.sum()), int(torch.isnan(got)[must].sum()))
            if bool(rest.any()):
                REST[key] += "; the rest of its tiles: %d of %d non-finite" % (int(bad[rest].sum()), int(rest.sum()))
            print(key + ": " + REST[key])


def test_conv1_rs_inf_and_nan_reach_exactly_their_pixel(L):
    """rg_leaky_res: 70 pixels in three tiles, the last ragged (6 pixels: its last pixel is read 27 times); K = 384, two groups"""
    name = "rg_leaky_res"
    c = W.ALL_CASES[name]
    shape = (c["n"], c["h"], c["w"], c["cout"])

    def pixel(n, hi, wi):
        m = torch.zeros(shape, dtype=torch.bool)
        m[n, hi, wi] = True
        return m

    one = torch.zeros(shape, dtype=torch.bool)
    one[0, 0, 0, 3] = True
    last = (c["n"] - 1, c["h"] - 1, c["w"] - 1)
    assert W.rs_geometry(c)["last_pixels"] < 32
    plants = [("x pixel 0 channel 0", "x", (0, 0, 0, c["x_off"]), pixel(0, 0, 0)),
              ("last pixel of image 0", "x", (0, c["h"] - 1, c["w"] - 1, c["x_off"] + 5), pixel(0, c["h"] - 1, c["w"] - 1)),
              ("last pixel of the ragged last tile", "x", last + (c["x_off"] + c["cin"] - 1,), pixel(*last)),
              ("residual row 0", "r", (0, 0, 0, c["r_off"] + 3), one)]
    _plant_and_compare(L, name, W.TILE_RS, [(lab, which, idx, m, m) for lab, which, idx, m in plants], "conv1_rs_f32")


@pytest.mark.parametrize("tile", [W.TILE_WINO, W.TILE_WINO2])
def test_winograd_inf_and_nan_reach_their_window_and_stay_in_their_tiles(L, tile):
    """wg_leaky_res: three 13 x 13 images, 147 tiles in three blocks"""
    name = "wg_leaky_res"
    c = W.ALL_CASES[name]
    shape = (c["n"], c["h"], c["w"], c["cout"])

    def window(n, hi, wi):
        m = torch.zeros(shape, dtype=torch.bool)
        m[n, max(hi - 1, 0):hi + 2, max(wi - 1, 0):wi + 2] = True
        return m

    def tiles_holding(n, hi, wi):
        """the 2x2 output tiles whose 4x4 input tile (rows 2 ty - 1 .. 2 ty + 2) holds the pixel"""
        m = torch.zeros(shape, dtype=torch.bool)
        for ty in range((c["h"] + 1) // 2):
            for tx in range((c["w"] + 1) // 2):
                if 2 * ty - 1 <= hi <= 2 * ty + 2 and 2 * tx - 1 <= wi <= 2 * tx + 2:
                    m[n, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = True
        return m

    one = torch.zeros(shape, dtype=torch.bool)
    one[0, 0, 0, 3] = True
    hl, wl = c["h"] - 1, c["w"] - 1
    plants = [("x pixel 0 channel 0", "x", (0, 0, 0, c["x_off"]), window(0, 0, 0), tiles_holding(0, 0, 0)),
              ("last pixel of image 1", "x", (1, hl, wl, c["x_off"] + 5), window(1, hl, wl), tiles_holding(1, hl, wl)),
              ("an inner pixel of image 2", "x", (2, 6, 5, c["x_off"] + 9), window(2, 6, 5), tiles_holding(2, 6, 5)),
              ("residual row 0", "r", (0, 0, 0, c["r_off"] + 3), one, one)]
    for _, _, _, must, may in plants:
        assert bool((may | ~must).all())
    _plant_and_compare(L, name, tile, plants, "F(2x2)")


def test_report_worst_ratios():
    """(last in the module) the largest err / bound of each family over the Gaussian cases that ran, for the module docstring"""
    print("worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    for line in ROUTES:
        print(line)
    for k, v in sorted(REST.items()):
        print(f"{k}: {v}")
