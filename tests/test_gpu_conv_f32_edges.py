"""GPU tests (``-m gpu``) of the exact-fp32 convolution kernels against an fp64 convolution of the same fp32 operands, through
the C ABI only, at the smallest shapes that reach every branch of their launch geometry. The bar is the per-element bound of
tests/conv_f32_cases.py (derived from the operands; tests/test_conv_f32_cases_host.py shows on every case that torch's fp32
convolution passes it and three subtly wrong kernels do not). Cases and what each is there for (`why`) are in that module:

  A  conv_igemm_f32 (conv_f32.hip)      forced tiles 1-4, and tile 0 where the heuristic routes here
       a_m25 / m64 / m65 / m129         M against BM (64, 128): less than a block, exactly one, one row more; cout 24 / 64 / 66 / 132
                                        against BN; KT = 1 (the loop never prefetches), 2, 3
       a_straddle_kt9_c255, a_kt27      M tiles straddle images; KT = 9, 27; cout 255 through the scalar NHWC stores
       a_s1_1x40 / 5x1 / 1x1            3x3 stride 1 where whole tap rows / columns are padding
       a_s2_7x9 / 16x16 / 1x1, a_k1s2   3x3 and 1x1 with stride 2 (odd, even and 1 x 1 maps)
       a_small_c{1,3,4}_k*              SMALLC (cin <= 4, one tap per 16-byte chunk), x_ld 4 and 8, x_off 4
       a_xview                          x_ld > cin, x_off 16
       a_head21 / a_head255             head layout, M ragged
       a_epi_*                          y / residual views: multiples of 4 (16-byte path); y_off 2 with y_ld cout + 6, y_ld odd, r_off 1
                                        (each element by element); NHWC and 2x upsampling stores; cout 64 and 66; acts 0 1 2
  B  conv_patch_f32 (conv_f32_v2.hip)   forced tiles 5, 6, 7, and tile 0 on the 3x3 cases (the heuristic's tile 7)
       b_13x13 ... b_52x52              the tile shapes pick_patch_tile chooses: tiles straddling 2, 5 and 7 images, TW = 1 (PC = 3),
                                        H = 1, W > 126, a 256-pixel patch, nblocks 1, < 8, = 8, and > 8 with a remainder; 1, 2, 3 chunks;
                                        cout 24 ... 136 (one to three n tiles)
       b1_m25 / m129 / m338             the 1x1 form: one row of M pixels in tiles of 128; head layout with cout 255
       b_epi_*                          the views, out modes, acts and residual of A; the odd ones run the scalar epilogue
  C  special values                     tiles 4, 6, 7: an Inf, then a NaN, at x pixel 0 channel 0 (where every clamped load points), at an
                                        image's last pixel, on the seam of two images inside one tile, in residual row 0
  D  the flagged kernels' epilogue      YOLO_FLAG_SPLIT_BF16 (tile 0) and YOLO_FLAG_SPLIT_K on an odd NHWC and an odd upsample view
  E  stem3x3_f32 (stem_f32.hip)         one pixel, a ragged last wave (70), a ragged single block (30), exactly one block (256), a ragged
                                        last block (4995 = 19 * 256 + 131); y_ld 32 (LDS-transposed store) and 48 / off 16 (direct store)

Every output buffer is pre-filled with a sentinel and followed by 256 guard bytes of 0xA5: channels outside
[y_off, y_off + cout) and the guard come back unchanged; x, residual and the packed weights are bit-unchanged. Within a case
tiles 1-4 give identical bits, and so do tiles 5-7; image 1 of a batch of 3 equals the image run alone; two runs agree.

Tiles 5-7 against tile 4 where cin == 32 or ksize == 1 (the K order is the same there): identical bits, asserted, with one
exception that is not asserted either way: Mish where conv_igemm_f32 stores element by element (cout % 4 != 0, a y or residual
view that is not a multiple of 4, the head layout). There conv_f32_epilogue applies the activation to the accumulator registers
and the compiler vectorises Mish's n = e (e + 2), n + 2 into v_pk_mul_f32 and v_add_f32: two roundings. conv_patch_f32 always
(and conv_igemm_f32 on its 16-byte path) applies it on the way into the LDS transpose, where n + 2 is contracted into one
v_fma_f32 (e, e + 2, 2): one rounding. The reciprocal's argument differs by an ulp, the result in its last bits (the cases
b_epi_yoff2_c64 / c66 and b_epi_up_odd_c64 / c66; both sides are within the fp64 bound). None and LeakyReLU have no such step.

Measured on an MI355X, the first run: identical on the 16 other comparable cases, different on exactly those four.

Worst err / bound, measured on an MI355X (printed by every test and by the last one; run with -s):
A (conv_igemm_f32) 0.106, B (conv_patch_f32) 0.040, E (stem3x3_f32) 0.068.
Tile 6 as the heuristic's choice needs 640 blocks of 128 channels on a 14 .. 26 row map, beyond the sizes of a quick test: tile 0
of every 3x3 case here is tile 7; tile 6 is forced.
"""
import functools

import pytest
import torch

from tests import conv_f32_cases as K
from tests.conv_f32_launch import GUARD, SENT
from tests.conv_f32_launch import bits as _bits, same_bits as _same_bits, sentinel_buffer as _sentinel_buffer, values as _values, y_shape as _y_shape

pytestmark = pytest.mark.gpu

WORST = {"A": 0.0, "B": 0.0, "E": 0.0}


@pytest.fixture(scope="module")
def L():
    from yolo_for_turbines_amd import _lib
    _lib.lib()                        # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


class Dev:
    """A case's operands on the device, with copies to compare against after every launch."""

    def __init__(self, L, c, ops):
        lib, st = L.lib(), L.current_stream()
        x, w, scale, shift, r = ops
        self.c = c
        self.x, self.scale, self.shift = x.cuda(), scale.cuda(), shift.cuda()
        self.r = r.cuda() if r is not None else None
        wd = w.cuda().contiguous()
        if c.get("stem"):
            self.wp = torch.empty(27 * 32, dtype=torch.float32, device="cuda")
            L.check(lib.yolo_stem_pack(wd.data_ptr(), self.wp.data_ptr(), 32, st), "stem_pack")
        else:
            self.wp = torch.zeros(lib.yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], L.F32), dtype=torch.uint8, device="cuda")
            L.check(lib.yolo_pack_weights(wd.data_ptr(), self.wp.data_ptr(), c["cout"], c["cin"], c["k"], L.F32, st), "pack")
        torch.cuda.synchronize()
        self.x0, self.wp0 = self.x.clone(), self.wp.clone()
        self.r0 = self.r.clone() if self.r is not None else None

    def inputs_unchanged(self):
        return _same_bits(self.x, self.x0) and torch.equal(self.wp, self.wp0) and (self.r is None or _same_bits(self.r, self.r0))


@functools.lru_cache(maxsize=None)
def _dev(L, name):
    c, ops, _, _ = K.shared(name)
    return Dev(L, c, ops)


def _desc(L, c, tile, flags):
    return L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=c["x_ld"], x_off=c["x_off"],
                      y_ld=c["y_ld"], y_off=c["y_off"], r_ld=c["r_ld"], r_off=c["r_off"], act=c["act"], out_mode=c["out"], dtype=L.F32,
                      flags=(L.FLAG_RESIDUAL if c["res"] else 0) | flags, tile=tile)


def _launch(L, dev, tile, flags=None, ws=False):
    """One yolo_conv_fwd[_ws] of dev's case. Asserts the return code, the guards and that the inputs are bit-unchanged; returns
    (the (n, ho, wo, cout) values on the host after the untouched-channel and upsample checks, the NaN flag)."""
    lib, st, c = L.lib(), L.current_stream(), dev.c
    raw, y = _sentinel_buffer(_y_shape(c))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    d = _desc(L, c, tile, L.FLAG_NANCHECK if flags is None else flags)
    if ws:
        need = lib.yolo_conv_workspace_bytes(d)
        assert need > 0
        wsb = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.yolo_conv_fwd_ws(d, dev.x.data_ptr(), dev.wp.data_ptr(), dev.scale.data_ptr(), dev.shift.data_ptr(), L.ptr(dev.r), y.data_ptr(),
                                  wsb.data_ptr(), need, flag.data_ptr(), st)
    else:
        rc = lib.yolo_conv_fwd(d, dev.x.data_ptr(), dev.wp.data_ptr(), dev.scale.data_ptr(), dev.shift.data_ptr(), L.ptr(dev.r), y.data_ptr(),
                               flag.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0, (c["name"], tile, lib.yolo_last_error())
    assert bool((raw[-GUARD:] == 0xA5).all()), (c["name"], tile, "wrote past the output buffer")
    if ws:
        assert bool((wsb[need:] == 0xA5).all()), (c["name"], tile, "wrote past the stated workspace")
    assert dev.inputs_unchanged(), (c["name"], tile, "an input changed")
    return _values(c, y.cpu(), tile), int(flag.item())


def _ratio(name, got):
    _, _, ref, bound = K.shared(name)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not bool((got == SENT).any()), (name, "an output element was not written")
    return float(((got.double() - ref).abs() / bound).max())


def _alone(L, c, ops):
    """Image 1 of a batch, as a case and device operands of its own."""
    x, w, scale, shift, r = ops
    one = dict(c, n=1)
    return Dev(L, one, (x[1:2].contiguous(), w, scale, shift, r[1:2].contiguous() if r is not None else None))


def _run_family(L, name, fam, tiles):
    """Every tile of `tiles` on one case: the bound, identical bits across the tiles, determinism, batch independence."""
    c, ops, _, _ = K.shared(name)
    dev = _dev(L, name)
    out = {}
    for tile in tiles:
        out[tile], flag = _launch(L, dev, tile)
        assert flag == 0, (name, tile, "NaN flag on clean data")
        ratio = _ratio(name, out[tile])
        WORST[fam] = max(WORST[fam], ratio)
        print(f"{name} tile {tile}: err/bound {ratio:.3f}")
        assert ratio <= 1.0, (name, tile, ratio)
    first = tiles[0]
    for tile in tiles[1:]:
        assert _same_bits(out[tile], out[first]), (name, f"tiles {first} and {tile} differ")
    again, _ = _launch(L, dev, tiles[-1])
    assert _same_bits(again, out[tiles[-1]]), (name, "two runs differ")
    if c["n"] == 3:
        alone = _alone(L, c, ops)
        for tile in tiles:
            y1, _ = _launch(L, alone, tile)
            assert _same_bits(y1, out[tile][1:2]), (name, tile, "image 1 depends on its batch")
    return out


# ====================================================================================== A. conv_igemm_f32
@pytest.mark.parametrize("name", [c["name"] for c in K.IGEMM_CASES])
def test_igemm_tiles_against_fp64(L, name):
    c = K.ALL_CASES[name]
    tiles = K.IGEMM_TILES + ((0,) if K.direct_tile(c) == 4 else ())
    _run_family(L, name, "A", tiles)


# ====================================================================================== B. conv_patch_f32
CROSS = {"equal": 0, "differ": []}


def _igemm_stores_16_bytes(c):
    """the `aligned4` branch of conv_f32_epilogue: activation on the way into the LDS transpose"""
    return c["out"] != K.OUT_HEAD and c["cout"] % 4 == 0 and (c["y_ld"] | c["y_off"]) & 3 == 0 and (not c["res"] or (c["r_ld"] | c["r_off"]) & 3 == 0)


@pytest.mark.parametrize("name", [c["name"] for c in K.PATCH_CASES])
def test_patch_tiles_against_fp64(L, name):
    c = K.ALL_CASES[name]
    tiles = K.PATCH_TILES + ((0,) if c["k"] == 3 else ())
    out = _run_family(L, name, "B", tiles)
    if c["cin"] == 32 or c["k"] == 1:
        # one chunk, or one tap: the K order of conv_igemm_f32, and the epilogue is the same expression
        y4, _ = _launch(L, _dev(L, name), 4)
        same = _same_bits(y4, out[5])
        if same:
            CROSS["equal"] += 1
        else:
            CROSS["differ"].append(name)
        print(f"{name}: tiles 5-7 {'equal' if same else 'DIFFER from'} tile 4 bit for bit")
        if not (c["act"] == 2 and not _igemm_stores_16_bytes(c)):     # (Mish in conv_igemm_f32's register path: see the module docstring)
            assert same, (name, "tiles 5-7 differ from tile 4 although the K order is the same")


# ====================================================================================== C. special values
def _plants(c):
    """(label, tensor, index, the (n, ho, wo, cout) mask of the outputs that depend on it)"""
    ho, wo = K.out_hw(c)
    assert c["s"] == 1 and c["res"] and c["n"] >= 2

    def around(n, hi, wi):
        m = torch.zeros((c["n"], ho, wo, c["cout"]), dtype=torch.bool)
        p = c["k"] // 2
        m[n, max(hi - p, 0):hi + p + 1, max(wi - p, 0):wi + p + 1] = True
        return m

    one = torch.zeros((c["n"], ho, wo, c["cout"]), dtype=torch.bool)
    one[0, 0, 0, 3] = True
    return [("x pixel 0 channel 0", "x", (0, 0, 0, c["x_off"]), around(0, 0, 0)),
            ("last pixel of image 1", "x", (1, c["h"] - 1, c["w"] - 1, c["x_off"] + 5), around(1, c["h"] - 1, c["w"] - 1)),
            ("seam: first row of image 1", "x", (1, 0, c["w"] // 2, c["x_off"] + 7), around(1, 0, c["w"] // 2)),
            ("residual row 0", "r", (0, 0, 0, c["r_off"] + 3), one)]


@pytest.mark.parametrize("tile", [4, 6, 7])
@pytest.mark.parametrize("name", ["b_epi_vec4_c64", "a_epi_vec4_c64", "b_epi_roff1_c64"])
def test_inf_and_nan_reach_exactly_what_depends_on_them(L, name, tile):
    """3x3 (two tiles of 14 rows over three images of 7: the first straddles images 0 and 1) and 1x1 (all 75 pixels in one tile);
    the 16-byte and the element-by-element epilogue. LeakyReLU: an Inf stays an Inf, so only a NaN sets the flag."""
    c, ops, _, _ = K.shared(name)
    clean, flag = _launch(L, _dev(L, name), tile)
    assert flag == 0 and bool(torch.isfinite(clean).all())
    for label, which, idx, mask in _plants(c):
        for value in (float("inf"), float("nan")):
            x, w, scale, shift, r = (t.clone() if t is not None else None for t in ops)
            (x if which == "x" else r)[idx] = value
            dev = Dev(L, c, (x, w, scale, shift, r))
            got, flag = _launch(L, dev, tile)
            assert torch.equal(~torch.isfinite(got), mask), (name, tile, label, value, "not exactly the dependent outputs are non-finite")
            assert torch.equal(_bits(got)[~mask], _bits(clean)[~mask]), (name, tile, label, value, "an independent output changed")
            has_nan = bool(torch.isnan(got).any())
            assert has_nan == (value != value)
            assert flag == (2 if has_nan else 0), (name, tile, label, value, flag)
            if has_nan:
                got_off, flag_off = _launch(L, dev, tile, flags=0)
                assert flag_off == 0 and _same_bits(got_off, got), (name, tile, label, "YOLO_FLAG_NANCHECK off")


# ====================================================================================== D. the flagged kernels
@pytest.mark.parametrize("name", [c["name"] for c in K.FLAGGED_CASES])
def test_flagged_kernels_on_odd_views(L, name):
    """YOLO_FLAG_SPLIT_BF16 (tile 0) and YOLO_FLAG_SPLIT_K on y / residual views that are not multiples of 4, held to the bars of
    tests/test_gpu_split3.py and tests/test_gpu_splitk.py: max|err| / max|y| against fp64 at most twice that of tile 4 on the same
    operands, which itself is below 3e-6. Tile 4 is also held to the per-element bound."""
    _, _, ref, _ = K.shared(name)
    dev = _dev(L, name)

    def rel(y):
        return float((y.double() - ref).abs().max() / ref.abs().max())

    exact, flag = _launch(L, dev, 4)
    assert flag == 0 and _ratio(name, exact) <= 1.0
    e_exact = rel(exact)
    assert e_exact < 3e-6
    for label, flags, ws in (("split3", L.FLAG_SPLIT_BF16, False), ("split-K", L.FLAG_SPLIT_K, True)):
        y, flag = _launch(L, dev, 0, flags=flags | L.FLAG_NANCHECK, ws=ws)
        e = rel(y)
        print(f"{name} {label}: {e:.3e}  exact {e_exact:.3e}  ratio {e / e_exact:.2f}")
        assert flag == 0 and e <= 2 * e_exact, (name, label, e, e_exact)
        again, _ = _launch(L, dev, 0, flags=flags | L.FLAG_NANCHECK, ws=ws)
        assert _same_bits(again, y), (name, label, "two runs differ")


# ====================================================================================== E. stem3x3_f32
def _stem(L, dev, c, expect_rc=0):
    lib, st = L.lib(), L.current_stream()
    raw, y = _sentinel_buffer((c["n"], c["h"], c["w"], c["y_ld"]))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.yolo_stem_fwd(dev.x.data_ptr(), dev.wp.data_ptr(), dev.scale.data_ptr(), dev.shift.data_ptr(), y.data_ptr(), c["n"], c["h"], c["w"],
                           32, c["y_ld"], c["y_off"], c["act"], L.F32, flag.data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == expect_rc, (c["name"], rc, lib.yolo_last_error())
    assert bool((raw[-GUARD:] == 0xA5).all()) and dev.inputs_unchanged(), c["name"]
    return y.cpu(), int(flag.item())


@pytest.mark.parametrize("name", [c["name"] for c in K.STEM_CASES])
def test_stem_against_fp64(L, name):
    c = K.ALL_CASES[name]
    dev = _dev(L, name)
    y, flag = _stem(L, dev, c)
    got = _values(c, y)
    ratio = _ratio(name, got)
    WORST["E"] = max(WORST["E"], ratio)
    print(f"{name}: err/bound {ratio:.3f}")
    assert flag == 0 and ratio <= 1.0, (name, ratio, flag)
    again, _ = _stem(L, dev, c)
    assert _same_bits(again, y), (name, "two runs differ")


@pytest.mark.parametrize("layout", K.STEM_LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 5, 3), (3, 37, 45)])
def test_stem_special_values(L, shape, layout):
    """Flag bit 1 (value 1) for a NaN input element anywhere, the last pixel included, and bit 2 (value 2) for the NaN outputs it
    makes; an Inf in a corner reaches its 2 x 2 neighbourhood only and sets neither (no activation: it stays an Inf)."""
    c = K.stem_case(shape, layout, 0)
    n, h, w = shape
    ops = K.operands(c)
    clean = _values(c, _stem(L, Dev(L, c, ops), c)[0])
    for idx in ((0, 0, 0, 0), (n - 1, 2, h - 1, w - 1), (n - 1, 1, h // 2, w // 2), (0, 2, 0, w - 1)):
        x = ops[0].clone()
        x[idx] = float("nan")
        y, flag = _stem(L, Dev(L, c, (x,) + ops[1:]), c)
        got = _values(c, y)
        mask = torch.zeros(got.shape, dtype=torch.bool)
        mask[idx[0], max(idx[2] - 1, 0):idx[2] + 2, max(idx[3] - 1, 0):idx[3] + 2] = True
        assert flag == 3, (c["name"], idx, flag)
        assert torch.equal(torch.isnan(got), mask) and torch.equal(_bits(got)[~mask], _bits(clean)[~mask]), (c["name"], idx)
    x = ops[0].clone()
    x[0, 1, 0, 0] = float("inf")
    got = _values(c, _stem(L, Dev(L, c, (x,) + ops[1:]), c)[0])
    mask = torch.zeros(got.shape, dtype=torch.bool)
    mask[0, :2, :2] = True
    assert torch.equal(torch.isinf(got), mask) and not bool(torch.isnan(got).any())
    assert torch.equal(_bits(got)[~mask], _bits(clean)[~mask])
    y, flag = _stem(L, Dev(L, c, (x,) + ops[1:]), c)
    assert flag == 0


@pytest.mark.parametrize("y_ld,y_off", [(34, 0), (48, 2), (33, 1)])
def test_stem_refuses_views_that_are_not_multiples_of_4(L, y_ld, y_off):
    c = dict(K.stem_case((2, 5, 3), (y_ld, y_off), 1))
    y, flag = _stem(L, Dev(L, c, K.operands(c)), c, expect_rc=-2)
    assert bool((y == SENT).all()) and flag == 0, "a refused call wrote something"


def test_report_worst_ratios():
    """(last in the module) the largest err / bound of each family over the cases that ran, for the module docstring"""
    print("worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    print(f"tiles 5-7 against tile 4: equal on {CROSS['equal']} cases, differ on {CROSS['differ']}")
