"""tests/conv_dma_h16_ref.py on the CPU: what tests/test_gpu_conv_dma_h16.py relies on when it asks conv1_dma_h16,
conv3_dma_h16 and conv3_ws_h16 for bit equality, proved of the reference alone for every integer case and both types:

  operands    activations and residual in +-{1..xmax}, every weight in {-1, 0, +1} and all three values present, scale in
              {1, 2, 0.5}, integer shift; the tables of tests/conv_h16_ref.py keep the operand bits they were merged with
  exactness   K * xmax * 2 + |shift| + |residual| < 2^24, and the fp32 evaluation gives the bits of the fp64 one (with the
              kernels' two order-independent roundings stated, for LeakyReLU)
  sharpness   at least 0.9 of the expected outputs of a bf16 case, and all of an fp16 case, need no rounding at the store
              (LeakyReLU: of the outputs on the identity branch). A condition on the reference: xmax is chosen to meet it
  statistics  (pixels a partial row sums) x max z^2 < 2^24 for the stored z of yolo_conv_fwd_stats: every partial sum of z
              and z^2 is an integer that fp32 holds, whatever the order, so the rows must add up to the fp64 sums exactly
"""
import zlib

import pytest
import torch

from tests import conv_dma_h16_ref as D
from tests import conv_h16_ref as R

DTYPES = ["bf16", "fp16"]
SHARP = {"bf16": 0.9, "fp16": 1.0}


def test_merged_cases_keep_their_operand_bits():
    """the xmax and tile fields must not reseed a case of the tables that were there before them"""
    assert len(R.INT_CASES) == 40 and all((c.xmax, c.tile) == (8, 0) for c in R.INT_CASES + R.GAUSS_CASES)
    for dtype, want in (("bf16", 2188897274), ("fp16", 1919584565)):
        crc = 0
        for c in R.INT_CASES:
            ops = R.operands(c, dtype)
            for k in ("x", "w", "scale", "shift", "r"):
                if ops[k] is not None:
                    crc = zlib.crc32(ops[k].contiguous().view(torch.uint8).numpy().tobytes(), crc)
        assert crc == want, dtype
    c = R.INT_1X1[0]                                                   # and a field that is set does reseed
    assert not torch.equal(R.operands(c, "bf16")["w"], R.operands(c._replace(tile=8), "bf16")["w"])


def test_case_tables_reach_what_they_name():
    named = lambda table, name: next(c for c in table if c.name.endswith(name))
    # ---- routing: every case lands in the kernel of its table, by its forced tile and (default) by tile 0; the fallback cases don't
    where = {"A": "conv1_dma_h16/0", "B": "conv1_dma_h16/1", "C": "conv1_dma_h16/2", "D": "conv3_dma_h16", "E": "conv3_ws_h16"}
    for c in D.INT_CASES + D.GAUSS_CASES:
        fallback = "fallback" in c.name
        assert D.default_kernel(c) == ("conv_patch_h16" if fallback else where[c.name.split("-")[-1 if c.name.startswith("gauss") else 0]]), c.name
        if c.kind == "fwd":
            assert c.default and D.forced_ok(c) == (not fallback), c.name
            # the forced tile picks ONE kernel: tile 8 is conv1_dma_h16 for a 1x1 and conv3_dma_h16 for a 3x3
            assert [D.dma1_ok(c), D.s2_ok(c), D.dma_ok(c), D.ws_eligible(c)].count(True) == (0 if fallback else 1), c.name
        else:
            assert D.s2g_ok(c) == (not fallback) and c.cout % 32 == 0, c.name
        assert c.x_ld % 8 == 0 and c.x_off % 8 == 0 and c.y_off + R.n_out(c) <= c.y_ld and (not c.res or c.r_off + R.n_out(c) <= c.r_ld), c.name
        assert c.x_off + (c.cout if c.kind == "dgrad" else c.cin) <= c.x_ld, c.name
    for t, tile in ((D.INT_A, D.TILE_DMA), (D.INT_B, D.TILE_S2_GEMM), (D.INT_D, D.TILE_DMA), (D.INT_E, D.TILE_WS)):
        assert all(c.tile == tile for c in t)
    for c in (named(D.INT_A, "fallback-y_ld132"), named(D.INT_D, "fallback-y_ld132"), named(D.INT_C, "fallback-dx_ld36")):
        assert c.y_ld % 8 and R.n_out(c) % 8 == 0
    names = [c.name for c in D.INT_CASES + D.GAUSS_CASES + R.INT_CASES + R.GAUSS_CASES]
    assert len(set(names)) == len(names)
    # ---- A: the 1x1 GEMM
    assert [D.kt(c) for c in D.INT_A[:6]] == [4, 5, 6, 7, 8, 9] and {D.kt(c) % D.RING_SLOTS for c in D.INT_A} == {0, 1, 2, 3, 4}
    assert all(c.B * c.H * c.W == 70 for c in D.INT_A[:6])
    blocks = {c.name: D.gemm_blocks(c) for c in D.INT_A}
    assert {b[0] * b[1] for b in blocks.values()} >= {1, 2, 7, 8, 9, 17}
    assert {(n // 8, n % 8) for n in (b[0] * b[1] for b in blocks.values())} >= {(0, 1), (0, 2), (0, 7), (1, 0), (1, 1), (2, 1)}
    assert blocks["A-one-pixel"] == (1, 1, 1) and blocks["A-2-blocks"] == (2, 1, 1) and blocks["A-9-blocks"] == (9, 1, 1)
    assert {c.cout for c in D.INT_A} >= {128, 136, 200, 256}
    c = named(D.INT_A, "cout136-res-view")
    assert c.res == 1 and (c.r_ld, c.r_off) == (144, 8) and c.cout % 128 == 8           # ragged second tile: 8 live channels
    c = named(D.INT_A, "slices")
    assert c.x_off > 0 and c.x_ld > c.x_off + c.cin and c.y_off > 0 and c.y_ld > c.y_off + c.cout
    c = named(D.INT_A, "up2x-two-images")
    assert c.out == R.OUT_UPSAMPLE2X and c.B > 1 and c.y_ld > c.cout
    assert any(c.act == R.ACT_LEAKY and c.res for c in D.INT_A)
    # ---- B: gathered rows
    assert {D.kt(c) for c in D.INT_B} >= {9, 18, 27} and all(c.cout >= 128 for c in D.INT_B)
    assert any((c.B, c.H, c.W) == (3, 2, 2) for c in D.INT_B)
    assert any(R.res_hw(c) == (5, 5) and c.B == 3 for c in D.INT_B)                        # 25 outputs per image
    assert any(D.gemm_blocks(c)[0] == 3 and D.gemm_blocks(c)[2] < 128 for c in D.INT_B)   # 338 pixels
    assert any(1 < R.res_hw(c)[0] != R.res_hw(c)[1] for c in D.INT_B)                     # rectangular: TW = Wo and PC = Ho Wo differ
    assert any(c.cout == 136 and c.res == 1 and c.y_ld > c.cout for c in D.INT_B) and any(c.x_off for c in D.INT_B)
    assert any(c.act == R.ACT_LEAKY for c in D.INT_B)
    # ---- C: the fused stride-2 gradient
    fused = [c for c in D.INT_C if D.s2g_ok(c)]
    assert {D.kt(c) for c in fused} >= {4, 8, 12, 20} and {c.cin for c in fused} == {32, 64}
    assert {D.gemm_blocks(c)[1] for c in fused} == {1, 2}                                # all four classes in one n tile; two n tiles
    assert {(c.B, c.H, c.W) for c in fused} >= {(1, 1, 1), (1, 3, 5), (3, 5, 5), (2, 13, 13)}
    assert {c.res for c in fused} == {0, 1, 2} and any(c.x_off and c.y_off for c in fused)
    # ---- D: the 3x3 LDS-DMA kernel
    assert {c.cin // 32 for c in D.INT_D} >= {1, 2, 3, 8} and {c.cout for c in D.INT_D} >= {72, 128, 136, 256}
    assert {(c.B, c.H, c.W) for c in D.INT_D} >= {(1, 1, 1), (1, 40, 1), (1, 1, 130), (5, 7, 7), (2, 13, 13), (1, 19, 19), (1, 9, 33), (1, 52, 52)}
    assert any(c.out == R.OUT_UPSAMPLE2X for c in D.INT_D) and any(c.act == R.ACT_LEAKY for c in D.INT_D)
    assert any(c.res and c.y_off for c in D.INT_D) and any(c.x_off for c in D.INT_D)
    # ---- E: weights in registers, persistent workgroups
    inst = lambda c: (c.cin, c.stride)
    assert {(c.cin, c.cout, c.stride) for c in D.INT_E} >= ({(32, n, 1) for n in (40, 48, 56, 64)} | {(64, n, 1) for n in (8, 24, 32)}
                                                            | {(32, n, 2) for n in (40, 64)})
    assert {D.ws_tiles(c)[0] for c in D.INT_E} >= {1, 4} and any((c.H, c.W) == (8, 16) and c.B == 1 for c in D.INT_E)
    assert any(c.stride == 2 and (c.H, c.W) == (2, 2) for c in D.INT_E)
    for key in ((32, 1), (64, 1), (32, 2)):
        tiles = [D.ws_tiles(c) for c in D.INT_E if inst(c) == key]
        assert (513, 2, 1) in tiles, key                                                 # one workgroup runs twice
        assert any(t[0] > 1024 and t[1] == 3 and t[2] < D.WS_GRID for t in tiles), key   # three iterations, ragged last round
        assert any(c.res and D.ws_tiles(c)[1] > 1 for c in D.INT_E if inst(c) == key), key    # a residual read past the first iteration
        # and with the fused statistics, whose running sums cross the iterations
        assert {D.ws_tiles(c)[1] for c in D.STATS_CASES if c.tile == D.TILE_WS and inst(c) == key} >= {1, 3}, key
    assert {D.ws_tiles(c)[1] for c in D.STATS_CASES if c.tile == D.TILE_WS} == {1, 2, 3}
    many = [c for c in D.INT_E if D.ws_tiles(c)[0] > D.WS_GRID]
    assert any(c.res for c in many) and any(c.y_off and c.y_ld > c.cout for c in many)
    # ---- statistics and NaN cases
    assert {c.name[0] for c in D.STATS_CASES} == set("ABDE") and {c.name[0] for c in D.NAN_CASES} == set("ABDE")
    assert all(c.act == R.ACT_NONE and not c.res and c.out == R.OUT_NHWC and "fallback" not in c.name for c in D.STATS_CASES + D.NAN_CASES)
    assert [D.default_kernel(c) for c in D.GAUSS_CASES] == [where[k] for k in "ABCDE"]
    assert all(c.res == 1 and (c.kind == "dgrad" or c.act == R.ACT_MISH) for c in D.GAUSS_CASES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", D.INT_CASES, ids=lambda c: c.name)
def test_integer_cases_are_exact_and_sharp(case, dtype):
    c, tdt = case, R.TDT[dtype]
    ops = R.operands(c, dtype)
    n = R.n_out(c)
    # operands as specified, and unchanged by the rounding to the 16-bit type; every weight value present (nothing thinned)
    x, w = ops["x"].float(), ops["w"]
    assert bool(((x.abs() >= 1) & (x.abs() <= c.xmax) & (x == x.round())).all()) and float(x.abs().max()) == c.xmax
    assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0} and torch.equal(w.to(tdt).float(), w)
    assert bool(torch.isin(ops["scale"], torch.tensor([1.0, 2.0, 0.5])).all()) and torch.equal(ops["shift"], ops["shift"].round())
    rmax = 0.0
    if c.res:
        r = ops["r"].float()
        assert bool(((r.abs() >= 1) & (r.abs() <= c.xmax) & (r == r.round())).all())
        rmax = float(r.abs().max())
    # exactness
    bound = R.k_terms(c) * c.xmax * 2 + float(ops["shift"].abs().max()) + rmax
    assert bound < 2 ** 24
    v64 = R.value(c, ops, torch.float64, kernel_steps=True)
    v32 = R.value(c, ops, torch.float32, kernel_steps=True)
    assert float(v64.abs().max()) <= bound
    assert v32.dtype == torch.float32 and torch.equal(v32.double(), v64)
    assert torch.equal(v32.view(torch.int32), v64.float().view(torch.int32))
    if c.act == R.ACT_NONE:                                        # and with no rounding at all: the plain fp64 value
        assert torch.equal(R.value(c, ops, torch.float64), v64)
    assert v64.shape[-1] == n
    # sharpness
    keep = torch.ones_like(v32, dtype=torch.bool)
    if c.act == R.ACT_LEAKY:                                       # the identity branch: scale * conv + shift >= 0
        keep = R.conv_fwd_ref(ops["x"][..., c.x_off:c.x_off + c.cin], w, ops["scale"], ops["shift"], R.ACT_NONE, c.stride) >= 0
    share = float((v32.to(tdt).float() == v32)[keep].float().mean())
    print("%s %s: bound %d, max |value| %g, stored without rounding %.3f" % (c.name, dtype, bound, float(v64.abs().max()), share))
    assert share >= SHARP[dtype]
    # a value of every sign: a dropped term cannot cancel everywhere
    assert bool((v64 > 0).any()) and bool((v64 < 0).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", D.STATS_CASES, ids=lambda c: c.name)
def test_statistics_rows_are_integer_sums(case, dtype):
    c, tdt = case, R.TDT[dtype]
    ops = R.operands(c, dtype)
    z64 = D.stats_value(c, ops)
    assert torch.equal(D.stats_value(c, ops, torch.float32).double(), z64)                    # z itself: any order, the same bits
    z = z64.float().to(tdt).double()                                                          # as stored
    assert torch.equal(z, z.round()) and bool((z > 0).any()) and bool((z < 0).any())
    pixels, zmax = D.stats_row_pixels(c), float(z.abs().max())
    print("%s %s: %d pixels per row, max |z| %g: %.3g of 2^24" % (c.name, dtype, pixels, zmax, pixels * zmax * zmax / 2 ** 24))
    assert pixels * zmax * zmax < 2 ** 24
    assert pixels == (32 * -(-D.ws_tiles(c)[0] // D.WS_GRID) if c.tile == D.TILE_WS else 64)
