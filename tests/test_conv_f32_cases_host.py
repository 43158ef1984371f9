"""The cases of tests/conv_f32_cases.py on the host (nothing is launched): the per-element bound lets torch's own fp32
convolution pass and catches three subtly wrong kernels on every case; the Python restatement of pick_patch_tile and of the
launch numbers equals yolo_conv_patch_plan; every address conv_patch_f32 forms lies inside its tensor or LDS buffer; the
tables hold the edges they name."""
import ctypes as C

import pytest
import torch

from tests import conv_f32_cases as K


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _desc(L, n, h, w, cin, cout, k, s=1):
    return L.ConvDesc(n=n, h=h, w=w, cin=cin, cout=cout, ksize=k, stride=s, x_ld=cin, y_ld=cout)


def _lib_plan(L, d, tile):
    out = (C.c_int32 * 8)()
    rc = L.lib().yolo_conv_patch_plan(d, tile, out)
    return rc, list(out)


def test_symbol_and_version(built):
    assert "yolo_conv_patch_plan" in built.EXPORTS
    assert built.lib().yolo_version() >= 104


def test_plan_refuses_what_the_kernel_does_not_run(built):
    L = built
    ok = _desc(L, 2, 13, 13, 64, 128, 3)
    for tile in (0, 1, 4, 8, 15):
        assert _lib_plan(L, ok, tile)[0] == -1, tile
    assert _lib_plan(L, _desc(L, 2, 13, 13, 64, 128, 3, s=2), 5)[0] == -2
    assert _lib_plan(L, _desc(L, 2, 13, 13, 3, 128, 3), 6)[0] == -2
    assert _lib_plan(L, _desc(L, 2, 13, 13, 48, 128, 3), 7)[0] == -2
    assert L.lib().yolo_conv_patch_plan(None, 5, (C.c_int32 * 8)()) == -1 and L.lib().yolo_conv_patch_plan(ok, 5, None) == -1
    assert _lib_plan(L, ok, 5)[0] == 0


def test_geometry_restatement_equals_the_library(built):
    """pick_patch_tile and the derived launch numbers, for all (H, W) in [1, 64]^2 plus W in {126, 127, 130, 208, 416}, on the three
    tiles, and for every patch case."""
    L = built
    widths = list(range(1, 65)) + [126, 127, 130, 208, 416]
    checked = 0
    for h in range(1, 65):
        for w in widths:
            for tile, n, cin, cout in ((5, 2, 32, 66), (6, 3, 64, 136), (7, 1, 96, 64)):
                rc, got = _lib_plan(L, _desc(L, n, h, w, cin, cout, 3), tile)
                assert rc == 0 and got == K.plan_out8(K.patch_plan(n, h, w, cin, cout, 3, tile)), (h, w, tile, got)
                checked += 1
    assert checked == 64 * 69 * 3
    for m in (1, 25, 127, 128, 129, 338, 4097):
        for tile in K.PATCH_TILES:
            rc, got = _lib_plan(L, _desc(L, 1, 1, m, 32, 255, 1), tile)
            assert rc == 0 and got == K.plan_out8(K.patch_plan(1, 1, m, 32, 255, 1, tile)), (m, tile, got)
    for c in K.PATCH_CASES:
        for tile in K.PATCH_TILES:
            rc, got = _lib_plan(L, _desc(L, c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"]), tile)
            assert rc == 0 and got == K.plan_out8(K.patch_plan(c["n"], c["h"], c["w"], c["cin"], c["cout"], c["k"], tile)), (c["name"], tile)


@pytest.fixture(scope="module")
def audits(built):
    """(plan, stats) of the address audit for every patch case (the flagged 3x3 / 1x1 cases too: tile 0 may run them here) and tile."""
    L = built
    res = {}
    for c in K.PATCH_CASES + K.FLAGGED_CASES:
        total = L.lib().yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], L.F32) // 4
        off, length = K.packed_f32_floats(c["cout"], c["cin"], c["k"])
        assert 0 < off and off + length <= total
        for tile in K.PATCH_TILES:
            res[c["name"], tile] = K.audit_patch(c, tile, (off, length, total))
    return res


def test_address_audit_is_clean(audits):
    assert len(audits) == 3 * (len(K.PATCH_CASES) + len(K.FLAGGED_CASES))
    for (name, tile), (p, st) in audits.items():
        assert st["max_PR"] <= p["prmax"] and p["prmax"] * p["PC"] <= p["patch_cap"], (name, tile)


def test_tables_hold_the_edges_they_name(built, audits):
    L = built

    def plan(name, tile=5):
        return audits[name, tile][0]

    def stats(name, tile=5):
        return audits[name, tile][1]

    # conv_patch_f32
    assert stats("b_7x1x1")["max_cross"] == 7 and stats("b_5x2x3")["max_cross"] == 5 and stats("b_13x13")["max_cross"] >= 2
    assert any(st["max_cross"] >= 3 for _, st in audits.values())
    p = plan("b_7x1x1")
    assert (p["TH"], p["TW"]) == (27, 1) and p["nblocks"] == 1                           # 27 x 1 for seven 1 x 1 images
    p = plan("b_20x20")
    assert (p["TH"], p["TW"], p["patch_cap"], p["tiles_w"]) == (32, 4, 256, 5)
    assert plan("b_20x20", 7)["patch_cap"] == 256 and plan("b_13x13", 7)["bufmask"] == 0
    assert any(p["patch_cap"] == 128 for p, _ in audits.values()), "the floor of 128 patch pixels"
    assert any(p["nblocks"] < 8 for p, _ in audits.values())                             # q = 0 in the block remap
    assert any(p["nblocks"] == 1 for p, _ in audits.values())
    p = plan("b_52x52")
    assert p["nblocks"] > 8 and 1 <= p["nblocks"] % 8 <= 7
    for name in ("b_13x13", "b_7x9", "b_52x52"):
        assert plan(name)["rows_total"] % plan(name)["TH"] != 0, name                    # a ragged last tile row
    assert plan("b_13x13", 5)["nblocks"] == 8                                            # q = 1, r = 0
    for name in ("b_13x13", "b_3x127"):
        assert plan(name)["W"] % plan(name)["TW"] != 0, name                             # ragged lanes on the right
    assert plan("b_3x127")["TW"] <= 126 < plan("b_3x127")["W"] and plan("b_3x127")["tiles_w"] >= 2
    assert plan("b_5x1")["PC"] == 3 and plan("b_1x40")["H"] == 1
    assert [plan(n)["nchunks"] for n in ("b_1x40", "b_13x13", "b_7x9")] == [1, 2, 3]    # one chunk, an even pair, an odd tail
    assert {c["cout"] for c in K.PATCH_CASES} >= {24, 64, 66, 128, 136, 255}
    assert {c["cin"] for c in K.PATCH_CASES} == {32, 64, 96}
    assert [plan(n)["W"] for n in ("b1_m25_head255", "b1_m129", "b1_m338")] == [25, 129, 338]
    assert [plan(n)["tiles_w"] for n in ("b1_m25_head255", "b1_m129", "b1_m338")] == [1, 2, 3]
    assert plan("b_7x9", 5)["tiles_n"] == 2 and plan("b_1x40", 6)["tiles_n"] == 2 and plan("b_1x40", 5)["tiles_n"] == 3
    shapes = {(c["n"], c["h"], c["w"]) for c in K.PATCH_CASES if c["k"] == 3}
    assert shapes >= {(2, 13, 13), (3, 7, 9), (1, 1, 40), (2, 5, 1), (7, 1, 1), (5, 2, 3), (2, 3, 127), (1, 20, 20), (1, 52, 52)}
    # tile 0 of the 3x3 patch cases is the patch kernel (6 or 7); of every igemm case the 64x64 register tile
    # (yolo_conv_pick_tile answers for a caller that brings a workspace; where that opens no Winograd route it is the direct choice)
    for c in K.PATCH_CASES + K.IGEMM_CASES:
        d = L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=c["x_ld"],
                       x_off=c["x_off"], y_ld=c["y_ld"], y_off=c["y_off"], r_ld=c["r_ld"], r_off=c["r_off"], act=c["act"], out_mode=c["out"])
        picked = L.lib().yolo_conv_pick_tile(d)
        assert picked > 0, c["name"]
        if picked < 13:
            assert picked == direct_tile(c), (c["name"], picked)
        assert direct_tile(c) == (7 if c["k"] == 3 and c["s"] == 1 and c["cin"] % 32 == 0 else 4), c["name"]
    # conv_igemm_f32: M against BM, cout against BN, K steps
    ms = {c["n"] * K.out_hw(c)[0] * K.out_hw(c)[1] for c in K.IGEMM_CASES}
    assert ms >= {25, 64, 65, 129, 507}
    assert {c["cout"] for c in K.IGEMM_CASES} >= {21, 24, 64, 66, 132, 255}
    kts = {K._round_up(c["k"] ** 2 * K._round_up(c["cin"], 4), 32) // 32 for c in K.IGEMM_CASES}
    assert kts >= {1, 2, 3, 9, 27}
    small = [c for c in K.IGEMM_CASES if c["cin"] <= 4]
    assert {(c["cin"], c["k"], c["s"]) for c in small} == {(ci, k, s) for ci in (1, 3, 4) for k, s in ((3, 1), (3, 2), (1, 1))}
    assert {c["x_ld"] for c in small} == {4, 8} and any(c["x_off"] == 4 for c in small)
    for fam in (K.IGEMM_CASES, K.PATCH_CASES):
        assert {c["act"] for c in fam} == {0, 1, 2} and {c["out"] for c in fam} == {0, 1, 2} and any(c["res"] for c in fam)
        odd = [c for c in fam if c["out"] != 2 and ((c["y_ld"] | c["y_off"]) & 3 or (c["res"] and (c["r_ld"] | c["r_off"]) & 3))]
        assert {(c["out"], c["cout"] % 4 == 0) for c in odd} == {(0, True), (0, False), (1, True), (1, False)}
        assert any(c["y_off"] == 2 and c["y_ld"] == c["cout"] + 6 for c in odd) and any(c["y_ld"] % 2 == 1 for c in odd)
        assert any(c["res"] and c["r_off"] == 1 and (c["y_ld"] | c["y_off"]) & 3 == 0 for c in odd)
    # stem: a ragged last wave, a ragged last block, exactly one block
    px = [n * h * w for n, h, w in K.STEM_SHAPES]
    assert 256 in px and any(p % 64 and p < 256 for p in px) and any(p > 256 and p % 256 for p in px) and 1 in px


direct_tile = K.direct_tile


@pytest.mark.parametrize("name", list(K.ALL_CASES))
def test_bound_passes_torch_fp32_and_catches_the_mutants(name):
    c, ops, ref, bound = K.shared(name)
    assert torch.isfinite(ref).all() and (bound > 0).all()
    err = (K.torch_fp32(c, ops).double() - ref).abs()
    assert (err <= bound).all(), (name, float((err / bound).max()))
    for label, wrong in K.mutants(c, ops):
        over = (wrong - ref).abs() > bound
        assert over.any(), (name, label, "the bound cannot tell this mutant from a correct kernel")
