"""The cases of tests/conv_wino_rs_cases.py on the host (nothing is launched): the reference alone meets both bars (a plain-torch
fp32 restatement of F(2x2), and torch's fp32 convolution for the 1x1 cases, stay under the per-element bound on every Gaussian
case and equal the fp64 reference bit for bit on every integer case); three subtly wrong F(2x2) variants, and a klim shifted by
one, fail on every case that has their edge; the exactness condition of every integer case holds; the tables hold the geometry
their `why` names, and the restated routing equals yolo_conv_pick_tile."""
import pytest
import torch

from tests import conv_wino_rs_cases as W
from tests.conv_f32_launch import bits, same_bits

RUNNABLE = [n for n, c in W.ALL_CASES.items()]
INT = [n for n in RUNNABLE if W.ALL_CASES[n]["kind"] == "int"]
GAUSS = [n for n in RUNNABLE if W.ALL_CASES[n]["kind"] == "gauss"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _fails(c, ref, bound, wrong):
    """does the case's bar tell `wrong` from a correct result?"""
    if c["kind"] == "int":
        return not same_bits(wrong, ref)
    return bool(((wrong.double() - ref).abs() > bound).any())


@pytest.mark.parametrize("name", INT)
def test_fp32_restatement_equals_the_reference_bit_for_bit(name):
    c, ops, ref, _ = W.shared(name)
    got = W.fp32_value(c, ops)
    assert got.dtype == torch.float32 and same_bits(got, ref), (name, int((bits(got) != bits(ref)).sum()))


@pytest.mark.parametrize("name", GAUSS)
def test_fp32_restatement_stays_under_the_bound(name):
    c, ops, ref, bound = W.shared(name)
    assert torch.isfinite(ref).all() and (bound > 0).all()
    ratio = float(((W.fp32_value(c, ops).double() - ref).abs() / bound).max())
    print(f"{name}: fp32 restatement err/bound {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("name", INT)
def test_integer_cases_are_exact_in_any_order(name):
    """8 S^ < 2^24 (the module text), and the premises of the signed-zero argument: every scale is positive, no shift is -0, no
    residual is zero, and the reference holds no -0."""
    c, ops, ref, _ = W.shared(name)
    margin = W.exactness_margin(c, ops)
    print(f"{name}: 8 S^ / 2^24 = {margin:.4f}")
    assert margin < 1.0, (name, margin)
    assert c["act"] in (0, 1)
    assert bool((ops["scale"] > 0).all()) and not bool(torch.signbit(ops["shift"])[ops["shift"] == 0].any())
    assert ops["r"] is None or bool((ops["r"] != 0).all())
    assert bool((ops["x"] != 0).all()) and float(ops["x"].abs().max()) <= c["xmax"] and float(ops["w"].abs().max()) <= c["wmax"]
    assert torch.equal(ops["w"], ops["w"].round())
    assert not bool(torch.signbit(ref)[ref == 0].any()), (name, "a -0 in the reference")


def test_signed_zero_arithmetic():
    """what the argument uses, in fp32: x + (-x) = +0, (-0) + (+0) = +0, (+-0) + s = s, LeakyReLU keeps +0 - and what it avoids:
    (-0) + (-0) = -0, so a chain that does not start at +0, or a shift of -0, would make a zero's sign a matter of order"""
    z, nz, one = torch.zeros(1), -torch.zeros(1), torch.ones(1)
    for v, neg in ((one + (-one), False), (nz + z, False), (nz * 2.0 + z, False), (torch.maximum(z, z * 0.1), False), (nz + nz, True),
                   (nz * 2.0 + nz, True)):
        assert float(v) == 0.0 and bool(torch.signbit(v)) == neg
    assert float(nz + 3.0) == 3.0


@pytest.mark.parametrize("variant", W.VARIANTS + ("klim-1", "klim+1"))
def test_wrong_variants_fail_wherever_their_edge_is(variant):
    """both kinds of case, every case that has the edge; a klim shifted down loses a real column, shifted up reads one garbage
    column of the filters against one garbage channel of dz"""
    hit = []
    for name in RUNNABLE:
        c, ops, ref, bound = W.shared(name)
        if not W.has_edge(c, variant):
            continue
        assert _fails(c, ref, bound, W.fp32_value(c, ops, variant)), (name, variant, "the bar cannot tell this variant from a correct kernel")
        hit.append(c["kind"])
    assert set(hit) == {"int", "gauss"}, (variant, hit)


def test_the_edges_are_in_the_tables():
    cases = W.ALL_CASES
    assert any(W.has_edge(c, "col") for c in W.WINO_CASES) and any(not W.has_edge(c, "col") for c in W.WINO_CASES)
    assert sum(W.has_edge(c, "klim") for c in W.DGRAD_CASES) == 3
    assert {c["klim"] for c in W.DGRAD_CASES} == {84, 33} and {c["cin"] for c in W.DGRAD_CASES} == {96, 64}
    assert {c["cout"] for c in W.DGRAD_CASES} == {64, 96} and any(c["res"] for c in W.DGRAD_CASES if c["kind"] == "int")
    for fam in (W.RS_GAUSS, W.WINO_GAUSS):
        assert {c["act"] for c in fam} == {0, 1, 2} and {c["act"] for c in fam if c["res"]} == {0, 1, 2}
    # ---- R
    geo = {n: W.rs_geometry(c) for n, c in cases.items() if c["k"] == 1}
    assert [geo[n]["M"] for n in ("r_m1", "r_m31", "r_m32", "r_m33")] == [1, 31, 32, 33]
    assert [geo[n]["tiles"] for n in ("r_m1", "r_m31", "r_m32", "r_m33")] == [1, 1, 1, 2]
    assert [geo[n]["last_pixels"] for n in ("r_m1", "r_m31", "r_m32", "r_m33")] == [1, 31, 32, 1]
    for n in ("r_m1", "r_m31", "r_m32", "r_m33", "r_groups2", "r_groups3"):
        g = geo[n]                                                     # fewer tiles than `per`: one tile each, all look-ahead from the zero page
        assert g["per"] == g["tiles"] < 256 // g["ngroups"] and set(g["counts"]) == {1} and set(g["zero_page"]) == {g["slots"] - 1}
    assert [geo[n]["ngroups"] for n in ("r_m1", "r_groups2", "r_groups3")] == [1, 2, 3]
    assert {cases[n]["cin"] for n in ("r_m31", "r_m32", "r_m33")} == {256, 384, 512}
    for k, ss in ((256, (3, 4)), (384, (3, 4)), (512, (2, 3))):
        slots = 3 if k <= 384 else 2
        assert ss == (slots, slots + 1)
        for s in ss:
            g = geo[f"r_wrap_k{k}_t{32 * s}"]
            assert (g["ngroups"], g["per"], g["tiles"], g["slots"]) == (8, 32, 32 * s, slots) and set(g["counts"]) == {s} and g["last_pixels"] == 32
            g = geo[f"r_wrap_k{k}_t{32 * s + 1}"]
            assert (g["per"], g["tiles"], g["slots"]) == (32, 32 * s + 1, slots) and g["extra"] == [0]
            assert g["counts"] == [s + 1] + [s] * 31 and 0 < g["last_pixels"] < 32
    g = geo["r_per256_t257"]
    assert (g["ngroups"], g["per"], g["tiles"], g["extra"], g["counts"][0]) == (1, 256, 257, [0], 2) and 0 < g["last_pixels"] < 32
    c = cases["r_up_13x13"]
    assert c["out"] == W.OUT_UP and (c["h"], c["w"]) == (13, 13) and 169 % 32 != 0 and c["n"] == 2
    c = cases["r_views4"]
    assert c["x_ld"] == c["cin"] + 4 and (c["x_off"], c["y_off"], c["r_off"]) == (4, 4, 4) and all(v % 8 == 4 for v in (c["x_ld"], c["x_off"], c["y_off"], c["r_off"]))
    assert {(c["act"], c["res"]) for c in W.RS_CASES if c["kind"] == "int"} >= {(0, True), (1, True), (0, False), (1, False)}
    assert [W.tile0_lands(cases[n]) for n in W.names(W.RS_ROUTE_CASES)] == [W.TILE_RS, W.TILE_REG64, W.TILE_REG64]
    assert [(c["h"], c["w"], c["res"]) for c in W.RS_ROUTE_CASES] == [(1, 2048, False), (1, 2047, False), (1, 2048, True)]
    for ci, cg in zip(W.RS_ROUTE_CASES, W.RS_ROUTE_GAUSS):             # the same launches on real values
        assert cg["kind"] == "gauss" and W.tile0_lands(cg) == W.tile0_lands(ci)
        assert {k: v for k, v in cg.items() if k not in ("name", "kind", "why")} == {k: v for k, v in ci.items() if k not in ("name", "kind", "why")}
    c = cases["wg_20x20"]                                              # the tile-13 side of wino2_maxpix on real values
    assert c["kind"] == "gauss" and c["h"] * c["w"] > W.WINO2_MAXPIX and W.tile0_lands(c) == W.TILE_WINO
    assert any(c["kind"] == "gauss" and W.tile0_lands(c) == W.TILE_WINO2 for c in W.WINO_GAUSS + W.DGRAD_CASES)
    assert any(c["n"] == 3 for c in W.RS_CASES) and any(c["n"] == 3 for c in W.RS_GAUSS)
    # ---- W
    geo = {n: W.wino_geometry(c) for n, c in cases.items() if c["k"] == 3}
    assert {(c["h"], c["w"]) for c in W.WINO_CASES} >= {(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (4, 5), (13, 13)}
    assert {geo[n]["T"] for n in W.names(W.WINO_CASES)} >= {3, 63, 64, 65, 512, 529}
    for n in ("w_1x1", "w_5x5_t63", "w_3x3_t64", "w_1x9"):
        assert geo[n]["max_images_per_block"] >= 3, n                  # tiles of one block in different images
    assert [geo[n]["T"] for n in ("w_1x1", "w_5x5_t63", "w_3x3_t64", "w_1x9")] == [3, 63, 64, 65]
    assert [geo[n]["n_mt"] for n in ("w_1x1", "w_5x5_t63", "w_3x3_t64", "w_1x9", "w_t512", "w_46x46")] == [1, 1, 1, 2, 8, 9]
    assert geo["w_t512"]["leaving"] == 0 and geo["w_46x46"]["rounds"] == 2 and geo["w_46x46"]["leaving"] == 7 * geo["w_46x46"]["n_nt"]
    assert (cases["w_46x46"]["n"], geo["w_46x46"]["T"]) == (1, 529)
    assert {c["cin"] for c in W.WINO_CASES} >= {4, 32, 96, 160} and {c["cout"] for c in W.WINO_CASES} >= {4, 60, 64, 68, 132}
    assert [geo[n]["stages"] for n in ("w_1x9", "w_9x1", "w_4x5")] == [1, 24, 40] and geo["w_9x1"]["stages"] == 6 * 4
    assert [geo[n]["cgroups"] for n in ("w_1x9", "w_1x1", "w_9x1", "w_4x5")] == [1, 1, 3, 5]
    assert [geo[n]["n_nt"] for n in ("w_1x9", "w_9x1", "w_3x3_t64", "w_2x2", "w_4x5")] == [1, 1, 1, 2, 3]
    c = cases["w_views4"]
    assert (c["x_off"], c["y_off"], c["r_off"]) == (4, 4, 4) and c["x_ld"] % 8 == 4 and W._views4(c)
    c = cases["w_layer_13x13"]
    assert (c["n"], c["h"], c["w"], c["cin"], c["cout"]) == (1, 13, 13, 512, 1024)
    assert W.tile0_lands(cases["w_13x13"]) == W.TILE_WINO2 and W.tile0_lands(cases["w_20x20"]) == W.TILE_WINO
    assert W.tile0_lands(cases["w_46x46"]) == 7 and W.tile0_lands(dict(cases["w_46x46"], cin=64)) == W.TILE_WINO4
    assert any(c["n"] == 3 for c in W.WINO_CASES) and any(c["n"] == 3 for c in W.WINO_GAUSS) and any(c["n"] == 3 for c in W.DGRAD_CASES)
    for c in W.RS_REFUSED + W.WINO_REFUSED:
        assert c["y_off"] == 2 and not W._views4(c) and W.tile0_lands(c) in (W.TILE_REG64, 7)


def test_restated_routing_and_workspace_equal_the_library(built):
    """yolo_conv_pick_tile reports the F(2x2) family as 13 (also where the launch takes the two-pass kernel) and a conv1_rs_f32
    layer as its direct tile; yolo_conv_workspace_bytes of tiles 13 / 14 is the V buffer of the restated geometry."""
    from tests.conv_h16_launch import switches
    L = built
    sw = switches(L)
    default_routing = not any(sw[k] for k in ("YOLO_NO_WINOGRAD", "YOLO_NO_CONV1_RS")) and sw["YOLO_WINO2_MAXPIX"] == W.WINO2_MAXPIX
    for name, c in W.ALL_CASES.items():
        def desc(tile):
            return L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=1, x_ld=c["x_ld"], x_off=c["x_off"],
                              y_ld=c["y_ld"], y_off=c["y_off"], r_ld=c["r_ld"], r_off=c["r_off"], act=c["act"], out_mode=c["out"], dtype=L.F32,
                              flags=L.FLAG_RESIDUAL if c["res"] else 0, tile=tile)
        lands = W.tile0_lands(c)
        if c["k"] == 3 and W._views4(c):                               # forced tiles: no switch bears on the size
            for tile in (W.TILE_WINO, W.TILE_WINO2):
                assert L.lib().yolo_conv_workspace_bytes(desc(tile)) == W.wino_geometry(c)["workspace_bytes"], (name, tile)
        if not default_routing:
            continue                                                    # an A/B switch is set: only what it bears on is left out
        picked = L.lib().yolo_conv_pick_tile(desc(0))
        want = {W.TILE_WINO2: W.TILE_WINO, W.TILE_RS: W.TILE_REG64}.get(lands, lands)
        assert picked == want, (name, picked, lands)
        if c["k"] == 3 and W._views4(c):
            need0 = L.lib().yolo_conv_workspace_bytes(desc(0))
            assert (need0 == W.wino_geometry(c)["workspace_bytes"]) == (lands in (W.TILE_WINO, W.TILE_WINO2)), (name, need0)
