"""YOLO_FLAG_SPLIT_K / ModelState.latency: the fp32 convolutions cut along K for small batches (conv_splitk_f32 + splitk_combine_f32).
Kernel level through yolo_conv_fwd_ws: accuracy against an fp64 convolution next to the exact-f32 kernel (tile 4), workspace
coverage, untouched memory, batch independence, the NaN flag. Network level with ``latency = "all"``: the golden forwards, the plan's
flags, batch independence, ``latency = False`` and detect_images."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import net as onet
from tests import golden_inputs as gi
from tests import rect_inputs as ri

pytestmark = pytest.mark.gpu
FWD_ATOL = 1e-3          # the bars of the whole-network golden test (tests/test_gpu_parity.py)
TIGHT_ATOL = 1e-4
SPARE = 4096


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _case(n, h, w, cin, cout, k, s, act=1, res=False, out=0, x_pad=0, x_off=0, y_pad=0, y_off=0, r_pad=0, r_off=0):
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, act=act, res=res, out=out, x_pad=x_pad, x_off=x_off, y_pad=y_pad,
                y_off=y_off, r_pad=r_pad, r_off=r_off)


# out: 0 NHWC, 1 2x upsampling store, 2 head layout
CASES = {
    "1x1_k32_25px": _case(1, 5, 5, 32, 384, 1, 1),                                            # one K step: S = 1; 25 ragged pixels
    "1x1_k96_straddle": _case(3, 13, 13, 96, 24, 1, 1, act=0),                                 # M tiles straddle images; ragged N tile; KT = 3
    "1x1_k256_res_views": _case(3, 13, 13, 256, 96, 1, 1, act=2, res=True, x_pad=32, x_off=16, y_pad=40, y_off=8, r_pad=16, r_off=4),
    "1x1_head": _case(2, 13, 13, 256, 255, 1, 1, act=0, out=2),                                # scalar store path, nc5 = 85
    "1x1_upsample": _case(2, 13, 13, 256, 128, 1, 1, out=1, y_pad=128, y_off=128),             # into a 256-wide concat buffer at offset 128
    "3x3s1_k4608": _case(1, 13, 13, 512, 64, 3, 1),                                            # many slices, a tap spans slices
    "3x3s1_one_row": _case(1, 1, 40, 32, 256, 3, 1),                                           # kh = 0 and 2 are padding everywhere
    "3x3s1_20x20_res": _case(1, 20, 20, 64, 64, 3, 1, res=True),
    "3x3s2_7x9": _case(5, 7, 9, 32, 96, 3, 2),
    "3x3s2_13x13_mish": _case(3, 13, 13, 64, 64, 3, 2, act=2),
}


def _operands(c, seed):
    g = torch.Generator().manual_seed(seed)
    k, s = c["k"], c["s"]
    ho, wo = (c["h"] + 2 * (k // 2) - k) // s + 1, (c["w"] + 2 * (k // 2) - k) // s + 1
    x = torch.randn((c["n"], c["h"], c["w"], c["cin"] + c["x_pad"]), generator=g)
    w = torch.randn((c["cout"], c["cin"], k, k), generator=g) * (1.0 / (k * k * c["cin"])) ** 0.5
    scale, shift = torch.rand(c["cout"], generator=g) + 0.5, torch.randn(c["cout"], generator=g) * 0.1
    r = torch.randn((c["n"], ho, wo, c["cout"] + c["r_pad"]), generator=g) if c["res"] else None
    if c["out"] == 2:
        y0 = torch.randn((c["n"], 3, ho, wo, c["cout"] // 3), generator=g)
    elif c["out"] == 1:
        y0 = torch.randn((c["n"], 2 * ho, 2 * wo, c["cout"] + c["y_pad"]), generator=g)
    else:
        y0 = torch.randn((c["n"], ho, wo, c["cout"] + c["y_pad"]), generator=g)
    return x, w, scale, shift, r, y0


def _view(c, y):
    """The layer's part of the output buffer, as (n, Ho, Wo, cout)."""
    if c["out"] == 2:
        n, _, ho, wo, nc5 = y.shape
        return y.permute(0, 2, 3, 1, 4).reshape(n, ho, wo, 3 * nc5)
    v = y[..., c["y_off"]:c["y_off"] + c["cout"]]
    return v[:, ::2, ::2] if c["out"] == 1 else v


def _reference(c, ops):
    x, w, scale, shift, r, _ = (t.double() if t is not None else None for t in ops)
    xv = x[..., c["x_off"]:c["x_off"] + c["cin"]].permute(0, 3, 1, 2)
    z = F.conv2d(xv, w, stride=c["s"], padding=c["k"] // 2).permute(0, 2, 3, 1) * scale + shift
    if c["act"] == 1:
        z = torch.maximum(z, 0.1 * z)
    elif c["act"] == 2:
        z = z * torch.tanh(F.softplus(z))
    if r is not None:
        z = z + r[..., c["r_off"]:c["r_off"] + c["cout"]]
    return z


@functools.lru_cache(maxsize=None)
def _shared(name):
    c = CASES[name]
    ops = _operands(c, 5200 + sum(ord(ch) for ch in name))
    return c, ops, _reference(c, ops)


def _launch(L, c, ops, flags, tile=0, fill=0, nancheck=True):
    """One yolo_conv_fwd_ws of case c with the workspace the descriptor asks for (pre-filled with byte `fill`) and SPARE bytes of
    0x5a behind it: (output buffer on the host, NaN flag, return code, the spare bytes after the launch)."""
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x, w, scale, shift, r, y0 = ops
    wp = torch.empty(lib.yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).contiguous().data_ptr(), wp.data_ptr(), c["cout"], c["cin"], c["k"], L.F32, st), "pack")
    xd, sc, sh, yd = x.to(dev), scale.to(dev), shift.to(dev), y0.to(dev)
    rd = r.to(dev) if r is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=x.shape[-1],
                   x_off=c["x_off"], y_ld=c["cout"] + c["y_pad"], y_off=c["y_off"], r_ld=r.shape[-1] if r is not None else 0,
                   r_off=c["r_off"], act=c["act"], out_mode=c["out"], dtype=L.F32,
                   flags=(L.FLAG_RESIDUAL if r is not None else 0) | (L.FLAG_NANCHECK if nancheck else 0) | flags, tile=tile)
    need = lib.yolo_conv_workspace_bytes(d)
    wsb = torch.full((need + SPARE,), fill, dtype=torch.uint8, device=dev)
    wsb[need:] = 0x5a
    rc = lib.yolo_conv_fwd_ws(d, xd.data_ptr(), wp.data_ptr(), sc.data_ptr(), sh.data_ptr(), L.ptr(rd), yd.data_ptr(),
                              wsb.data_ptr() if need else None, need, flag.data_ptr(), st)
    torch.cuda.synchronize()
    return yd.cpu(), int(flag.item()), rc, wsb[need:].cpu()


def _rel_err(c, y, ref):
    return float((_view(c, y).double() - ref).abs().max() / ref.abs().max())


def _outside_untouched(c, y, y0):
    if c["out"] == 2:
        return True
    a, b = y.clone(), y0.clone()
    a[..., c["y_off"]:c["y_off"] + c["cout"]] = 0
    b[..., c["y_off"]:c["y_off"] + c["cout"]] = 0
    return torch.equal(a, b)


def test_slice_counts_of_the_cases(L):
    lib = L.lib()
    S = {}
    for name, c in CASES.items():
        d = L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=c["cin"] + c["x_pad"],
                       x_off=c["x_off"], y_ld=c["cout"] + c["y_pad"], y_off=c["y_off"], act=c["act"], out_mode=c["out"], dtype=L.F32)
        S[name] = lib.yolo_conv_splitk_slices(d)
    assert S["1x1_k32_25px"] == 1 and S["1x1_k96_straddle"] == 1
    assert S["3x3s1_k4608"] == 29                      # 144 K steps in slices of 5, 16 K steps per tap: a tap spans slices
    assert S["1x1_k256_res_views"] > 1 and S["3x3s2_13x13_mish"] > 1 and S["3x3s1_20x20_res"] > 1


@pytest.mark.parametrize("name", list(CASES))
def test_split_k_is_as_accurate_as_the_f32_kernel(L, name):
    """(a) max|err| / max|y| against fp64 is at most twice the exact-f32 kernel's (tile 4, no flag) on the same operands: the pair
    only reorders the sum into S shorter chains. (b) Two launches into workspaces pre-filled with different garbage (all-ones bytes,
    zeros) are bit-equal: every partial that is read was written by its launch. (c) The rest of the output buffer stays as it was,
    the 2x upsampling store writes four equal pixels. (e) The bytes behind the workspace stay as they were.
    Measured (MI355X): profiles/latency/accuracy.txt."""
    c, ops, ref = _shared(name)
    exact, flag0, rc, _ = _launch(L, c, ops, 0, 4)
    assert rc == 0 and flag0 == 0
    e_exact = _rel_err(c, exact, ref)
    assert e_exact < 3e-6
    y, flag, rc, spare = _launch(L, c, ops, L.FLAG_SPLIT_K, fill=0xff)
    assert rc == 0, L.lib().yolo_last_error()
    e = _rel_err(c, y, ref)
    print(f"{name}: split-K {e:.3e}  exact {e_exact:.3e}  ratio {e / e_exact:.2f}")
    assert flag == 0
    assert e <= 2 * e_exact, (e, e_exact)
    assert torch.equal(spare, torch.full((SPARE,), 0x5a, dtype=torch.uint8))
    assert _outside_untouched(c, y, ops[5])
    if c["out"] == 1:
        v = y[..., c["y_off"]:c["y_off"] + c["cout"]]
        assert torch.equal(v[:, ::2, ::2], v[:, 1::2, ::2]) and torch.equal(v[:, ::2, ::2], v[:, ::2, 1::2])
        assert torch.equal(v[:, ::2, ::2], v[:, 1::2, 1::2])
    again, _, rc, spare = _launch(L, c, ops, L.FLAG_SPLIT_K, fill=0x00)
    assert rc == 0 and torch.equal(again, y), "launches into differently filled workspaces differ"
    assert torch.equal(spare, torch.full((SPARE,), 0x5a, dtype=torch.uint8))


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["n"] > 1])
def test_an_image_does_not_depend_on_its_batch(L, name):
    """(d) Every image of the batch equals the same image run alone, bit for bit."""
    c, ops, _ = _shared(name)
    x, w, scale, shift, r, y0 = ops
    yb, _, rc, _ = _launch(L, c, ops, L.FLAG_SPLIT_K)
    assert rc == 0
    one = dict(c, n=1)
    for i in range(c["n"]):
        alone = (x[i:i + 1].contiguous(), w, scale, shift, r[i:i + 1].contiguous() if r is not None else None, y0[i:i + 1].contiguous())
        y1, _, rc1, _ = _launch(L, one, alone, L.FLAG_SPLIT_K)
        assert rc1 == 0 and torch.equal(yb[i:i + 1], y1), i


def test_nan_flag(L):
    """A NaN in one input pixel sets bit 2 of the flag under YOLO_FLAG_NANCHECK; finite inputs leave it 0; without the flag bit the
    word is not touched."""
    c, ops, _ = _shared("3x3s2_13x13_mish")
    _, flag, rc, _ = _launch(L, c, ops, L.FLAG_SPLIT_K)
    assert rc == 0 and flag == 0
    x = ops[0].clone()
    x[1, 6, 3, 5] = float("nan")
    bad = (x,) + tuple(ops[1:])
    y, flag, rc, _ = _launch(L, c, bad, L.FLAG_SPLIT_K)
    assert rc == 0 and flag == 2
    v = _view(c, y)
    assert torch.isnan(v[1]).any() and torch.isfinite(v[0]).all() and torch.isfinite(v[2]).all()
    _, flag, rc, _ = _launch(L, c, bad, L.FLAG_SPLIT_K, nancheck=False)
    assert rc == 0 and flag == 0


def test_forced_tile_is_refused_and_writes_nothing(L):
    c, ops, _ = _shared("3x3s1_20x20_res")
    y, _, rc, _ = _launch(L, c, ops, L.FLAG_SPLIT_K, tile=4)
    assert rc == -2 and torch.equal(y, ops[5])


# ------------------------------------------------------------------------------------------- whole network
def _model(yt, nc, act, wseed, latency):
    m = yt.YOLOv3(num_classes=nc, activation=act)
    m.load_state_dict(onet.synth_state_dict(wseed, 3, nc, gain=gi.NET_GAIN))
    m = m.cuda().eval()
    if latency is not None:
        m._engine.latency = latency
    return m


def _flags(L, m):
    return [[p.table[i].d.flags for i in range(len(p.table))] for p in m._engine._plans.values()]


@pytest.mark.parametrize("name", ["nc80_s96_b2_leaky", "nc80_s96_b1_mish"])
def test_network_forward_latency_all_vs_golden(L, golden, name):
    """The bars of the whole-network golden test; every launch behind the stem carries YOLO_FLAG_SPLIT_K and none of the other kernel
    flags; image 1 of the batch of 2 equals its own batch-1 run, bit for bit."""
    import yolo_for_turbines_amd as yt
    g = golden("net_fwd")
    c = gi.NET_CASES[name]
    m = _model(yt, c["nc"], c["act"], c["wseed"], "all")
    x = onet.synth_input(c["xseed"], c["batch"], c["size"]).cuda()
    with torch.no_grad():
        preds = [p.clone() for p in m(x)]
    for i, p in enumerate(preds):
        ref = g[f"{name}/p{i}"]
        assert tuple(p.shape) == ref.shape and p.dtype == torch.float32
        err = np.abs(p.cpu().numpy() - ref).max()
        print(f"{name} scale {i}: max abs err {err:.3e}")
        assert err <= FWD_ATOL, f"scale {i}: max abs err {err}"
        assert err <= TIGHT_ATOL, f"scale {i}: exact fp32 products should be well inside tolerance, got {err}"
    (plan,) = m._engine._plans.values()
    others = L.FLAG_FILTERS_READY | L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY
    for i in range(plan.first, len(plan.table)):
        d = plan.table[i].d
        assert d.flags & L.FLAG_SPLIT_K, i                      # (every layer behind the stem has cin % 32 == 0; the 3x3 stride-1 ones among them)
        assert not d.flags & others, i
    assert any(plan.table[i].d.ksize == 3 and plan.table[i].d.stride == 1 for i in range(plan.first, len(plan.table)))
    if c["batch"] > 1:
        with torch.no_grad():
            alone = m(x[1:2].contiguous())
        for p, a in zip(preds, alone):
            assert torch.equal(p[1:2], a)


def test_latency_off_is_the_default_forward_bit_for_bit(L):
    """latency = False on a model whose attribute was set and reset: no launch carries the flag, and the predictions equal those of a
    fresh model whose attribute was never touched; the latency forward of the same weights differs in some bit."""
    import yolo_for_turbines_amd as yt
    c = gi.NET_CASES["nc80_s96_b2_leaky"]
    x = onet.synth_input(c["xseed"], c["batch"], c["size"]).cuda()
    with torch.no_grad():
        m = _model(yt, c["nc"], c["act"], c["wseed"], "all")
        lat = [p.clone() for p in m(x)]
        m._engine.latency = False
        off = [p.clone() for p in m(x)]
        fresh_m = _model(yt, c["nc"], c["act"], c["wseed"], None)
        fresh = [p.clone() for p in fresh_m(x)]
    by_plan = _flags(L, m)
    assert len(by_plan) == 2
    assert any(f & L.FLAG_SPLIT_K for f in by_plan[0]) and not any(f & L.FLAG_SPLIT_K for f in by_plan[1])
    assert not any(f & L.FLAG_SPLIT_K for fl in _flags(L, fresh_m) for f in fl)
    assert all(torch.equal(a, b) for a, b in zip(off, fresh))
    assert any(not torch.equal(a, b) for a, b in zip(lat, fresh))


def test_network_forward_rect_latency_all_vs_golden(L, golden):
    import yolo_for_turbines_amd as yt
    name = "nc80_96x160_b2_leaky"
    g = golden("net_rect")
    c = ri.RECT_NET_CASES[name]
    m = _model(yt, c["nc"], c["act"], c["wseed"], "all")
    x = ri.rect_input(c["xseed"], c["batch"], c["H"], c["W"])
    with torch.no_grad():
        preds = m(x.cuda())
    for i, (p, s) in enumerate(zip(preds, (32, 16, 8))):
        assert tuple(p.shape) == (c["batch"], 3, c["H"] // s, c["W"] // s, 5 + c["nc"]) and p.dtype == torch.float32
        if f"{name}/p{i}" in g.files:
            got, ref = p.cpu().numpy(), g[f"{name}/p{i}"]
        else:
            got, ref = p.cpu().reshape(-1)[::3].numpy(), g[f"{name}/p{i}_every3"]
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        assert err <= FWD_ATOL, f"scale {i}: max abs err {err}"
        assert err <= TIGHT_ATOL, f"scale {i}: fp32 path should be well inside tolerance, got {err}"
    assert any(f & L.FLAG_SPLIT_K for fl in _flags(L, m) for f in fl)


def test_detect_images_in_latency_mode(L):
    """detect_images with latency = "all" returns a (B, N, 6) box buffer that is, within the decode tolerance (rtol 3e-6, atol 1e-7,
    classes equal: the bars of test_detect_pipeline_vs_oracle in tests/test_gpu_parity.py), the oracle's decode of the latency
    forward's own predictions: decode and plumbing are held to the bar for equal inputs. The two modes' forwards differ in their
    last bits, so their boxes are not compared at that bar; instead the forwards are: every layer's kernel is within 3e-6 of max|y|
    of an fp64 convolution in either mode (asserted above and in tests/test_gpu_split3.py), the golden forwards are met within
    2.4e-6 absolute by both, and the two predictions must agree within 1e-5 of max(1, max|y|). Kept indices are not compared: scores
    differ in their last bits."""
    import yolo_for_turbines_amd as yt
    from oracle import postprocess as opp
    c = gi.NET_CASES["nc80_s96_b2_leaky"]
    x = onet.synth_input(77, 2, 128).cuda()
    anchors = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
               [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]
    sa = [torch.tensor(a) * g for a, g in zip(anchors, (4, 8, 16))]
    preds = {}
    for mode in (False, "all"):
        m = _model(yt, c["nc"], c["act"], c["wseed"], mode)
        with torch.no_grad():
            preds[mode] = [p.clone().cpu() for p in m(x)]
        boxes, keep, count = yt.detect_images(m, x, sa, 0.45, 0.5, "center")
        assert tuple(boxes.shape) == (2, 3 * (16 + 64 + 256), 6) and tuple(keep.shape) == (2, boxes.shape[1]) and tuple(count.shape) == (2,)
        assert any(bool(f & L.FLAG_SPLIT_K) for fl in _flags(L, m) for f in fl) == (mode == "all")
        if mode == "all":
            got = boxes.cpu().numpy()
            ref = torch.cat([opp.cells_to_boxes(p.clone(), a, p.shape[2]) for p, a in zip(preds[mode], sa)], dim=1).numpy()
            np.testing.assert_allclose(got[..., :5], ref[..., :5], rtol=3e-6, atol=1e-7)
            np.testing.assert_array_equal(got[..., 5], ref[..., 5])
            assert (count.cpu() > 0).all() and (count.cpu() <= boxes.shape[1]).all()
    for i, (a, b) in enumerate(zip(preds["all"], preds[False])):
        diff, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
        print(f"latency vs default predictions, scale {i}: max abs diff {diff:.3e}, max |y| {scale:.3e}")
        assert diff <= 1e-5 * scale, (i, diff, scale)
