"""Winograd F(4x4, 3x3) (tile 15) on the small maps: the filters transformed once, in place behind the packed weights
(YOLO_FLAG_FILTERS_APPENDED), the launch of 13 x 13 maps at batch 32 as one round of half workgroups, and the engine's route."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return pkg


def _cut(L, d):
    whole, half = C.c_int(-1), C.c_int(-1)
    L.check(L.lib().yolo_conv_wino4_blocks(d, C.byref(whole), C.byref(half)), "yolo_conv_wino4_blocks")
    return whole.value, half.value


def _desc(L, B, H, W, cin, cout, residual=False, y_ld=None, r_ld=0, r_off=0, flags=0):
    return L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=3, stride=1, x_ld=cin, x_off=0, y_ld=y_ld or cout, y_off=0,
                      r_ld=r_ld, r_off=r_off, act=L.ACT_LEAKY, out_mode=L.OUT_NHWC, dtype=L.F32,
                      flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK | flags, tile=15)


def _appended(L, d, w, dev, st, guard=64, fill=0x55):
    """The packed weights of `w` with U4 made in place behind them, in a buffer with `guard` bytes of `fill` behind the stated size.
    Returns (buffer, stated size, offset of U4)."""
    lib = L.lib()
    cout, cin = w.shape[:2]
    packed = lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32)
    off = (packed + 15) // 16 * 16
    size = lib.yolo_wino4_appended_bytes(d)
    assert size == off + lib.yolo_wino4_filter_bytes(d)
    buf = torch.full((size + guard,), fill, dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), buf.data_ptr(), cout, cin, 3, L.F32, st), "yolo_pack_weights")
    front = buf[:off].clone()
    L.check(lib.yolo_wino4_filters(d, buf.data_ptr(), buf.data_ptr() + off, st), "yolo_wino4_filters")
    torch.cuda.synchronize()
    assert torch.equal(buf[:off], front)                                       # the packed section is as it was
    assert int(buf[size:].min()) == fill and int(buf[size:].max()) == fill    # nothing written behind the stated size
    return buf, size, off


SOURCE_CASES = [  # (B, H, W, cin, cout, residual, r_ld, r_off, cut = (whole, half tile blocks))
    (2, 13, 13, 64, 64, False, 0, 0, (0, 1)),             # one tile block of 32 tiles: the second half workgroup is empty
    (3, 13, 13, 68, 84, True, 96, 8, (0, 1)),             # residual view, odd C4 (17 -> padded plane), ragged channel block
    (2064, 8, 8, 4, 64, False, 0, 0, (129, 0)),           # more than half a round: whole workgroups
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SOURCE_CASES)
def test_three_filter_sources_give_the_same_bits(yt, case):
    """A tile-15 launch that reads U4 behind the packed weights (YOLO_FLAG_FILTERS_APPENDED) equals, bit for bit, one that reads a
    separate U4 (YOLO_FLAG_FILTERS_READY) and one that transforms the filters itself; the in-place transform leaves the packed
    section and the bytes behind yolo_wino4_appended_bytes alone and writes the U4 that yolo_wino4_filters writes elsewhere."""
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, r_ld, r_off, cut = case
    g = torch.Generator().manual_seed(8100 + B + cin + cout)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, W, cin), generator=g).to(dev)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
    r = torch.randn((B, H, W, r_ld), generator=g).to(dev) if residual else None
    d = _desc(L, B, H, W, cin, cout, residual, r_ld=r_ld, r_off=r_off)
    assert _cut(L, d) == cut
    wa, size, off = _appended(L, d, w, dev, st)
    nu = lib.yolo_wino4_filter_bytes(d)
    u4 = torch.empty(nu, dtype=torch.uint8, device=dev)
    L.check(lib.yolo_wino4_filters(d, wa.data_ptr(), u4.data_ptr(), st), "yolo_wino4_filters")
    torch.cuda.synchronize()
    assert torch.equal(wa[off:size], u4)
    need = lib.yolo_conv_workspace_bytes(d)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def run(flags, wptr):
        dd = _desc(L, B, H, W, cin, cout, residual, r_ld=r_ld, r_off=r_off, flags=flags)
        assert lib.yolo_conv_workspace_bytes(dd) == need
        y = torch.zeros((B, H, W, cout), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.yolo_conv_fwd_ws(dd, x.data_ptr(), wptr, scale.data_ptr(), shift.data_ptr(), L.ptr(r), y.data_ptr(),
                                     ws.data_ptr(), need, flag.data_ptr(), st), "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        return y.view(torch.int32).cpu()

    plain = run(0, wa.data_ptr())
    assert int(plain.abs().max()) > 0
    assert torch.equal(run(L.FLAG_FILTERS_APPENDED, wa.data_ptr()), plain)
    assert torch.equal(run(L.FLAG_FILTERS_READY, u4.data_ptr()), plain)


FP64_CASES = [  # (B, H, W, cin, cout, residual, cut)
    (1, 13, 13, 512, 64, False, (0, 1)),                  # the flagship K: 64 stages per pass
    (2, 13, 13, 512, 128, True, (0, 1)),
    (32, 13, 13, 8, 1024, False, (0, 8)),                 # the flagship grid: 8 tile blocks x 16 channel blocks x 2 halves = 256; one stage
    (32, 13, 13, 24, 1024, False, (0, 8)),                # ... three stages: the ring's prologue alone
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FP64_CASES)
def test_small_maps_against_fp64(yt, case):
    """Tile 15 with appended filters on 13 x 13 maps against an fp64 convolution of the same operands, bar 1e-5 of max|y| (the
    kernel's bar in test_gpu_wino4.py). The batch-32 cases are the launch geometry of the 416 network's 13 x 13 layers; they also
    raise the NaN flag for a NaN in the last tile."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, cut = case
    g = torch.Generator().manual_seed(8200 + B + cin + cout)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, W, cin), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    r = torch.randn((B, H, W, cout), generator=g) if residual else None
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1).permute(0, 2, 3, 1)
    if residual:
        ref = ref + r.double()
    d = _desc(L, B, H, W, cin, cout, residual, r_ld=cout if residual else 0, flags=L.FLAG_FILTERS_APPENDED)
    assert _cut(L, d) == cut
    wa, _, _ = _appended(L, d, w, dev, st)
    xd, sd, shd = x.to(dev), scale.to(dev), shift.to(dev)
    rd = r.to(dev) if residual else None
    need = lib.yolo_conv_workspace_bytes(d)
    ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)

    def run(xp):
        y = torch.zeros((B, H, W, cout), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.yolo_conv_fwd_ws(d, xp.data_ptr(), wa.data_ptr(), sd.data_ptr(), shd.data_ptr(), L.ptr(rd), y.data_ptr(),
                                     ws.data_ptr(), need, flag.data_ptr(), st), "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
        return y.cpu(), int(flag.item())

    got, flag = run(xd)
    assert flag == 0
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print("max|err| / max|y| =", err)
    assert err <= 1e-5, err
    assert int(ws[need:].min()) == 0x7f                              # nothing written past the stated workspace
    if B == 32:
        xn = xd.clone()
        xn[B - 1, H - 1, W - 1, 0] = float("nan")                    # the last tile of the last half workgroup
        assert run(xn)[1] & 2


@pytest.fixture(scope="module")
def net13(yt):
    """One 416 x 416 image through a 2-class network: the smallest input whose 512 -> 1024 layers see a 13 x 13 map. Returns
    (state dict, input, outputs with the route on, the plan's launches that carry the flag)."""
    from oracle import net as onet
    from yolo_for_turbines_amd import _lib as L
    sd = onet.synth_state_dict(21, 3, 2, gain=0.8)
    x = onet.synth_input(22, 1, 416).cuda()
    m = yt.YOLOv3(num_classes=2)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    with torch.no_grad():
        out = [o.clone() for o in m(x)]
    plan = next(iter(m._engine._plans.values()))
    flagged = [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_FILTERS_APPENDED]
    return sd, x, out, flagged, m


@pytest.mark.gpu
def test_model_route_on_and_off_agree(yt, net13):
    """The eval forward with the seven 13 x 13 layers as F(4x4) on appended filters against the same network with
    ModelState.wino4_small = False (F(2x2) there): max|on - off| / max|off| per head within 1.2e-5, the project's bound for a change
    of an fp32 route (each route alone holds 1e-5 of max|y| per layer against fp64)."""
    from yolo_for_turbines_amd import _lib as L
    sd, x, on, flagged, _ = net13
    assert len(flagged) == 7
    m = yt.YOLOv3(num_classes=2)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    m._engine.wino4_small = False
    with torch.no_grad():
        off = m(x)
    plan = next(iter(m._engine._plans.values()))
    assert not any(plan.table[i].d.flags & L.FLAG_FILTERS_APPENDED for i in range(len(plan.table)))
    for a, b in zip(on, off):
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        print("max|on - off| / max|off| =", err)
        assert 0 < err <= 1.2e-5, err


@pytest.mark.gpu
def test_appended_filters_follow_a_weight_update(yt, net13):
    """After an in-place weight change the next eval forward equals a fresh model's bit for bit: the filters behind the packed
    weights are made again with them."""
    from yolo_for_turbines_amd.model import CNNBlock
    sd, x, before, flagged, m = net13
    assert len(flagged) == 7
    with torch.no_grad():
        blocks = [b for b in m.modules() if isinstance(b, CNNBlock) and b.conv.kernel_size[0] == 3]
        for k, b in enumerate(blocks):
            b.conv.weight.mul_(1.0 + 0.03 * ((k % 5) - 2.5))
        after = m(x)
        fresh = yt.YOLOv3(num_classes=2)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        fresh = fresh.cuda().eval()
        want = fresh(x)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    for a, w_ in zip(after, want):
        assert torch.equal(a, w_)
