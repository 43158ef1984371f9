"""Winograd F(4x4, 3x3) (tile 15): the short last round cut into half workgroups, the filters transformed once
(YOLO_FLAG_FILTERS_READY), and the engine keeping those filters in step with the weights."""
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


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _cut(L, d):
    whole, half = C.c_int(-1), C.c_int(-1)
    L.check(L.lib().yolo_conv_wino4_blocks(d, C.byref(whole), C.byref(half)), "yolo_conv_wino4_blocks")
    return whole.value, half.value


def _desc(L, B, H, W, cin, cout, residual=False, act=1, x_ld=None, y_ld=None, y_off=0, r_ld=0, r_off=0, flags=0, ksize=3):
    return L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=ksize, stride=1, x_ld=x_ld or cin, x_off=0, y_ld=y_ld or cout, y_off=y_off,
                      r_ld=r_ld, r_off=r_off, act=act, out_mode=L.OUT_NHWC, dtype=L.F32,
                      flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK | flags, tile=15)


HALF_CASES = [  # (B, H, W, cin, cout, residual, act, y_ld, r_ld, r_off)
    (1, 4, 4, 4, 64, False, 1, 64, 0, 0),            # one tile: the second half workgroup has no valid tile and writes nothing
    (3, 9, 7, 256, 512, True, 2, 512, 512, 0),       # Mish + residual; 18 tiles, all in the first half
    (5, 52, 52, 128, 64, True, 1, 64, 64, 0),        # 845 tiles = 14 tile blocks; the last has 13 tiles: ragged first half, empty second
    (2, 6, 8, 128, 84, True, 1, 84, 96, 8),          # residual view; ragged channel block
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", HALF_CASES)
def test_half_workgroups_against_fp64(yt, case):
    """Launches of at most half a round of workgroups run as half workgroups (asserted through yolo_conv_wino4_blocks). Reference and
    bar of test_gpu_wino4.py: an fp64 convolution of the same operands, 1e-5 of max|y|; the rest of the output buffer untouched;
    the NaN flag."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, act, y_ld, r_ld, r_off = case
    g = torch.Generator().manual_seed(2300 + cin + cout + H + W + B)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, W, cin), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    y0 = torch.randn((B, H, W, y_ld + 4), generator=g)          # four channels behind the layer's: must stay as they are
    r = torch.randn((B, H, W, r_ld), generator=g) if residual else None
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1) if act == 1 else (F.mish(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + r[..., r_off:r_off + cout].double()
    xd, sd, shd = x.to(dev), scale.to(dev), shift.to(dev)
    rd = r.to(dev) if residual else None
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), wp.data_ptr(), cout, cin, 3, L.F32, st))
    d = _desc(L, B, H, W, cin, cout, residual, act, y_ld=y_ld + 4, r_ld=r_ld, r_off=r_off)
    n_mt = (B * ((H + 3) // 4) * ((W + 3) // 4) + 63) // 64
    assert _cut(L, d) == (0, n_mt)
    need = lib.yolo_conv_workspace_bytes(d)
    ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)

    def run(xp):
        yd = y0.clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.yolo_conv_fwd_ws(d, xp.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                  yd.data_ptr(), ws.data_ptr(), need, flag.data_ptr(), st)
        torch.cuda.synchronize()
        return rc, yd.cpu(), int(flag.item())

    rc, got, flag = run(xd)
    assert rc == 0 and flag == 0, lib.yolo_last_error()
    err = float((got[..., :cout].double() - ref).abs().max() / ref.abs().max())
    print("max|err| / max|y| =", err)
    assert err <= 1e-5, err
    assert torch.equal(got[..., cout:], y0[..., cout:])              # neighbouring channels of the buffer untouched
    assert int(ws[need:].min()) == 0x7f                              # nothing written past the stated workspace
    xn = xd.clone()
    xn[B - 1, H - 1, W - 1, 0] = float("nan")                        # the last tile: in the ragged half
    assert run(xn)[2] & 2


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True])
def test_whole_and_half_workgroups_give_the_same_bits(yt, residual):
    """8 x 8 maps, 4 -> 64 channels: 2,064 images are 129 tile blocks, more than half the compute units, so every block is whole;
    the first 16 images alone are one tile block, cut into halves. The 16 images' outputs agree bit for bit (also the batch
    independence test_gpu_fullsize.py asks of the network)."""
    from yolo_for_turbines_amd import _lib as L
    B, Bs, H, cin, cout = 2064, 16, 8, 4, 64
    g = torch.Generator().manual_seed(77 + residual)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, H, cin), generator=g).to(dev)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
    r = torch.randn((B, H, H, cout), generator=g).to(dev) if residual else None
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), wp.data_ptr(), cout, cin, 3, L.F32, st))
    outs = []
    for n, want in ((B, (129, 0)), (Bs, (0, 1))):
        d = _desc(L, n, H, H, cin, cout, residual, 1, r_ld=cout if residual else 0)
        assert _cut(L, d) == want
        need = lib.yolo_conv_workspace_bytes(d)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        y = torch.zeros((n, H, H, cout), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.yolo_conv_fwd_ws(d, x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(), L.ptr(r), y.data_ptr(),
                                     ws.data_ptr(), need, flag.data_ptr(), st), "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        outs.append(y[:Bs].cpu())
    assert float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(128, 256), (64, 96), (4, 64)])
def test_filters_transformed_once(yt, cin, cout):
    """yolo_wino4_filters writes the bytes a launch without the flag leaves in the U4 part of its workspace; a launch with
    YOLO_FLAG_FILTERS_READY gives the same output bytes and leaves that part of the workspace alone."""
    from yolo_for_turbines_amd import _lib as L
    B, H, W = 2, 8, 12
    g = torch.Generator().manual_seed(501 + cin + cout)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, W, cin), generator=g).to(dev)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
    r = torch.randn((B, H, W, cout), generator=g).to(dev)
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), wp.data_ptr(), cout, cin, 3, L.F32, st))
    d = _desc(L, B, H, W, cin, cout, True, 1, r_ld=cout)
    c4p, coutp = (cin // 4 + 1) // 2 * 2, (cout + 63) // 64 * 64
    tpad = (B * 2 * 3 + 63) // 64 * 64
    nu = 36 * c4p * coutp * 16
    assert lib.yolo_wino4_filter_bytes(d) == nu
    need = lib.yolo_conv_workspace_bytes(d)
    assert need == 36 * c4p * tpad * 16 + nu

    def run(desc, wptr):
        ws = torch.full((need,), 0x7f, dtype=torch.uint8, device=dev)
        y = torch.zeros((B, H, W, cout), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.yolo_conv_fwd_ws(desc, x.data_ptr(), wptr, scale.data_ptr(), shift.data_ptr(), r.data_ptr(), y.data_ptr(),
                                     ws.data_ptr(), need, flag.data_ptr(), st), "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        return y.cpu(), ws[need - nu:].cpu()

    y_plain, u_plain = run(d, wp.data_ptr())
    u4 = torch.full((nu + 64,), 0x55, dtype=torch.uint8, device=dev)
    L.check(lib.yolo_wino4_filters(d, wp.data_ptr(), u4.data_ptr(), st), "yolo_wino4_filters")
    torch.cuda.synchronize()
    assert torch.equal(u4[:nu].cpu(), u_plain)
    assert int(u4[nu:].min()) == 0x55 and int(u4[nu:].max()) == 0x55
    dr = _desc(L, B, H, W, cin, cout, True, 1, r_ld=cout, flags=L.FLAG_FILTERS_READY)
    y_ready, u_ready = run(dr, u4.data_ptr())
    assert torch.equal(y_ready.view(torch.int32), y_plain.view(torch.int32))
    assert int(u_ready.min()) == 0x7f and int(u_ready.max()) == 0x7f


def test_filters_ready_on_another_family_is_an_argument_error(built):
    """The flag on a 1x1 descriptor (and on a 3x3 one forced to a direct tile) is refused before anything is launched."""
    L = built
    lib = L.lib()
    for ksize, tile in ((1, 0), (3, 5)):
        d = _desc(L, 1, 8, 8, 64, 64, ksize=ksize, flags=L.FLAG_FILTERS_READY)
        d.flags &= ~L.FLAG_NANCHECK
        d.tile = tile
        rc = lib.yolo_conv_fwd_ws(d, 16, 16, 16, 16, 0, 16, 16, 1 << 30, 0, 0)       # never dereferenced: refused on the arguments
        assert rc == -1
        assert b"FILTERS_READY" in lib.yolo_last_error()
    d = _desc(L, 2, 52, 52, 128, 256)
    assert lib.yolo_wino4_filter_bytes(d) == 36 * 32 * 256 * 16                      # (cin, cout) only
    d.n = 32
    assert lib.yolo_wino4_filter_bytes(d) == 36 * 32 * 256 * 16
    assert lib.yolo_wino4_filter_bytes(_desc(L, 1, 8, 8, 64, 64, ksize=1)) == 0


def test_packed_block_marks_its_filters_stale(built):
    """Host side of the engine's bookkeeping: U4 is sized by (cin, cout), starts stale, and `invalidate` makes it stale again."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine
    L = built
    blk = yt.model.CNNBlock(128, 256, kernel_size=3, padding=1)
    st = engine.ModelState()
    pk = st.packed(blk, torch.device("cpu"))
    assert "u4" not in pk.prepared
    u4 = pk.want("u4", _desc(L, 1, 52, 52, 128, 256))
    assert u4.numel() == 36 * 32 * 256 * 16 and pk.prepared["u4"].stamp is None
    assert pk.want("u4", _desc(L, 8, 104, 104, 128, 256)) is u4                        # one buffer serves every plan
    pk.prepared["u4"].stamp = pk.stamp = engine.PackedBlock.stamp_of(blk)[0]
    st.invalidate()
    assert pk.stamp is None and pk.prepared["u4"].stamp is None


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["inplace", "set_layers"])
def test_eval_forward_after_a_weight_update_matches_a_fresh_model(yt, how):
    """The transformed filters follow the weights: after an in-place update that PyTorch's version counters see, and after
    `.data` writes handed back through `set_layers` (the reference loader's way), the next eval forward equals a fresh model's
    bit for bit."""
    from oracle import net as onet
    from yolo_for_turbines_amd import _lib as L
    from yolo_for_turbines_amd.model import CNNBlock
    NC, S, B = 2, 224, 1                       # 56 x 56 and 28 x 28 maps: their 3x3 stride-1 layers pick tile 15
    sd = onet.synth_state_dict(11, 3, NC, gain=0.8)
    x = onet.synth_input(12, B, S).cuda()
    m = yt.YOLOv3(num_classes=NC)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    with torch.no_grad():
        before = [o.clone() for o in m(x)]
        plan = next(iter(m._engine._plans.values()))
        ready = [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_FILTERS_READY]
        assert len(ready) >= 4, ready
        blocks = [b for b in m.modules() if isinstance(b, CNNBlock) and b.conv.kernel_size[0] == 3]
        for k, b in enumerate(blocks):
            f = 1.0 + 0.03 * ((k % 5) - 2.5)
            if how == "inplace":
                b.conv.weight.mul_(f)
            else:
                b.conv.weight.data.mul_(f)
                b.set_layers([b.conv, b.batch_norm, b.activation])
        after = m(x)
        fresh = yt.YOLOv3(num_classes=NC)
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        fresh = fresh.cuda().eval()
        want = fresh(x)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    for a, w_ in zip(after, want):
        assert torch.equal(a, w_)


def test_eval_plan_hands_the_tile_15_layers_their_filters(built):
    """Host side of the eval plan (built on the CPU device: no launch): at batch 32, 416 x 416, 80 classes the 24 launches that pick
    tile 15 carry YOLO_FLAG_FILTERS_READY and point at their block's U4 (261.9 MB in all); a second plan shares those buffers; a
    plan forced to another tile sets no flag."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine
    L = built
    m = yt.YOLOv3(num_classes=80).eval()
    st = engine.ModelState()
    dev = torch.device("cpu")
    plan = engine.Plan(engine.build_network_program(m, 32, 416), st, dev)
    ready = [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_FILTERS_READY]
    assert len(ready) == 24
    for i in ready:
        e = plan.table[i]
        pk = st.packed(plan.blocks[i], dev)
        assert L.lib().yolo_conv_pick_tile(C.byref(e.d)) == 15 and e.w_packed == pk.prepared["u4"].buf.data_ptr() and pk.prepared["u4"].stamp is None
        assert e.workspace_bytes >= L.lib().yolo_conv_workspace_bytes(C.byref(e.d)) > 0
    others = [i for i in range(len(plan.table)) if i not in ready]
    assert all(plan.table[i].w_packed == st.packed(plan.blocks[i], dev).w.data_ptr() for i in others)
    total = sum(pk.prepared["u4"].buf.numel() for per in st._packed.values() for pk in per.values() if "u4" in pk.prepared)
    assert total == 261_881_856
    plan2 = engine.Plan(engine.build_network_program(m, 8, 416), st, dev)
    assert sum(pk.prepared["u4"].buf.numel() for per in st._packed.values() for pk in per.values() if "u4" in pk.prepared) == total
    assert sum(1 for i in range(len(plan2.table)) if plan2.table[i].d.flags & L.FLAG_FILTERS_READY) == 24
    plan13 = engine.Plan(engine.build_network_program(m, 1, 416), st, dev, tile_override=13)
    assert not any(plan13.table[i].d.flags & L.FLAG_FILTERS_READY for i in range(len(plan13.table)))
