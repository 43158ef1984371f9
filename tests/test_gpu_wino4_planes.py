"""YOLO_FLAG_FILTER_PLANES through the C-ABI: the bf16 planes of the Winograd F(4x4) filters made once (yolo_wino4_filter_planes) give
the bits and the bytes of the launch that splits its filters itself, and the engine keeps them in step with the weights; the half
workgroups and the block map of conv_wino4s_f32 give the bits of whole workgroups, and fp32 accuracy against an fp64 convolution."""
import pytest
import torch


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return pkg


class Layer:
    """One 3x3 stride-1 layer on the device: operands, and one buffer of packed weights, U4 behind them (YOLO_FLAG_FILTERS_APPENDED),
    the planes of that U4 behind it, and 64 bytes of 0x55 behind those. YOLO_FLAG_FILTERS_READY launches point at the U4 inside."""

    def __init__(self, L, B, H, W, cin, cout, residual=False, act=1, seed=0):
        self.L, self.lib, self.dev, self.st = L, L.lib(), torch.device("cuda:0"), L.current_stream()
        self.B, self.H, self.W, self.cin, self.cout, self.residual, self.act = B, H, W, cin, cout, residual, act
        g = torch.Generator().manual_seed(4160 + seed + B + H + W + cin + cout)
        dev, lib, st = self.dev, self.lib, self.st
        self.xd = torch.randn((B, H, W, cin), generator=g).to(dev)
        w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
        self.sd, self.shd = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)
        self.rd = torch.randn((B, H, W, cout), generator=g).to(dev) if residual else None
        d = self.desc(0)
        self.na, self.nu, self.npl = lib.yolo_wino4_appended_bytes(d), lib.yolo_wino4_filter_bytes(d), lib.yolo_wino4_filter_plane_bytes(d)
        assert self.npl == 36 * cin * ((cout + 63) // 64 * 64) * 6
        self.buf = torch.full((self.na + self.npl + 64,), 0x55, dtype=torch.uint8, device=dev)
        self.u4_at = self.buf.data_ptr() + self.na - self.nu
        L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), self.buf.data_ptr(), cout, cin, 3, L.F32, st), "yolo_pack_weights")
        L.check(lib.yolo_wino4_filters(d, self.buf.data_ptr(), self.u4_at, st), "yolo_wino4_filters")
        L.check(lib.yolo_wino4_filter_planes(d, self.u4_at, self.u4_at + self.nu, st), "yolo_wino4_filter_planes")
        torch.cuda.synchronize()

    def desc(self, flags, n=None):
        L = self.L
        return L.ConvDesc(n=n or self.B, h=self.H, w=self.W, cin=self.cin, cout=self.cout, ksize=3, stride=1, x_ld=self.cin, y_ld=self.cout,
                          r_ld=self.cout if self.residual else 0, act=self.act, out_mode=L.OUT_NHWC, dtype=L.F32,
                          flags=(L.FLAG_RESIDUAL if self.residual else 0) | L.FLAG_NANCHECK | flags, tile=15)

    def run(self, flags, first=0, n=None):
        """(y on the host, workspace with 64 bytes behind its stated size) of one launch (of images first .. first + n - 1); the
        workspace starts as 0x7f"""
        L, lib, dev = self.L, self.lib, self.dev
        d = self.desc(flags, n)
        need = lib.yolo_conv_workspace_bytes(d)
        ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)
        yd = torch.zeros((d.n, self.H, self.W, self.cout), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        wp = self.buf.data_ptr() if flags & L.FLAG_FILTERS_APPENDED else self.u4_at
        rc = lib.yolo_conv_fwd_ws(d, self.xd[first:].data_ptr(), wp, self.sd.data_ptr(), self.shd.data_ptr(),
                                  self.rd[first:].data_ptr() if self.residual else 0, yd.data_ptr(), ws.data_ptr(),
                                  need, flag.data_ptr(), self.st)
        torch.cuda.synchronize()
        assert rc == 0 and int(flag.item()) == 0, lib.yolo_last_error()
        return yd.cpu(), ws.cpu()


# 24 x 24 at batch 2: 72 tiles, a second tile block with 8 tiles, three K chunks, a partial channel block; 9 x 13 at batch 3: partial
# tiles on both edges, Mish; 4 x 4: one tile, one chunk (the ring's prologue alone)
CASES = [(2, 24, 24, 96, 80, True, 1), (3, 9, 13, 64, 80, True, 2), (1, 4, 4, 32, 64, False, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_planes_once_equal_planes_per_launch(yt, case):
    """With either filter flag: the same output bits; the bytes yolo_wino4_filter_planes wrote are the U region the per-launch
    workspace holds, and nothing behind them is written; with the flag the launch leaves its U region, and what lies behind the
    stated size, as they were. The flag without YOLO_FLAG_WINO_SPLIT_BF16 is ignored: the bits of the f32 GEMMs."""
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, act = case
    ly = Layer(L, B, H, W, cin, cout, residual, act)
    S, P = L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTER_PLANES
    tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
    v_bytes = 36 * cin * ((tiles + 63) // 64 * 64) * 6
    planes = ly.buf[ly.na:ly.na + ly.npl].cpu()
    assert int(ly.buf[ly.na + ly.npl:].min()) == 0x55 and int(ly.buf[ly.na + ly.npl:].max()) == 0x55
    for filt in (L.FLAG_FILTERS_READY, L.FLAG_FILTERS_APPENDED):
        y_per, ws_per = ly.run(filt | S)
        y_once, ws_once = ly.run(filt | S | P)
        assert ws_per.numel() == ws_once.numel() == v_bytes + ly.npl + 64
        assert float(y_per.abs().max()) > 0
        assert torch.equal(y_once.view(torch.int32), y_per.view(torch.int32))
        assert torch.equal(ws_per[v_bytes:v_bytes + ly.npl], planes)
        assert torch.equal(ws_once[:v_bytes], ws_per[:v_bytes])
        assert int(ws_once[v_bytes:].min()) == 0x7f and int(ws_once[v_bytes:].max()) == 0x7f
        assert int(ws_per[v_bytes + ly.npl:].min()) == 0x7f and int(ws_per[v_bytes + ly.npl:].max()) == 0x7f
        y_f32, _ = ly.run(filt)
        y_f32p, _ = ly.run(filt | P)
        assert torch.equal(y_f32p.view(torch.int32), y_f32.view(torch.int32))


def _model(yt, sd, mode):
    m = yt.YOLOv3(num_classes=2)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    m._engine.wino4_split = mode
    return m


@pytest.mark.gpu
def test_engine_keeps_the_planes_in_step_with_the_weights(yt):
    """224 x 224 at batch 1, the smallest input of the tile-15 tests (56 x 56 and 28 x 28 maps): under ``wino4_split = "all"`` launches
    carry 128 | 256. After an in-place weight change the prediction equals a fresh model's, and "all" (planes once) and "perlaunch"
    (every launch splitting its filters) predict the same bits, before and after the change."""
    from oracle import net as onet
    from yolo_for_turbines_amd import _lib as L
    from yolo_for_turbines_amd.model import CNNBlock
    sd = onet.synth_state_dict(11, 3, 2, gain=0.8)
    x = onet.synth_input(12, 1, 224).cuda()
    S, P = L.FLAG_WINO_SPLIT_BF16, L.FLAG_FILTER_PLANES
    with torch.no_grad():
        m, per = _model(yt, sd, "all"), _model(yt, sd, "perlaunch")
        before = [o.clone() for o in m(x)]
        plan = next(iter(m._engine._plans.values()))
        both = [i for i in range(len(plan.table)) if plan.table[i].d.flags & (S | P) == S | P]
        assert len(both) >= 4, both
        for a, b in zip(before, per(x)):
            assert torch.equal(a, b)
        pplan = next(iter(per._engine._plans.values()))
        assert [pplan.table[i].d.flags for i in range(len(pplan.table))] == [plan.table[i].d.flags & ~P for i in range(len(plan.table))]
        for mm in (m, per):
            for k, b in enumerate(b for b in mm.modules() if isinstance(b, CNNBlock) and b.conv.kernel_size[0] == 3):
                b.conv.weight.mul_(1.0 + 0.03 * ((k % 5) - 2.5))
        after = [o.clone() for o in m(x)]
        fresh = _model(yt, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, "all")
        want = fresh(x)
        assert any(not torch.equal(a, b) for a, b in zip(after, before))
        for a, w_, p_ in zip(after, want, per(x)):
            assert torch.equal(a, w_) and torch.equal(a, p_)


# ---------------------------------------------------------------------------------------------- half workgroups of conv_wino4s_f32
def _cut(L, d):
    import ctypes as C
    whole, half = C.c_int(-1), C.c_int(-1)
    L.check(L.lib().yolo_conv_wino4_blocks(d, C.byref(whole), C.byref(half)), "yolo_conv_wino4_blocks")
    return whole.value, half.value


class Maps:
    """B maps of 8 x 8, 32 -> 64 channels (4 tiles each: 16 images are one tile block, one channel block), filters and planes made once."""

    def __init__(self, L, B, residual, seed):
        self.L, self.lib, self.dev, self.st, self.residual = L, L.lib(), torch.device("cuda:0"), L.current_stream(), residual
        g = torch.Generator().manual_seed(seed)
        dev, lib = self.dev, self.lib
        self.x = torch.randn((B, 8, 8, 32), generator=g).to(dev)
        w = torch.randn((64, 32, 3, 3), generator=g) * (1.0 / 288) ** 0.5
        self.scale, self.shift = (torch.rand(64, generator=g) + 0.5).to(dev), (torch.randn(64, generator=g) * 0.1).to(dev)
        self.r = torch.randn((B, 8, 8, 64), generator=g).to(dev) if residual else None
        d = self.desc(1)
        wp = torch.empty(lib.yolo_packed_weight_bytes(64, 32, 3, L.F32), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), wp.data_ptr(), 64, 32, 3, L.F32, self.st), "yolo_pack_weights")
        nu = lib.yolo_wino4_filter_bytes(d)
        self.u4 = torch.empty(nu + lib.yolo_wino4_filter_plane_bytes(d), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_wino4_filters(d, wp.data_ptr(), self.u4.data_ptr(), self.st), "yolo_wino4_filters")
        L.check(lib.yolo_wino4_filter_planes(d, self.u4.data_ptr(), self.u4.data_ptr() + nu, self.st), "yolo_wino4_filter_planes")

    def desc(self, n):
        L = self.L
        return L.ConvDesc(n=n, h=8, w=8, cin=32, cout=64, ksize=3, stride=1, x_ld=32, y_ld=64, r_ld=64 if self.residual else 0, act=1,
                          out_mode=L.OUT_NHWC, dtype=L.F32, tile=15, flags=(L.FLAG_RESIDUAL if self.residual else 0) | L.FLAG_NANCHECK
                          | L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16 | L.FLAG_FILTER_PLANES)

    def run(self, first, n):
        """images first .. first + n - 1 as a launch of their own"""
        L, lib, dev = self.L, self.lib, self.dev
        d = self.desc(n)
        need = lib.yolo_conv_workspace_bytes(d)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        y = torch.zeros((n, 8, 8, 64), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.yolo_conv_fwd_ws(d, self.x[first:].data_ptr(), self.u4.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(),
                                     self.r[first:].data_ptr() if self.residual else 0, y.data_ptr(), ws.data_ptr(), need, flag.data_ptr(), self.st),
                "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        return y


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True])
def test_whole_and_half_workgroups_give_the_same_bits(yt, residual):
    """2,064 images are 129 tile blocks, more than half the compute units, so every block is whole; the first 16 images alone are one
    tile block, cut into halves. The 16 images' outputs agree bit for bit."""
    from yolo_for_turbines_amd import _lib as L
    mp = Maps(L, 2064, residual, 78 + residual)
    assert _cut(L, mp.desc(2064)) == (129, 0) and _cut(L, mp.desc(16)) == (0, 1)
    whole, halves = mp.run(0, 2064)[:16].cpu(), mp.run(0, 16).cpu()
    assert float(whole.abs().max()) > 0
    assert torch.equal(whole.view(torch.int32), halves.view(torch.int32))


@pytest.mark.gpu
def test_a_mixed_cut_gives_the_bits_of_its_parts(yt):
    """The smallest batch for which yolo_conv_wino4_blocks reports whole and half tile blocks in one launch (found by asking it, one
    more tile block at a time): its last 16 images, 15 of them in the last whole block and one in the block in halves, equal their
    own launch."""
    from yolo_for_turbines_amd import _lib as L
    probe = Maps(L, 1, True, 90)
    B = next(b for b in (16 * k + 1 for k in range(1, 4096)) if min(_cut(L, probe.desc(b))) > 0)
    whole, half = _cut(L, probe.desc(B))
    assert whole > 0 and half > 0 and whole + half == (4 * B + 63) // 64
    mp = Maps(L, B, True, 91)
    mixed, alone = mp.run(0, B)[B - 16:].cpu(), mp.run(B - 16, 16).cpu()
    assert _cut(L, mp.desc(16)) == (0, 1)
    assert float(mixed.abs().max()) > 0
    assert torch.equal(mixed.view(torch.int32), alone.view(torch.int32))


@pytest.mark.gpu
def test_the_block_map_of_an_all_halves_launch_gives_the_same_bits(yt):
    """13 x 13 maps, 32 -> 1024 channels: 32 images are 8 tile blocks x 16 channel blocks, all in halves where that is at most half the
    compute units, and then mapped 4 tile blocks x 4 channel blocks x both halves per XCD; 16 images are 4 x 16, on the plain map.
    Index arithmetic only: both halves of the batch equal their own launches. (On a device that cuts differently the test still
    compares two launches of the same tiles.)"""
    from yolo_for_turbines_amd import _lib as L
    ly = Layer(L, 32, 13, 13, 32, 1024, True, 1, seed=3)
    f = L.FLAG_FILTERS_APPENDED | L.FLAG_WINO_SPLIT_BF16 | L.FLAG_FILTER_PLANES
    both, _ = ly.run(f)
    assert float(both.abs().max()) > 0
    for first in (0, 16):
        part, _ = ly.run(f, first=first, n=16)
        assert torch.equal(part.view(torch.int32), both[first:first + 16].view(torch.int32))


HALF_CASES = [  # (B, H, W, cin, cout, residual, act, y_ld, r_ld, r_off): test_gpu_wino4_tail.py::HALF_CASES with cin a multiple of 32
    (1, 4, 4, 32, 64, False, 1, 64, 0, 0),           # one tile: the second half workgroup has no valid tile and writes nothing
    (5, 52, 52, 128, 64, True, 1, 64, 64, 0),        # 845 tiles = 14 tile blocks; the last has 13 tiles: ragged first half, empty second
    (2, 6, 8, 128, 84, True, 1, 84, 96, 8),          # residual view; ragged channel block
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", HALF_CASES)
def test_half_workgroups_against_fp64(yt, case, capsys):
    """Launches that are all halves (asserted through yolo_conv_wino4_blocks), on filter planes made once: max|err| / max|y| against
    an fp64 convolution at most 1e-5 and at most twice the f32 GEMMs' on the same operands; the rest of the output buffer
    untouched; a NaN in the last tile raises bit 2."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, act, y_ld, r_ld, r_off = case
    g = torch.Generator().manual_seed(2400 + cin + cout + H + W + B)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, W, cin), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    y0 = torch.randn((B, H, W, y_ld + 4), generator=g)          # four channels behind the layer's: must stay as they are
    r = torch.randn((B, H, W, r_ld), generator=g) if residual else None
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1).permute(0, 2, 3, 1)
    if residual:
        ref = ref + r[..., r_off:r_off + cout].double()
    xd, sd, shd = x.to(dev), scale.to(dev), shift.to(dev)
    rd = r.to(dev) if residual else None

    def desc(flags):
        return L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=3, stride=1, x_ld=cin, y_ld=y_ld + 4, r_ld=r_ld, r_off=r_off, act=act,
                          out_mode=L.OUT_NHWC, dtype=L.F32, tile=15, flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK | flags)
    d = desc(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16 | L.FLAG_FILTER_PLANES)
    assert _cut(L, d) == (0, (B * ((H + 3) // 4) * ((W + 3) // 4) + 63) // 64)
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).data_ptr(), wp.data_ptr(), cout, cin, 3, L.F32, st))
    nu = lib.yolo_wino4_filter_bytes(d)
    u4 = torch.empty(nu + lib.yolo_wino4_filter_plane_bytes(d), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_wino4_filters(d, wp.data_ptr(), u4.data_ptr(), st), "yolo_wino4_filters")
    L.check(lib.yolo_wino4_filter_planes(d, u4.data_ptr(), u4.data_ptr() + nu, st), "yolo_wino4_filter_planes")

    def run(dd, xp):
        need = lib.yolo_conv_workspace_bytes(dd)
        ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)
        yd = y0.clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.yolo_conv_fwd_ws(dd, xp.data_ptr(), u4.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                  yd.data_ptr(), ws.data_ptr(), need, flag.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == 0, lib.yolo_last_error()
        assert int(ws[need:].min()) == 0x7f                          # nothing written past the stated workspace
        return yd.cpu(), int(flag.item())

    got, flag = run(d, xd)
    f32, flag32 = run(desc(L.FLAG_FILTERS_READY), xd)
    assert flag == 0 and flag32 == 0
    err = float((got[..., :cout].double() - ref).abs().max() / ref.abs().max())
    err32 = float((f32[..., :cout].double() - ref).abs().max() / ref.abs().max())
    with capsys.disabled():
        print(f"\nwino4 split halves {B}x{H}x{W} {cin}->{cout}: split {err:.3e}  f32 {err32:.3e}  ratio {err / err32:.2f}")
    assert err <= 1e-5, err
    assert err <= 2 * err32, (err, err32)
    assert torch.equal(got[..., cout:], y0[..., cout:])              # neighbouring channels of the buffer untouched
    xn = xd.clone()
    xn[B - 1, H - 1, W - 1, 0] = float("nan")                        # the last tile: in the ragged half
    assert run(d, xn)[1] & 2
