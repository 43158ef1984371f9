"""Winograd F(4x4, 3x3) with its 36 GEMMs on bf16 planes (conv_wino4s_f32.hip, YOLO_FLAG_WINO_SPLIT_BF16) through the C-ABI: against an
fp64 convolution and against the f32 GEMMs (tile 15 without the flag) on the same operands; the plane layout; bit equality where it is
promised; non-finite inputs."""
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
    """One 3x3 stride-1 layer on the device: operands, packed weights, U4 made once (and once more behind the packed weights)."""

    def __init__(self, L, B, H, W, cin, cout, residual=False, act=1, x_ld=None, x_off=0, y_ld=None, y_off=0, r_ld=None, r_off=0, seed=0):
        self.L, self.lib, self.dev, self.st = L, L.lib(), torch.device("cuda:0"), L.current_stream()
        self.B, self.H, self.W, self.cin, self.cout, self.residual, self.act = B, H, W, cin, cout, residual, act
        self.x_ld, self.x_off, self.y_ld, self.y_off = x_ld or cin, x_off, y_ld or cout, y_off
        self.r_ld, self.r_off = (r_ld or cout, r_off) if residual else (0, 0)
        g = torch.Generator().manual_seed(4150 + seed + B + H + W + cin + cout)
        self.x = torch.randn((B, H, W, self.x_ld), generator=g)
        self.w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
        self.scale, self.shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        self.y0 = torch.randn((B, H, W, self.y_ld), generator=g)
        self.r = torch.randn((B, H, W, self.r_ld), generator=g) if residual else None
        dev, lib, st = self.dev, self.lib, self.st
        self.xd, self.sd, self.shd = self.x.to(dev), self.scale.to(dev), self.shift.to(dev)
        self.rd = self.r.to(dev) if residual else None
        d = self.desc(0)
        packed = lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32)
        self.u4_off = (packed + 15) // 16 * 16
        self.wa = torch.empty(lib.yolo_wino4_appended_bytes(d), dtype=torch.uint8, device=dev)       # packed weights, then U4
        L.check(lib.yolo_pack_weights(self.w.to(dev).data_ptr(), self.wa.data_ptr(), cout, cin, 3, L.F32, st), "yolo_pack_weights")
        L.check(lib.yolo_wino4_filters(d, self.wa.data_ptr(), self.wa.data_ptr() + self.u4_off, st), "yolo_wino4_filters")
        self.u4 = self.wa[self.u4_off:].clone()                                                     # ... and U4 alone

    def desc(self, flags, B=None):
        L = self.L
        return L.ConvDesc(n=B or self.B, h=self.H, w=self.W, cin=self.cin, cout=self.cout, ksize=3, stride=1, x_ld=self.x_ld,
                          x_off=self.x_off, y_ld=self.y_ld, y_off=self.y_off, r_ld=self.r_ld, r_off=self.r_off, act=self.act,
                          out_mode=L.OUT_NHWC, dtype=L.F32, flags=(L.FLAG_RESIDUAL if self.residual else 0) | L.FLAG_NANCHECK | flags,
                          tile=15)

    def run(self, flags, x=None, ws=None, B=None, r=None):
        """(return code, y on the host, NaN flag, workspace) of one launch on finished filters; flags name the filter source."""
        L, lib, dev = self.L, self.lib, self.dev
        d = self.desc(flags, B)
        need = lib.yolo_conv_workspace_bytes(d)
        if ws is None:
            ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)      # NaN-ish garbage: the transform pass defines all that is read
        x = self.xd if x is None else x
        r = self.rd if r is None else r
        yd = self.y0[:d.n].clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        wp = self.wa if flags & L.FLAG_FILTERS_APPENDED else self.u4
        rc = lib.yolo_conv_fwd_ws(d, x.data_ptr(), wp.data_ptr(), self.sd.data_ptr(), self.shd.data_ptr(), r.data_ptr() if self.residual else 0,
                                  yd.data_ptr(), ws.data_ptr(), need, flag.data_ptr(), self.st)
        torch.cuda.synchronize()
        assert int(ws[need:].min()) == 0x7f or ws.numel() == need                  # nothing written past the stated size
        return rc, yd.cpu(), int(flag.item()), ws

    def reference(self):
        import torch.nn.functional as F
        xin = self.x[..., self.x_off:self.x_off + self.cin].double().permute(0, 3, 1, 2)
        ref = F.conv2d(xin, self.w.double(), padding=1) * self.scale.double().view(1, -1, 1, 1) + self.shift.double().view(1, -1, 1, 1)
        ref = F.leaky_relu(ref, 0.1) if self.act == 1 else (F.mish(ref) if self.act == 2 else ref)
        ref = ref.permute(0, 2, 3, 1)
        return ref + self.r[..., self.r_off:self.r_off + self.cout].double() if self.residual else ref

    def out(self, y):
        return y[..., self.y_off:self.y_off + self.cout]


# cin 64 (two K steps per xi), 96 (three: the ring of four slots wraps inside a pass at a different xi each time) and 160; cout 64 and
# 80 (a partial channel block); 8 x 8 and 9 x 7 at batch 1 (partial tiles on both edges, one workgroup, most tiles absent), 24 x 24 at
# batch 2 (72 tiles: a second tile block with 8 tiles); residual; ld / off views (the route-concat view); every activation
FP64_CASES = [  # (B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off)
    (1, 8, 8, 64, 64, False, 1, None, 0, None, 0, None, 0),
    (1, 9, 7, 96, 80, True, 2, None, 0, None, 0, None, 0),
    (2, 24, 24, 160, 80, False, 0, None, 0, None, 0, None, 0),
    (2, 24, 24, 64, 64, True, 1, 96, 32, 192, 128, 96, 8),
    (1, 9, 7, 160, 64, False, 1, None, 0, None, 0, None, 0),
    (1, 8, 8, 96, 80, True, 0, None, 0, None, 0, None, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FP64_CASES)
def test_split_gemms_against_fp64(yt, case, capsys):
    """max|err| / max|y| against an fp64 convolution: at most twice the figure of the f32 GEMMs (tile 15 without the flag) on the same
    inputs, the ratio bound of tests/test_gpu_split3.py, and at most 1e-5, the bar of the Winograd tests. The rest of the output
    buffer stays untouched; the workspace is the planes' size; a smaller one is refused."""
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off = case
    ly = Layer(L, B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off)
    ref = ly.reference()
    rc, y_f32, flag, _ = ly.run(L.FLAG_FILTERS_READY)
    assert rc == 0 and flag == 0, ly.lib.yolo_last_error()
    rc, y_split, flag, ws = ly.run(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16)
    assert rc == 0 and flag == 0, ly.lib.yolo_last_error()
    tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
    assert ws.numel() - 64 == 36 * cin * ((tiles + 63) // 64 * 64 + (cout + 63) // 64 * 64) * 6
    e_f32 = float((ly.out(y_f32).double() - ref).abs().max() / ref.abs().max())
    e_split = float((ly.out(y_split).double() - ref).abs().max() / ref.abs().max())
    with capsys.disabled():
        print(f"\nwino4 split {B}x{H}x{W} {cin}->{cout} res={int(residual)} act={act}: split {e_split:.3e}  f32 {e_f32:.3e}  ratio {e_split / e_f32:.2f}")
    assert e_split <= 2 * e_f32, (e_split, e_f32)
    assert e_split <= 1e-5, e_split
    keep = torch.ones(ly.y_ld, dtype=torch.bool)
    keep[ly.y_off:ly.y_off + cout] = False
    assert torch.equal(y_split[..., keep], ly.y0[..., keep])
    d = ly.desc(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16)
    need = ly.lib.yolo_conv_workspace_bytes(d)
    flagw = torch.zeros(1, dtype=torch.int32, device=ly.dev)
    yd = ly.y0.clone().to(ly.dev)
    assert ly.lib.yolo_conv_fwd_ws(d, ly.xd.data_ptr(), ly.u4.data_ptr(), ly.sd.data_ptr(), ly.shd.data_ptr(), ly.rd.data_ptr() if residual else 0,
                                   yd.data_ptr(), ws.data_ptr(), need - 16, flagw.data_ptr(), ly.st) == -4
    torch.cuda.synchronize()


def _plane_offsets(n_rows, cin, nkc, nblk):
    """Byte offsets of wino4_planes.h for every (xi, channel, row): [36][cin][n_rows] of plane 0 (the planes are 4096 bytes apart)."""
    xi = torch.arange(36).view(36, 1, 1)
    ci = torch.arange(cin).view(1, cin, 1)
    row = torch.arange(n_rows).view(1, 1, n_rows)
    r, c = row & 63, ci & 31
    g = (0x78 >> (2 * ((r >> 2) & 3))) & 3
    slot = ((c >> 3) ^ g) & 3
    return ((xi * nkc + (ci >> 5)) * nblk + (row >> 6)) * 12288 + r * 64 + slot * 16 + (c & 7) * 2


@pytest.mark.gpu
def test_planes_hold_the_exact_split_at_their_offsets(yt):
    """The workspace a flagged launch leaves behind, read back with the layout of wino4_planes.h written out here: hi + mid + lo of
    every element is, bit for bit, the fp32 V4 that the launch without the flag leaves (and the U4 the caller brought), hi and mid
    are the truncations the split promises, and the padding tiles and channels hold zeros."""
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout = 2, 24, 24, 96, 80
    ly = Layer(L, B, H, W, cin, cout, seed=5)
    _, _, _, ws32 = ly.run(L.FLAG_FILTERS_READY)
    _, _, _, wsp = ly.run(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16)
    T = B * 6 * 6
    Tpad, coutp, nkc = (T + 63) // 64 * 64, (cout + 63) // 64 * 64, cin // 32
    v32 = ws32[:36 * cin * Tpad * 4].cpu().view(torch.float32).view(36, cin // 4, Tpad, 4).permute(0, 1, 3, 2).reshape(36, cin, Tpad)
    u32 = ly.u4.cpu().view(torch.float32).view(36, cin // 4, coutp, 4).permute(0, 1, 3, 2).reshape(36, cin, coutp)
    planes = wsp[:-64].cpu().view(torch.int16)
    v_bytes = 36 * nkc * (Tpad // 64) * 12288
    for want, n_rows, base in ((v32, Tpad, 0), (u32, coutp, v_bytes)):
        off = (_plane_offsets(n_rows, cin, nkc, n_rows // 64) + base) // 2
        parts = [(planes[off + q * 2048].to(torch.int32) << 16).view(torch.float32) for q in range(3)]
        hi, mid, lo = parts
        assert torch.equal((hi.double() + mid.double() + lo.double()).float(), want)
        assert torch.equal(hi, (want.view(torch.int32) & -65536).view(torch.float32))
        assert torch.equal(mid, ((want - hi).view(torch.int32) & -65536).view(torch.float32))
        assert torch.equal(lo, (want - hi) - mid)
    assert float(v32[:, :, T:].abs().max()) == 0 and float(u32[:, :, cout:].abs().max()) == 0


@pytest.mark.gpu
def test_both_filter_sources_give_the_same_bits(yt):
    """A flagged launch on U4 of its own (YOLO_FLAG_FILTERS_READY) and one on U4 behind the packed weights (YOLO_FLAG_FILTERS_APPENDED)."""
    from yolo_for_turbines_amd import _lib as L
    ly = Layer(L, 2, 24, 24, 96, 80, residual=True, act=1, seed=6)
    rc, a, flag, _ = ly.run(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16)
    assert rc == 0 and flag == 0, ly.lib.yolo_last_error()
    rc, b, flag, _ = ly.run(L.FLAG_FILTERS_APPENDED | L.FLAG_WINO_SPLIT_BF16)
    assert rc == 0 and flag == 0, ly.lib.yolo_last_error()
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_an_image_does_not_depend_on_its_batch(yt):
    """Finite data: batch 1 against the same image inside batch 3 (where it shares its workgroup with both neighbours: 3 x 12 tiles)."""
    from yolo_for_turbines_amd import _lib as L
    ly = Layer(L, 3, 9, 13, 64, 80, residual=True, act=2, seed=7)
    f = L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16
    rc, y3, flag, _ = ly.run(f)
    assert rc == 0 and flag == 0, ly.lib.yolo_last_error()
    for n in range(3):
        rc, y1, flag, _ = ly.run(f, x=ly.xd[n:n + 1].contiguous(), B=1, r=ly.rd[n:n + 1].contiguous())
        assert rc == 0 and flag == 0
        # (y0 of the single launch is image 0's: compare the channels the launch writes)
        assert torch.equal(ly.out(y1[0]), ly.out(y3[n]))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_input_raises_the_flag(yt, bad):
    """One Inf / one NaN planted in x: bit 2 of the NaN flag, as the launch without the flag raises it on the same input."""
    from yolo_for_turbines_amd import _lib as L
    ly = Layer(L, 1, 9, 7, 64, 80, seed=8)
    x = ly.xd.clone()
    x[0, 4, 3, 17] = bad
    assert ly.run(L.FLAG_FILTERS_READY, x=x)[2] & 2
    assert ly.run(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16, x=x)[2] & 2


@pytest.mark.gpu
def test_large_finite_values_make_no_new_nan(yt):
    """Values near FLT_MAX / 64 planted in x, of both signs, in the corner, on an edge and inside, next to each other and alone (the
    transform multiplies a single value by at most 6.25, a whole patch of them by at most 42.25: V4 stays finite, and the split of a
    finite value is finite): an output that is NaN with the flag is NaN without it."""
    from yolo_for_turbines_amd import _lib as L
    ly = Layer(L, 1, 9, 7, 64, 80, act=0, seed=9)
    big = 0.99 * 3.4028234e38 / 64
    x = ly.xd.clone()
    for (r, c, ch, sgn) in ((0, 0, 0, 1), (4, 3, 17, -1), (4, 4, 17, 1), (8, 6, 63, -1), (3, 0, 40, 1), (5, 5, 33, -1)):
        x[0, r, c, ch] = sgn * big
    _, y_f32, _, _ = ly.run(L.FLAG_FILTERS_READY, x=x)
    _, y_split, _, _ = ly.run(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16, x=x)
    new_nan = torch.isnan(y_split) & ~torch.isnan(y_f32)
    assert not bool(new_nan.any()), (int(new_nan.sum()), int(torch.isnan(y_f32).sum()))
    assert float(torch.nan_to_num(y_split, nan=0.0, posinf=3e38, neginf=-3e38).abs().max()) > 1e30                         # (the planted values did reach the output)
