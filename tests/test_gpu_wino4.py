"""Winograd F(4x4, 3x3) (conv_wino4_f32.hip, tile 15) through the C-ABI against an fp64 convolution of the same operands."""
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


WINO4_CASES = [  # (B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off)
    (2, 13, 13, 128, 128, False, 1, 128, 0, 128, 0, 0, 0),         # H, W not multiples of 4: the last tile row / column writes one pixel
    (3, 9, 7, 256, 512, True, 2, 256, 0, 512, 0, 512, 0),          # H != W, both odd, Mish + residual
    (2, 6, 8, 128, 84, True, 1, 128, 0, 84, 0, 96, 8),             # cout not a multiple of 64 (ragged channel block); residual view
    (1, 4, 4, 4, 64, False, 1, 4, 0, 64, 0, 0, 0),                 # one tile, cin = 4: one stage with a zero padding plane
    (1, 5, 6, 64, 64, False, 0, 64, 0, 64, 0, 0, 0),               # eight stages, identity epilogue
    (1, 24, 20, 256, 128, False, 0, 384, 128, 384, 256, 0, 0),     # reads a slice of a concat buffer, writes into one
    (5, 52, 52, 128, 64, True, 1, 128, 0, 64, 0, 64, 0),           # 845 tiles: 14 tile blocks over the 8 XCD lanes of the block map
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINO4_CASES)
def test_fp32_winograd4_kernel(yt, case):
    """tile 15: ragged tile and channel blocks, odd and non-square maps, 1- and 8-stage K, ld / off views, residual, every activation;
    the rest of the output buffer untouched, nothing written past the stated workspace, a too-small workspace refused (tile 15) or
    routed elsewhere (tile 0); the NaN flag. Bar: 1e-5 of max|y| against fp64 (the north-star bar is 1e-3)."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off = case
    g = torch.Generator().manual_seed(1900 + cin + cout + H + W + B)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, W, x_ld), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    y0 = torch.randn((B, H, W, y_ld), generator=g)
    r = torch.randn((B, H, W, r_ld), generator=g) if residual else None
    xd, sd, shd, wd = x.to(dev), scale.to(dev), shift.to(dev), w.to(dev)
    rd = r.to(dev) if residual else None
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(wd.data_ptr(), wp.data_ptr(), cout, cin, 3, L.F32, st))
    xin = x[..., x_off:x_off + cin].double().permute(0, 3, 1, 2)
    ref = F.conv2d(xin, w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1) if act == 1 else (F.mish(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + r[..., r_off:r_off + cout].double()

    def desc(tile):
        return L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=3, stride=1, x_ld=x_ld, x_off=x_off, y_ld=y_ld, y_off=y_off,
                          r_ld=r_ld, r_off=r_off, act=act, out_mode=L.OUT_NHWC, dtype=L.F32,
                          flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK, tile=tile)

    def run(tile, ws_ptr, ws_bytes, xp=None, y_init=None):
        yd = (y0 if y_init is None else y_init).clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.yolo_conv_fwd_ws(desc(tile), (xp if xp is not None else xd).data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(),
                                  rd.data_ptr() if residual else 0, yd.data_ptr(), ws_ptr, ws_bytes, flag.data_ptr(), st)
        torch.cuda.synchronize()
        return rc, yd.cpu(), int(flag.item())

    need = lib.yolo_conv_workspace_bytes(desc(15))
    tiles = B * ((H + 3) // 4) * ((W + 3) // 4)
    c4p = (cin // 4 + 1) // 2 * 2
    assert need == 36 * c4p * ((tiles + 63) // 64 * 64 + (cout + 63) // 64 * 64) * 16
    ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)          # NaN-ish garbage: the transform pass must define all it reads
    rc, got, flag = run(15, ws.data_ptr(), need)
    assert rc == 0 and flag == 0, lib.yolo_last_error()
    err = float((got[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err
    keep = torch.ones(y_ld, dtype=torch.bool)
    keep[y_off:y_off + cout] = False
    assert torch.equal(got[..., keep], y0[..., keep])                # neighbouring channels of the buffer untouched
    assert int(ws[need:].min()) == 0x7f                              # nothing written past the stated size
    # too small a workspace: tile 15 refuses; tile 0 takes another kernel (F(2x2) or the direct one) and computes the same
    assert run(15, ws.data_ptr(), need - 16)[0] == -4
    rc, got0, flag = run(0, ws.data_ptr(), need - 16)
    assert rc == 0 and flag == 0
    assert float((got0[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max()) <= 1e-5
    # a NaN in the input reaches the flag
    xn = xd.clone()
    xn[0, 0, 0, x_off] = float("nan")
    assert run(15, ws.data_ptr(), need, xp=xn)[2] & 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 12, 12, 128, 256, False), (3, 13, 9, 256, 64, True), (1, 52, 52, 64, 96, True)])
def test_fp32_winograd4_input_gradient(yt, case):
    """The stride-1 3x3 input gradient through tile 15: the filter transform reads the row-major section of
    `yolo_pack_weights_dgrad(flip = 1)`, dx = conv_transpose(dz, w) [+ the gradient already in dx]. Reference: fp64."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, accumulate = case
    g = torch.Generator().manual_seed(177 + cin + cout + H)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    coutp = (cout + 31) // 32 * 32
    dz = torch.zeros((B, H, W, coutp))
    dz[..., :cout] = torch.randn((B, H, W, cout), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
    dx0 = torch.randn((B, H, W, cin), generator=g)
    ref = F.conv_transpose2d(dz[..., :cout].double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    if accumulate:
        ref = ref + dx0.double()
    wp = torch.empty(lib.yolo_packed_dgrad_bytes(cout, cin, 3, 1, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights_dgrad(w.to(dev).data_ptr(), wp.data_ptr(), cout, cin, 3, 1, L.F32, st))
    ones, zeros = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    d = L.ConvDesc(n=B, h=H, w=W, cin=coutp, cout=cin, ksize=3, stride=1, x_ld=coutp, x_off=0, y_ld=cin, y_off=0, r_ld=cin, r_off=0,
                   act=L.ACT_NONE, out_mode=L.OUT_NHWC, dtype=L.F32, flags=L.FLAG_RESIDUAL if accumulate else 0, tile=15)
    need = lib.yolo_conv_workspace_bytes(d)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    dx = dx0.clone().to(dev)
    L.check(lib.yolo_conv_fwd_ws(d, dz.to(dev).data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), dx.data_ptr() if accumulate else 0,
                                 dx.data_ptr(), ws.data_ptr(), need, 0, st), "yolo_conv_fwd_ws(dgrad, tile 15)")
    torch.cuda.synchronize()
    err = float((dx.cpu().double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err


def test_winograd4_pick_is_shape_only(built):
    """The heuristic looks at (H, W, cin, cout), never at the batch: the same tile and the same kernel for n = 1 and n = 32;
    F(4x4) (tile 15) on the 104 x 104, 52 x 52 and 26 x 26 layers of the 416 network, F(2x2) (tile 13) on 13 x 13 (tile padding)."""
    lib = built.lib()
    for hw, cin, cout, want in ((104, 64, 128, 15), (52, 128, 256, 15), (26, 256, 512, 15), (13, 512, 1024, 13), (76, 128, 256, 15),
                                (19, 512, 1024, 13), (38, 256, 512, 15)):
        picks = []
        for n in (1, 32):
            d = built.ConvDesc(n=n, h=hw, w=hw, cin=cin, cout=cout, ksize=3, stride=1, x_ld=cin, y_ld=cout, dtype=built.F32, tile=0)
            picks.append(lib.yolo_conv_pick_tile(d))
            if picks[-1] == 15:                                     # the workspace of the chosen kernel: V4 + U4
                tiles = n * ((hw + 3) // 4) ** 2
                assert lib.yolo_conv_workspace_bytes(d) == 36 * (cin // 4) * ((tiles + 63) // 64 * 64 + (cout + 63) // 64 * 64) * 16
        assert picks == [want, want], (hw, picks)
