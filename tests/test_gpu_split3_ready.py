"""YOLO_FLAG_SPLIT_WEIGHTS_READY: conv_split3_f32 on weights split into their bf16 planes once (yolo_split3_weights) — the same
bits as the launch that splits them itself, the documented layout of the prepared buffer (packed weights, planes, non-finite table),
preparing in place, Inf / NaN, refusals, and the eval plan."""

import numpy as np
import pytest
import torch

from tests import test_gpu_split3 as s3

CASES, SPLIT_TILES = s3.CASES, s3.SPLIT_TILES


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


def _desc(L, c, ops, flags, tile, code):
    x, r = ops[0], ops[4]
    return L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=x.shape[-1],
                      x_off=c["x_off"], y_ld=c["cout"] + c["y_pad"], y_off=c["y_off"], r_ld=r.shape[-1] if r is not None else 0,
                      r_off=c["r_off"], act=c["act"], out_mode=c["out"], dtype=code,
                      flags=(L.FLAG_RESIDUAL if r is not None else 0) | L.FLAG_NANCHECK | flags, tile=tile)


def _prepared(L, c, w):
    """(prepared buffer, packed weights), both on the device, of weights w (cout, cin, k, k): yolo_pack_weights, then
    yolo_split3_weights into a buffer of its own."""
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    wp = torch.empty(lib.yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).contiguous().data_ptr(), wp.data_ptr(), c["cout"], c["cin"], c["k"], L.F32, st), "pack")
    d = L.ConvDesc(n=1, h=8, w=8, cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=c["cin"], y_ld=c["cout"], dtype=L.F32)
    n = lib.yolo_split3_weight_bytes(d)
    assert n > 0
    buf = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    L.check(lib.yolo_split3_weights(d, wp.data_ptr(), buf.data_ptr(), st), "yolo_split3_weights")
    torch.cuda.synchronize()
    return buf, wp


def _launch(L, c, ops, flags, tile, ready=None, dtype=None, ws=False):
    """One launch of case c like test_gpu_split3._launch; ready: the prepared buffer that stands in for the packed weights."""
    if ready is None:
        return s3._launch(L, c, ops, flags, tile, dtype=dtype, ws=ws)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x, w, scale, shift, r, y0 = ops
    xd, sc, sh, yd = x.to(dev), scale.to(dev), shift.to(dev), y0.to(dev)
    rd = r.to(dev) if r is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = _desc(L, c, ops, flags, tile, L.F32 if dtype is None else dtype)
    if ws:
        need = lib.yolo_conv_workspace_bytes(d)
        wsb = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        rc = lib.yolo_conv_fwd_ws(d, xd.data_ptr(), ready.data_ptr(), sc.data_ptr(), sh.data_ptr(), L.ptr(rd), yd.data_ptr(), wsb.data_ptr(),
                                  need, flag.data_ptr(), st)
    else:
        rc = lib.yolo_conv_fwd(d, xd.data_ptr(), ready.data_ptr(), sc.data_ptr(), sh.data_ptr(), L.ptr(rd), yd.data_ptr(), flag.data_ptr(), st)
    torch.cuda.synchronize()
    return yd.cpu(), int(flag.item()), rc


def _table(L, c, buf):
    """The non-finite words behind the planes, one per 32 output channels of cout_pad128."""
    cp = (c["cout"] + 127) // 128 * 128
    return buf.cpu().numpy()[-(cp // 32) * 4:].view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_prepared_launch_has_the_bits_of_the_in_flight_launch(L, name):
    """Every tile, and the heuristic: SPLIT_BF16 | SPLIT_WEIGHTS_READY on the prepared buffer writes the output buffer that SPLIT_BF16
    alone writes on the packed weights, bit for bit, with the same NaN flag. The order of additions of an element does not depend on
    the tile, so every tile's output equals the heuristic's too."""
    c, ops, _ = s3._shared(name)
    buf, _ = _prepared(L, c, ops[1])
    outs = {}
    for tile in (1, 2, 4, 0):
        want, flag0, rc0 = _launch(L, c, ops, L.FLAG_SPLIT_BF16, tile)
        got, flag, rc = _launch(L, c, ops, L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY, tile, ready=buf)
        assert rc0 == 0 and rc == 0, L.lib().yolo_last_error()
        assert flag == flag0 == 0
        assert torch.equal(got, want), tile
        outs[tile] = got
    assert all(torch.equal(outs[t], outs[0]) for t in (1, 2, 4))


def _host_planes(w):
    """numpy restatement of yolo_split3_weights: [K step][hi, mid, lo][cout_pad128][four 16-byte slots of 8 bf16, slot s of channel n
    at s ^ ((n >> 2) & 3)], then cout_pad128 / 32 zero words. Truncation split: mask the low 16 bits, subtract, twice."""
    cout, cin, k, _ = w.shape
    cp, K = (cout + 127) // 128 * 128, k * k * cin
    wm = np.zeros((cp, K), dtype=np.float32)
    wm[:cout] = w.permute(0, 2, 3, 1).reshape(cout, K).numpy()          # K index = (kh * k + kw) * cin + ci
    mask = np.uint32(0xffff0000)
    hi = wm.view(np.uint32) & mask
    r1 = wm - hi.view(np.float32)
    mid = r1.view(np.uint32) & mask
    r2 = r1 - mid.view(np.float32)
    lo = r2.view(np.uint32) & mask
    assert np.array_equal(hi.view(np.float32).astype(np.float64) + mid.view(np.float32) + lo.view(np.float32), wm.astype(np.float64))
    planes = (np.stack([hi, mid, lo]) >> np.uint32(16)).astype(np.uint16)           # [3][cp][K]
    rows = planes.reshape(3, cp, K // 32, 4, 8).transpose(2, 0, 1, 3, 4)          # [KT][3][cp][slot][8]
    out = np.empty_like(rows)
    n = np.arange(cp)
    for s in range(4):
        out[:, :, n, s ^ ((n >> 2) & 3), :] = rows[:, :, n, s, :]
    return np.concatenate([np.frombuffer(out.astype("<u2").tobytes(), dtype=np.uint8), np.zeros(cp // 32 * 4, dtype=np.uint8)])


def _planes_offset(L, c):
    return (L.lib().yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], L.F32) + 15) // 16 * 16


@pytest.mark.gpu
@pytest.mark.parametrize("cout,cin,k", [(24, 96, 1), (255, 256, 1), (96, 32, 3)])
def test_prepared_buffer_is_the_documented_layout(L, cout, cin, k):
    """The downloaded buffer is the packed weights, byte for byte, and behind them (from their size rounded up to 16) the host
    model byte for byte: split, K-step-major planes, swizzled slots, zero rows up to cout_pad128, and an all-clear non-finite
    table. Its size is the header's formula. Prepared in place, in a packed buffer with that much room, it holds the same bytes."""
    c = s3._case(1, 8, 8, cin, cout, k, 1)
    w = s3._operands(c, 77 + cout)[1]
    buf, wp = _prepared(L, c, w)
    want = _host_planes(w)
    cp = (cout + 127) // 128 * 128
    off = _planes_offset(L, c)
    assert buf.numel() == off + k * k * cin // 32 * 3 * cp * 64 + cp // 32 * 4 == off + want.size
    got = buf.cpu().numpy()
    assert not _table(L, c, buf).any()
    assert np.array_equal(got[:wp.numel()], wp.cpu().numpy())
    assert np.array_equal(got[off:], want)
    lib, st = L.lib(), L.current_stream()
    both = torch.full((buf.numel(),), 0x5A, dtype=torch.uint8, device=buf.device)
    both[:wp.numel()] = wp
    d = L.ConvDesc(n=1, h=8, w=8, cin=cin, cout=cout, ksize=k, stride=1, x_ld=cin, y_ld=cout, dtype=L.F32)
    L.check(lib.yolo_split3_weights(d, both.data_ptr(), both.data_ptr(), st), "in place")
    assert lib.yolo_split3_weights(d, both.data_ptr(), both.data_ptr() + 16, st) == -1          # overlapping and not the same: refused
    torch.cuda.synchronize()
    assert np.array_equal(both.cpu().numpy()[:wp.numel()], got[:wp.numel()]) and np.array_equal(both.cpu().numpy()[off:], got[off:])


def _same_with_nans(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1_k96_straddle", "3x3s2_13x13"])
def test_inf_and_nan_take_the_exact_path_where_the_in_flight_kernel_does(L, name):
    """-Inf, then NaN, in one weight: the table marks exactly that weight's group of 32 output channels, and the prepared launch
    equals the in-flight flagged launch bit for bit (NaNs by position), NaN flag included, on every tile. The same with the
    value in x, which the A side's own check still finds."""
    c, ops, _ = s3._shared(name)
    for where, value in (("w", float("-inf")), ("w", float("nan")), ("x", float("inf")), ("x", float("nan"))):
        x, w, scale, shift, r, y0 = (t.clone() if t is not None else None for t in ops)
        if where == "x":
            x[1, c["h"] // 2, 3, c["x_off"] + 5] = value
            x[0, 0, 0, c["x_off"]] = value
        else:
            w[c["cout"] - 1, 7, c["k"] // 2, c["k"] // 2] = value
        bad = (x, w, scale, shift, r, y0)
        buf, _ = _prepared(L, c, w)
        marked = np.flatnonzero(_table(L, c, buf)).tolist()
        assert marked == ([(c["cout"] - 1) // 32] if where == "w" else []), (where, value, marked)
        for tile in SPLIT_TILES:
            want, flag0, rc0 = _launch(L, c, bad, L.FLAG_SPLIT_BF16, tile)
            got, flag, rc = _launch(L, c, bad, L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY, tile, ready=buf)
            assert rc0 == 0 and rc == 0 and flag == flag0, (where, value, tile, flag, flag0)
            assert not torch.isfinite(s3._view(c, want)).all()
            assert _same_with_nans(got, want), (where, value, tile)


@pytest.mark.gpu
def test_the_ready_flag_is_refused_without_the_split_flag_and_where_the_split_flag_is(L):
    """SPLIT_WEIGHTS_READY alone; with SPLIT_BF16 on a Winograd launch, a 16-bit descriptor and the stem: YOLO_ERR_UNSUPPORTED and an
    untouched output. yolo_split3_weight_bytes is 0, and yolo_split3_weights refuses, where the split flag is not honoured."""
    lib = L.lib()
    both = L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY
    small = s3._case(1, 8, 8, 32, 64, 1, 1)
    ops = s3._operands(small, 2)
    buf, wp = _prepared(L, small, ops[1])
    y, _, rc = _launch(L, small, ops, L.FLAG_SPLIT_WEIGHTS_READY, 0, ready=wp)
    assert rc == -2 and b"SPLIT_WEIGHTS_READY" in lib.yolo_last_error() and torch.equal(y, ops[5])
    y, _, rc = _launch(L, small, ops, both, 0, ready=buf)
    assert rc == 0
    h16 = tuple(t.bfloat16() if i in (0, 5) else t for i, t in enumerate(ops))
    for flags in (both, L.FLAG_SPLIT_WEIGHTS_READY):
        y, _, rc = _launch(L, small, h16, flags, 0, ready=buf, dtype=L.BF16)
        assert rc == -2 and torch.equal(y, h16[5])
    wino = s3._case(1, 52, 52, 128, 256, 3, 1)
    wops = s3._operands(wino, 1)
    for tile in (0, 15):                             # (refused before the weights are looked at: any buffer will do)
        y, _, rc = _launch(L, wino, wops, both, tile, ready=buf, ws=True)
        assert rc == -2 and torch.equal(y, wops[5])
    stem = s3._case(1, 8, 8, 3, 32, 3, 1, x_pad=1)
    sops = s3._operands(stem, 3)
    y, _, rc = _launch(L, stem, sops, both, 0, ready=buf)
    assert rc == -2 and torch.equal(y, sops[5])
    for cin, k, s, dtype in ((3, 3, 1, L.F32), (48, 1, 1, L.F32), (32, 1, 1, L.BF16)):
        d = L.ConvDesc(n=1, h=8, w=8, cin=cin, cout=32, ksize=k, stride=s, x_ld=(cin + 3) // 4 * 4, y_ld=32, dtype=dtype)
        assert lib.yolo_split3_weight_bytes(d) == 0
        assert lib.yolo_split3_weights(d, wp.data_ptr(), buf.data_ptr(), L.current_stream()) == -2


@pytest.mark.gpu
def test_eval_model_reads_prepared_weights_and_remakes_them(L):
    """The small eval model: split3 = True (prepared weights) and "inflight" predict the same bits; True flags its split launches
    READY (their w_packed stays the block's packed buffer, prepared in place), "inflight" none, False neither flag and prepares nothing. After an in-place change of a flagged layer's weight
    the prediction equals that of a model built fresh with the changed weight: the prepared buffer was made again."""
    import yolo_for_turbines_amd as yt
    from oracle import net as onet
    x = onet.synth_input(22, 3, 96).cuda()

    def flags_of(m):
        return [p.table[i].d.flags for p in m._engine._plans.values() for i in range(len(p.table))]

    with torch.no_grad():
        ready = s3._small_model(yt, True)
        got = [o.clone() for o in ready(x)]
        inflight = s3._small_model(yt, "inflight")
        want = [o.clone() for o in inflight(x)]
        fr, fi = flags_of(ready), flags_of(inflight)
        assert [f & L.FLAG_SPLIT_BF16 for f in fr] == [f & L.FLAG_SPLIT_BF16 for f in fi] and any(f & L.FLAG_SPLIT_BF16 for f in fr)
        assert all(bool(f & L.FLAG_SPLIT_WEIGHTS_READY) == bool(f & L.FLAG_SPLIT_BF16) for f in fr)
        assert not any(f & L.FLAG_SPLIT_WEIGHTS_READY for f in fi)
        assert all(torch.equal(g, w_) for g, w_ in zip(got, want))

        (plan,) = ready._engine._plans.values()
        i = next(i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_SPLIT_WEIGHTS_READY)
        pk = ready._engine.packed(plan.blocks[i], x.device)
        assert plan.table[i].w_packed == pk.w.data_ptr() == pk.prepared["s3"].buf.data_ptr() and pk.prepared["s3"].stamp == pk.stamp
        name = next(n for n, mod in ready.named_modules() if mod is plan.blocks[i])
        plan.blocks[i].conv.weight.mul_(1.25)
        changed = [o.clone() for o in ready(x)]
        fresh = s3._small_model(yt, True)
        dict(fresh.named_modules())[name].conv.weight.mul_(1.25)
        want2 = [o.clone() for o in fresh(x)]
        assert all(torch.equal(g, w_) for g, w_ in zip(changed, want2))
        assert any(not torch.equal(g, w_) for g, w_ in zip(changed, got))

        off = s3._small_model(yt, False)
        off(x)
        assert not any(f & (L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY) for f in flags_of(off))
        assert all("s3" not in pk.prepared for per_dev in off._engine._packed.values() for pk in per_dev.values())
