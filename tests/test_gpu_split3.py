"""YOLO_FLAG_SPLIT_BF16: the fp32 direct convolutions as three-way bf16 split products (conv_split3_f32) — accuracy against an
fp64 convolution next to the exact-f32 kernel (tile 4), special values, determinism, batch independence and routing."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

SPLIT_TILES = (0, 1, 2, 4)        # heuristic, 128x128, 128x64, 64x64


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def _case(n, h, w, cin, cout, k, s, act=1, res=False, out=0, x_pad=0, x_off=0, y_pad=0, y_off=0, r_pad=0, r_off=0):
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, act=act, res=res, out=out, x_pad=x_pad, x_off=x_off, y_pad=y_pad,
                y_off=y_off, r_pad=r_pad, r_off=r_off)


# every case has at least 8192 output values; out: 0 NHWC, 1 2x upsampling store, 2 head layout
CASES = {
    "1x1_k32_25px": _case(1, 5, 5, 32, 384, 1, 1),                                           # one K step, 25 ragged pixels
    "1x1_k96_straddle": _case(3, 13, 13, 96, 24, 1, 1, act=0),                                # M tiles straddle images; ragged N tile
    "1x1_k256_res_views": _case(3, 13, 13, 256, 96, 1, 1, act=2, res=True, x_pad=32, x_off=16, y_pad=40, y_off=8, r_pad=16, r_off=4),
    "1x1_head": _case(2, 13, 13, 256, 255, 1, 1, act=0, out=2),                               # nc5 = 85
    "1x1_upsample": _case(2, 13, 13, 256, 128, 1, 1, out=1, y_pad=256, y_off=128),            # the route layer's writer
    "3x3s2_7x9": _case(5, 7, 9, 32, 96, 3, 2),
    "3x3s2_13x13": _case(3, 13, 13, 64, 64, 3, 2, act=2),
    "3x3s2_16x16": _case(6, 16, 16, 32, 24, 3, 2, x_pad=8, x_off=4),
    "3x3s1_20x20": _case(1, 20, 20, 32, 64, 3, 1, res=True),
    "3x3s1_one_row": _case(1, 1, 40, 32, 256, 3, 1),                                          # kh = 0 and 2 are padding everywhere
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
    ops = _operands(c, 4100 + sum(ord(ch) for ch in name))
    return c, ops, _reference(c, ops)


def _launch(L, c, ops, flags, tile, dtype=None, ws=False):
    """One yolo_conv_fwd of case c: (output buffer on the host, NaN flag, return code)."""
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x, w, scale, shift, r, y0 = ops
    code = L.F32 if dtype is None else dtype
    wp = torch.empty(lib.yolo_packed_weight_bytes(c["cout"], c["cin"], c["k"], code), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.to(dev).contiguous().data_ptr(), wp.data_ptr(), c["cout"], c["cin"], c["k"], code, st), "pack")
    xd, sc, sh, yd = x.to(dev), scale.to(dev), shift.to(dev), y0.to(dev)
    rd = r.to(dev) if r is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.ConvDesc(n=c["n"], h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ksize=c["k"], stride=c["s"], x_ld=x.shape[-1],
                   x_off=c["x_off"], y_ld=c["cout"] + c["y_pad"], y_off=c["y_off"], r_ld=r.shape[-1] if r is not None else 0,
                   r_off=c["r_off"], act=c["act"], out_mode=c["out"], dtype=code,
                   flags=(L.FLAG_RESIDUAL if r is not None else 0) | L.FLAG_NANCHECK | flags, tile=tile)
    if ws:
        need = lib.yolo_conv_workspace_bytes(d)
        wsb = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        rc = lib.yolo_conv_fwd_ws(d, xd.data_ptr(), wp.data_ptr(), sc.data_ptr(), sh.data_ptr(), L.ptr(rd), yd.data_ptr(), wsb.data_ptr(),
                                  need, flag.data_ptr(), st)
    else:
        rc = lib.yolo_conv_fwd(d, xd.data_ptr(), wp.data_ptr(), sc.data_ptr(), sh.data_ptr(), L.ptr(rd), yd.data_ptr(), flag.data_ptr(), st)
    torch.cuda.synchronize()
    return yd.cpu(), int(flag.item()), rc


def _rel_err(c, y, ref):
    return float((_view(c, y).double() - ref).abs().max() / ref.abs().max())


def _outside_untouched(c, y, y0):
    if c["out"] == 2:
        return True
    a, b = y.clone(), y0.clone()
    a[..., c["y_off"]:c["y_off"] + c["cout"]] = 0
    b[..., c["y_off"]:c["y_off"] + c["cout"]] = 0
    return torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_split_products_are_as_accurate_as_the_f32_kernel(L, name):
    """max|err| / max|y| against fp64 of the flagged kernel, every tile size, is at most twice the exact-f32 kernel's (tile 4,
    no flag) on the same operands: the three dropped terms are at most one more fp32 rounding per product. The rest of the
    output buffer stays as it was, a second run gives the same bits, the 2x upsampling store writes four equal pixels."""
    c, ops, ref = _shared(name)
    exact, flag0, rc = _launch(L, c, ops, 0, 4)
    assert rc == 0 and flag0 == 0
    e_exact = _rel_err(c, exact, ref)
    assert e_exact < 3e-6
    for tile in SPLIT_TILES:
        y, flag, rc = _launch(L, c, ops, L.FLAG_SPLIT_BF16, tile)
        assert rc == 0, L.lib().yolo_last_error()
        e = _rel_err(c, y, ref)
        print(f"{name} tile {tile}: split {e:.3e}  exact {e_exact:.3e}  ratio {e / e_exact:.2f}")
        assert flag == 0
        assert e <= 2 * e_exact, (tile, e, e_exact)
        assert _outside_untouched(c, y, ops[5])
        if c["out"] == 1:
            v = y[..., c["y_off"]:c["y_off"] + c["cout"]]
            assert torch.equal(v[:, ::2, ::2], v[:, 1::2, ::2]) and torch.equal(v[:, ::2, ::2], v[:, ::2, 1::2])
            assert torch.equal(v[:, ::2, ::2], v[:, 1::2, 1::2])
        again, _, _ = _launch(L, c, ops, L.FLAG_SPLIT_BF16, tile)
        assert torch.equal(again, y), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1_k96_straddle", "3x3s2_13x13"])
def test_inf_and_nan_behave_as_in_the_exact_kernel(L, name):
    """An Inf or a NaN in x or w gives Inf / NaN at the output positions of tile 4, with the same NaN-flag bit; with 64x64 blocks
    (tile 4 against tile 4) every block that holds such a value equals the exact kernel's in its finite values too, bit for bit."""
    c, ops, _ = _shared(name)
    for where, value in (("x", float("inf")), ("x", float("nan")), ("w", float("-inf")), ("w", float("nan"))):
        x, w, scale, shift, r, y0 = (t.clone() if t is not None else None for t in ops)
        if where == "x":
            x[1, c["h"] // 2, 3, c["x_off"] + 5] = value
            x[0, 0, 0, c["x_off"]] = value
        else:
            w[c["cout"] - 1, 7, c["k"] // 2, c["k"] // 2] = value
        bad = (x, w, scale, shift, r, y0)
        exact, flag0, rc0 = _launch(L, c, bad, 0, 4)
        assert rc0 == 0
        ve = _view(c, exact)
        assert not torch.isfinite(ve).all()
        for tile in SPLIT_TILES:
            y, flag, rc = _launch(L, c, bad, L.FLAG_SPLIT_BF16, tile)
            v = _view(c, y)
            assert rc == 0 and flag == flag0, (where, value, tile, flag, flag0)
            assert torch.equal(torch.isnan(v), torch.isnan(ve)), (where, value, tile)
            assert torch.equal(torch.isinf(v), torch.isinf(ve)) and torch.equal(v[torch.isinf(v)], ve[torch.isinf(ve)]), (where, value, tile)
            if tile == 4:
                # a 64x64 block that staged the value computes its tile again in the exact kernel's order: the same bits
                a, b = v.reshape(-1, c["cout"]), ve.reshape(-1, c["cout"])
                hit = 0
                for m0 in range(0, a.shape[0], 64):
                    for n0 in range(0, c["cout"], 64):
                        ta, tb = a[m0:m0 + 64, n0:n0 + 64], b[m0:m0 + 64, n0:n0 + 64]
                        if not torch.isfinite(tb).all():
                            hit += 1
                            assert torch.equal(torch.nan_to_num(ta), torch.nan_to_num(tb)), (where, value, m0, n0)
                assert hit


@pytest.mark.gpu
def test_huge_finite_operands_stay_finite(L):
    """Operands of magnitude 3.3e38 (rounding them to bf16 to nearest would overflow) with weights that keep the outputs finite."""
    c, ops, _ = _shared("3x3s2_13x13")
    x, w, scale, shift, r, y0 = (t.clone() if t is not None else None for t in ops)
    x = torch.where(x >= 0, 3.3e38, -3.3e38).float()
    w = w * 1e-6
    scale, shift = torch.ones_like(scale), torch.zeros_like(shift)
    big = (x, w, scale, shift, r, y0)
    ref = _reference(c, big)
    assert torch.isfinite(ref.float()).all()
    for tile in SPLIT_TILES:
        y, flag, rc = _launch(L, c, big, L.FLAG_SPLIT_BF16, tile)
        assert rc == 0 and flag == 0
        assert torch.isfinite(_view(c, y)).all()
        assert _rel_err(c, y, ref) < 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1_k256_res_views", "3x3s2_13x13"])
def test_an_image_does_not_depend_on_its_batch(L, name):
    """Image 1 of the batch of 3 equals the same image run alone, bit for bit."""
    c, ops, _ = _shared(name)
    x, w, scale, shift, r, y0 = ops
    one = dict(c, n=1)
    alone = (x[1:2].contiguous(), w, scale, shift, r[1:2].contiguous() if r is not None else None, y0[1:2].contiguous())
    for tile in SPLIT_TILES:
        y3, _, rc3 = _launch(L, c, ops, L.FLAG_SPLIT_BF16, tile)
        y1, _, rc1 = _launch(L, one, alone, L.FLAG_SPLIT_BF16, tile)
        assert rc3 == 0 and rc1 == 0
        assert torch.equal(y3[1:2], y1), tile


@pytest.mark.gpu
def test_the_flag_is_refused_where_the_direct_kernels_do_not_run(L):
    """A Winograd-family descriptor with its workspace, a 16-bit descriptor, the stem shape and a tile the kernel does not have."""
    lib = L.lib()
    wino = _case(1, 52, 52, 128, 256, 3, 1)
    ops = _operands(wino, 1)
    y, _, rc = _launch(L, wino, ops, L.FLAG_SPLIT_BF16, 0, ws=True)
    assert rc == -2 and b"SPLIT_BF16" in lib.yolo_last_error() and torch.equal(y, ops[5])
    y, _, rc = _launch(L, wino, ops, L.FLAG_SPLIT_BF16, 15, ws=True)
    assert rc == -2 and torch.equal(y, ops[5])
    _, _, rc = _launch(L, wino, ops, L.FLAG_SPLIT_BF16, 0)            # no workspace: the layer runs on the direct kernels
    assert rc == 0
    small = _case(1, 8, 8, 32, 64, 1, 1)
    ops = _operands(small, 2)
    h16 = tuple(t.bfloat16() if i in (0, 5) else t for i, t in enumerate(ops))
    y, _, rc = _launch(L, small, h16, L.FLAG_SPLIT_BF16, 0, dtype=L.BF16)
    assert rc == -2 and torch.equal(y, h16[5])
    stem = _case(1, 8, 8, 3, 32, 3, 1, x_pad=1)
    ops = _operands(stem, 3)
    y, _, rc = _launch(L, stem, ops, L.FLAG_SPLIT_BF16, 0)
    assert rc == -2 and torch.equal(y, ops[5])
    ops = _operands(small, 2)
    for tile in (3, 5, 7):
        y, _, rc = _launch(L, small, ops, L.FLAG_SPLIT_BF16, tile)
        assert rc == -2 and torch.equal(y, ops[5])


def test_eval_plan_flags_what_split3_eligible_accepts(built):
    """Host side (plans built on the CPU device: no launch): at batch 32, 416 x 416, 80 classes the eval plan flags exactly the
    launches from plan.first on that yolo_conv_split3_eligible accepts (with ModelState.split3 = "all": that
    yolo_conv_split3_supported accepts: the direct launches with cin % 32 == 0), none of them a Winograd launch; with
    ModelState.split3 off, with a forced tile, on a 16-bit plan and on a train plan nothing is flagged."""
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine, train_engine
    L = built
    lib = L.lib()
    m = yt.YOLOv3(num_classes=80).eval()
    dev = torch.device("cpu")
    prog = engine.build_network_program(m, 32, 416)
    st = engine.ModelState()
    for mode, accepts in ((True, lib.yolo_conv_split3_eligible), ("all", lib.yolo_conv_split3_supported)):
        st = engine.ModelState()
        st.split3 = mode
        plan = engine.Plan(prog, st, dev)
        flagged = [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_SPLIT_BF16]
        want = []
        for i in range(plan.first, len(plan.table)):
            d = L.ConvDesc.from_buffer_copy(plan.table[i].d)
            d.flags &= ~L.FLAG_SPLIT_BF16
            if accepts(C.byref(d)):
                want.append(i)
        assert flagged == want
        for i in flagged:
            d = plan.table[i].d
            assert lib.yolo_conv_workspace_bytes(C.byref(d)) == 0 and plan.table[i].workspace == 0
            assert not d.flags & L.FLAG_FILTERS_READY and lib.yolo_conv_pick_tile(C.byref(d)) not in (13, 14, 15)
            assert d.cin % 32 == 0 and d.dtype == L.F32
        ready = [i for i in range(len(plan.table)) if plan.table[i].d.flags & L.FLAG_FILTERS_READY]
        assert len(ready) == 24 and not set(ready) & set(flagged)
    # "all": the 74 launches behind the stem less the 24 + 7 Winograd ones = the 5 stride-2, the 32 -> 64 3x3 at 208 x 208, 34 1x1, 3 heads
    assert len(flagged) == len(plan.table) - plan.first - 31, len(flagged)
    st_off = engine.ModelState()
    st_off.split3 = False
    for p in (engine.Plan(prog, st_off, dev), engine.Plan(prog, st, dev, tile_override=4),
              engine.Plan(engine.build_network_program(m, 32, 416, ch_align=8), st, dev, dtype="bf16")):
        assert not any(p.table[i].d.flags & L.FLAG_SPLIT_BF16 for i in range(len(p.table)))
    # the train path builds its descriptors from the program's flags alone (train_engine._desc): the program carries no such flag
    tprog = engine.build_network_program(m, 2, 96)
    train_engine.TrainPlan(tprog, dev, "fp32")
    for op in tprog.ops:
        cv = op["block"].conv
        d = train_engine._desc(2, op["x"], cv.in_channels, cv.out_channels, op["k"], op["s"], cv.out_channels, 0, flags=op["flags"])
        assert not op["flags"] & L.FLAG_SPLIT_BF16 and not d.flags & L.FLAG_SPLIT_BF16


def _small_model(yt, split3):
    from oracle import net as onet
    m = yt.YOLOv3(num_classes=2)
    m.load_state_dict(onet.synth_state_dict(21, 3, 2, gain=0.8))
    m = m.cuda().eval()
    m._engine.split3 = split3
    return m


@pytest.mark.gpu
def test_small_eval_model_flagged_against_exact(L):
    """96 x 96, batch 3, 2 classes: the flagged forward agrees with the exact-f32 forward within the bar test_gpu_parity.py holds the
    fp32 network to against the oracle (1e-4 absolute); image 1 of the batch equals the same image run alone, bit for bit (every launch
    the library honours the flag on carries it: ModelState.split3 = "all"); with ModelState.split3 off no launch carries the flag, so the library runs what it ran before the flag existed."""
    import yolo_for_turbines_amd as yt
    from oracle import net as onet
    x = onet.synth_input(22, 3, 96).cuda()
    with torch.no_grad():
        on = _small_model(yt, "all")
        got = [o.clone() for o in on(x)]
        alone = [o.clone() for o in on(x[1:2].contiguous())]
        off = _small_model(yt, False)
        want = [o.clone() for o in off(x)]
        flags_on = [p.table[i].d.flags & L.FLAG_SPLIT_BF16 for p in on._engine._plans.values() for i in range(len(p.table))]
        flags_off = [p.table[i].d.flags & L.FLAG_SPLIT_BF16 for p in off._engine._plans.values() for i in range(len(p.table))]
        assert any(flags_on) and not any(flags_off)
    for g, w_, a in zip(got, want, alone):
        err = float((g - w_).abs().max())
        print(f"flagged vs exact: max abs diff {err:.3e} (max |y| {float(w_.abs().max()):.3e})")
        assert err <= 1e-4
        assert torch.equal(g[1:2], a)


@pytest.mark.gpu
def test_split3_off_runs_the_unflagged_launches_bit_for_bit(L):
    """ModelState.split3 = False: the forward's predictions equal, bit for bit, the plan's launches issued one by one through
    yolo_conv_fwd_ws with descriptors that carry no YOLO_FLAG_SPLIT_BF16 (what a C-ABI caller from before the flag runs); the
    flagged forward of the same weights differs from it in some bit, so the comparison can tell the two apart."""
    import yolo_for_turbines_amd as yt
    from oracle import net as onet
    lib = L.lib()
    x = onet.synth_input(22, 3, 96).cuda()
    with torch.no_grad():
        off = _small_model(yt, False)
        want = [o.clone() for o in off(x)]
        flagged = [o.clone() for o in _small_model(yt, True)(x)]
        (plan,) = off._engine._plans.values()
        st = L.current_stream()
        plan.nan_flag.zero_()
        plan.load_input(x.contiguous(), st)
        outs = {i: torch.zeros((3, 3, gh, plan.prog.ops[i]["Wo"], c3), device=x.device) for i, gh, c3 in plan.pred_ops.values()}
        for i in range(plan.first, len(plan.table)):
            e = plan.table[i]
            d = L.ConvDesc.from_buffer_copy(e.d)
            assert not d.flags & L.FLAG_SPLIT_BF16
            y = outs[i].data_ptr() if i in outs else e.y
            L.check(lib.yolo_conv_fwd_ws(d, e.x, e.w_packed, e.scale, e.shift, e.residual or None, y, e.workspace or None,
                                         e.workspace_bytes, plan.nan_flag.data_ptr(), st), "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
    got = [outs[plan.pred_ops[k][0]] for k in range(plan.prog.n_pred)]
    assert all(torch.equal(g, w_) for g, w_ in zip(got, want))
    assert any(not torch.equal(f, w_) for f, w_ in zip(flagged, want))
