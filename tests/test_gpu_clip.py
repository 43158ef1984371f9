"""GPU tests (``-m gpu``) of gradient clipping by global norm (`yolo_for_turbines_amd/optim.py`, the `clip_*` kernels and
`sgd_step_kernel<EMA, CLIP>` of `csrc/optim.hip`): the norm against fp64 through the C ABI, the coefficient against CPU PyTorch bit
for bit, the fused step (plain, loss-scaled, with the weight average; skipped steps included) against a twin that does
``unscale_`` + ``clip_grads_with_norm_`` + ``torch.optim.SGD.step`` + `tests/ema_ref.py` on plain PyTorch, the free function, and
the network eagerly and as one captured graph."""
import math

import numpy as np
import pytest
import torch

from tests import clip_ref, ema_ref
from tests.test_gpu_ema import SHAPES, Bag, _case, _net, _set_grads

pytestmark = pytest.mark.gpu
INF = math.inf
# test_sgd_step_same_bits_as_torch
CFGS = [dict(lr=1e-4, momentum=0.9, weight_decay=5e-4), dict(lr=0.01), dict(lr=0.05, momentum=0.8, dampening=0.1),
        dict(lr=0.02, momentum=0.9, weight_decay=1e-3, nesterov=True), dict(lr=0.03, momentum=0.5, maximize=True), dict(lr=0.01, weight_decay=0.1)]


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return pkg


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _torch_coef(total, max_norm):
    """What CPU PyTorch makes of the device norm: the expression of `clip_grads_with_norm_`."""
    return torch.clamp(max_norm / (torch.tensor(float(total), dtype=torch.float32) + 1e-6), max=1.0).numpy()


# ---- 1 + 2. the norm against fp64 and the coefficient against CPU PyTorch, through the C ABI --------------------------------------

# two parameter groups: the shapes of the EMA tests, a view 4 bytes into its allocation and an item without a gradient; then chunk
# edges (3, 4095, 4096, 8197) and a tensor of 4096 * 1025 + 1 elements, which alone gives more partials than the finalize block
# has threads
GROUPS = [[int(np.prod(s)) for s in SHAPES] + [1030, 77], [3, 4095, 4096, 8197, 4096 * 1025 + 1]]
VIEW, NO_GRAD = (0, len(SHAPES)), (0, len(SHAPES) + 1)


class _Tables:
    """Device tables over GROUPS for one fill of the gradients; `grads[g][i]` is a CUDA tensor or None."""

    def __init__(self, lib, fill):
        ce = lib.yolo_sgd_chunk_elems()
        self.grads, self.rows, self.chunks = [], [], []
        for gi, sizes in enumerate(GROUPS):
            gs = []
            for i, n in enumerate(sizes):
                if (gi, i) == NO_GRAD:
                    gs.append(None)
                    continue
                host = fill(gi, i, n)
                if (gi, i) == VIEW:
                    base = torch.zeros(n + 1)
                    base[1:] = host
                    g = base.cuda()[1:]
                    assert g.data_ptr() % 16 == 4
                else:
                    g = host.cuda()
                gs.append(g)
            self.grads.append(gs)
            self.rows.append(torch.tensor([[0, 0 if g is None else g.data_ptr(), 0, n] for g, n in zip(gs, sizes)], dtype=torch.int64).cuda())
            self.chunks.append(torch.tensor([(i, s) for i, n in enumerate(sizes) for s in range(0, n, ce)], dtype=torch.int32).reshape(-1, 2).cuda())
        self.total = sum(c.shape[0] for c in self.chunks)
        assert self.chunks[0].shape[0] > len(GROUPS[0]) and self.chunks[1].shape[0] > 1025 > 256      # more partials than finalize threads

    def host(self):
        return [g.cpu().numpy() for gs in self.grads for g in gs if g is not None]

    def norm(self, L, lib, kind, scale=None, max_norm=1.0, found_inf=None):
        """partials per group + one finalize -> (the state's four words as float32, the partials)."""
        ws = torch.full((self.total,), float("nan"), dtype=torch.float64, device="cuda")      # every slot must be written
        state = torch.tensor([max_norm, -1.0, -1.0, -1.0], dtype=torch.float32).cuda()
        st, off = L.current_stream(), 0
        for k, (rows, chunks) in enumerate(zip(self.rows, self.chunks)):
            L.check(lib.yolo_clip_norm_partials(rows.data_ptr(), chunks.data_ptr(), chunks.shape[0], L.ptr(scale), kind,
                                                ws.data_ptr() + 8 * off, L.ptr(found_inf), int(k == 0), st))
            off += chunks.shape[0]
        L.check(lib.yolo_clip_finalize(ws.data_ptr(), self.total, kind, state.data_ptr(), st))
        return state.cpu().numpy(), ws


def _randn(gi, i, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(1000 * gi + i))


def _one_big(gi, i, n):
    g = _randn(gi, i, n) * 1e-3
    if (gi, i) == (1, 4):
        g[4096 * 700 + 5] = 3e19                      # its square overflows fp32; the norm does not
    return g


FILLS = {"randn": _randn, "one_3e19": _one_big, "all_1e-30": lambda gi, i, n: torch.full((n,), 1e-30),
         "zeros": lambda gi, i, n: torch.zeros(n)}


@pytest.fixture(scope="module")
def tables(yt):
    from yolo_for_turbines_amd import _lib as L
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Tables(L.lib(), FILLS[name])
        return cache[name]
    return get


@pytest.mark.parametrize("scale", [None, 1536.0])
@pytest.mark.parametrize("fill", list(FILLS))
def test_norm_against_fp64_and_coefficient_against_cpu_torch(yt, tables, fill, scale):
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    t = tables(fill)
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32).cuda()
    state, ws = t.norm(L, lib, 0, sc, max_norm=1.0)
    again, ws2 = t.norm(L, lib, 0, sc, max_norm=1.0)
    assert np.array_equal(_bits(state), _bits(again)) and torch.equal(ws.view(torch.int64), ws2.view(torch.int64)), "two runs, equal bits"
    assert not bool(torch.isnan(ws).any()) and _bits(state)[3] == 0 and state[0] == 1.0
    want = clip_ref.total_norm(t.host(), scale)
    got = float(state[1])
    print(f"{fill} scale={scale}: norm {got!r} want {want!r} rel err {abs(got - want) / want if want else 0.0:.3e} coef {float(state[2])!r}")
    assert abs(got - want) <= clip_ref.BOUND * want
    if fill == "zeros":
        assert got == 0.0 and state[2] == 1.0
    if fill == "one_3e19":
        assert got > 1e19 / (scale or 1.0)          # the planted element is the norm; its fp32 square is inf
    if fill == "all_1e-30":
        assert 0 < got < 1e-25
    # the coefficient for this norm, at a maximum that bites, one that does not, and an odd one: only the finalize runs again
    for max_norm in (1.0, 1e4, 0.37, INF):
        st = torch.tensor([max_norm, 0, 0, 0], dtype=torch.float32).cuda()
        L.check(lib.yolo_clip_finalize(ws.data_ptr(), t.total, 0, st.data_ptr(), L.current_stream()))
        st = st.cpu().numpy()
        assert _bits(st[1]) == _bits(state[1])
        assert _bits(st[2]) == _bits(_torch_coef(st[1], max_norm)) == _bits(clip_ref.coef(st[1], max_norm)), (fill, max_norm)


@pytest.mark.parametrize("scale", [None, 1536.0])
def test_inf_norm_is_the_largest_magnitude_bit_for_bit(yt, tables, scale):
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32).cuda()
    for fill in ("randn", "one_3e19", "zeros"):
        t = tables(fill)
        state, ws = t.norm(L, lib, 1, sc, max_norm=0.5)
        again, _ = t.norm(L, lib, 1, sc, max_norm=0.5)
        want = clip_ref.total_norm(t.host(), scale, INF)
        assert _bits(state[1]) == _bits(want) == _bits(again[1]) and _bits(state)[3] == 1, fill
        assert _bits(state[2]) == _bits(_torch_coef(state[1], 0.5)), fill
    # a NaN anywhere is the answer, whatever else is there (torch.max propagates it)
    t = tables("randn")
    g = t.grads[1][3]
    keep = g[8196].clone()
    g[8196] = float("nan")
    try:
        state, _ = t.norm(L, lib, 1, sc)
        assert np.isnan(state[1]) and np.isnan(state[2])
    finally:
        g[8196] = keep


def test_check_fused_into_the_norm_pass(yt, tables):
    """With a flag the same launch does the non-finite check: raised by an inf or a NaN in any group, cleared otherwise, and the
    partial sums are the bits of the launch without it."""
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    t = tables("randn")
    sc = torch.tensor(1536.0).cuda()
    flag = torch.ones((), device="cuda")
    plain, ws0 = t.norm(L, lib, 0, sc)
    state, ws = t.norm(L, lib, 0, sc, found_inf=flag)
    assert float(flag) == 0.0 and np.array_equal(_bits(plain), _bits(state)) and torch.equal(ws0.view(torch.int64), ws.view(torch.int64))
    for (gi, i, at), bad in (((1, 4, 4096 * 1025), float("inf")), ((0, VIEW[1], 1029), float("nan")), ((0, 3, 17), float("-inf"))):
        g = t.grads[gi][i].view(-1)
        keep = g[at].clone()
        g[at] = bad
        try:
            flag.zero_()
            state, _ = t.norm(L, lib, 0, sc, found_inf=flag)
            assert float(flag) == 1.0 and not np.isfinite(state[1]), (gi, i)
        finally:
            g[at] = keep


@pytest.mark.parametrize("max_norm", [1.0, 0.37, 1e4])
def test_coefficient_at_and_one_ulp_around_max_norm(yt, max_norm):
    """A single gradient element v has the norm |v| exactly: plant it at max_norm and one ulp to either side."""
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    at = np.float32(max_norm)
    for v in (at, np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(INF))):
        g = torch.tensor([-float(v)], dtype=torch.float32).cuda()
        rows = torch.tensor([[0, g.data_ptr(), 0, 1]], dtype=torch.int64).cuda()
        chunks = torch.zeros((1, 2), dtype=torch.int32).cuda()
        ws = torch.zeros(1, dtype=torch.float64).cuda()
        st = torch.tensor([max_norm, 0, 0, 0], dtype=torch.float32).cuda()
        L.check(lib.yolo_clip_norm_partials(rows.data_ptr(), chunks.data_ptr(), 1, 0, 0, ws.data_ptr(), 0, 0, L.current_stream()))
        L.check(lib.yolo_clip_finalize(ws.data_ptr(), 1, 0, st.data_ptr(), L.current_stream()))
        st = st.cpu().numpy()
        assert _bits(st[1]) == _bits(v)
        assert _bits(st[2]) == _bits(_torch_coef(st[1], max_norm)), (max_norm, v)


# ---- 3. the fused step ------------------------------------------------------------------------------------------------------------

def _same_or_both_nan(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _assert_same_state(a, oa, b, ob, where, eq=torch.equal):
    for i, (p, q) in enumerate(zip(a.ps, b.ps)):
        assert eq(p, q), (where, i)
        ba, bb = oa.state[p].get("momentum_buffer"), ob.state[q].get("momentum_buffer")
        assert (ba is None) == (bb is None) and (ba is None or eq(ba, bb)), (where, i)


@pytest.mark.parametrize("max_norm", [1.0, 1e4])
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("cfg", CFGS)
def test_fused_step_same_bits_as_unscale_clip_step_on_torch(yt, cfg, scaled, with_ema, max_norm):
    a, b = Bag(), Bag()
    oa, ob = yt.SGD(a.parameters(), max_grad_norm=max_norm, **cfg), torch.optim.SGD(b.parameters(), **cfg)
    sa, sb = (yt.GradScaler(init_scale=1024.0), torch.amp.GradScaler(init_scale=1024.0)) if scaled else (None, None)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa) if with_ema else None
    ref = ema_ref.EmaRef(b.state_dict(), decay=0.5, warmup=True) if with_ema else None
    norm_at = oa.grad_norm.data_ptr()
    for step in range(3):
        factor = sa.scale(torch.ones((), device="cuda")) if scaled else None
        assert not scaled or float(sb.scale(torch.ones((), device="cuda"))) == float(factor)
        _set_grads((a, b), step, scale=factor)
        for m in (a, b):
            m.touch_buffers(step)
        put = [None if p.grad is None else p.grad.clone() for p in a.ps]
        if scaled:
            sa.step(oa)
            sa.update()
            sb.unscale_(ob)
        else:
            oa.step()
        assert oa.grad_norm.data_ptr() == norm_at and oa.grad_norm.dim() == 0 and oa.grad_norm.dtype == torch.float32
        torch.nn.utils.clip_grads_with_norm_(list(b.parameters()), max_norm, oa.grad_norm)
        if scaled:
            sb.step(ob)
            sb.update()
            assert sa.get_scale() == sb.get_scale()
        else:
            ob.step()
        _assert_same_state(a, oa, b, ob, step)
        if with_ema:
            ref.update(b.state_dict())
            got = ema.module.state_dict()
            for k, v in got.items():
                assert torch.equal(v, ref.shadow[k]), (step, k)
        # the norm the step used is the norm of the gradients the twin holds after its unscale, before its clip ... which the
        # twin has scaled by coef since; so against the reference on what was put into .grad
        want = clip_ref.total_norm([g.cpu().numpy() for g in put if g is not None], float(factor) if scaled else None)
        assert abs(float(oa.grad_norm) - want) <= clip_ref.BOUND * want
        coef = float(oa.clip_coef)
        assert _bits(coef) == _bits(_torch_coef(float(oa.grad_norm), max_norm))
        assert coef < 1.0 if max_norm == 1.0 else coef == 1.0
        # the native step unscales and clips in registers: .grad holds what was put there (the SCALED values under a scaler)
        for p, g in zip(a.ps, put):
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
    if with_ema:
        assert ema.updates == 3


def test_skipped_step_under_the_scaler_touches_nothing(yt):
    cfg = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    a = Bag()
    oa = yt.SGD(a.parameters(), max_grad_norm=1.0, **cfg)
    sa = yt.GradScaler(init_scale=1024.0)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa)
    scales = []
    for step, planted in enumerate((True, False, True)):                  # the very first step skipped: no buffer written yet
        factor = sa.scale(torch.ones((), device="cuda"))
        _set_grads((a,), step, scale=factor)
        a.touch_buffers(step)
        if planted:
            a.ps[3].grad[7, 100] = float("inf")
        before = dict(p=[p.detach().clone() for p in a.ps],
                      buf=[oa.state[p]["momentum_buffer"].clone() if "momentum_buffer" in oa.state.get(p, {}) else None for p in a.ps],
                      written=oa._tables[0].written.clone() if oa._tables else None,
                      shadow={k: v.clone() for k, v in ema.module.state_dict().items()}, updates=ema.updates)
        sa.step(oa)
        sa.update()
        scales.append(sa.get_scale())
        if not planted:
            assert ema.updates == before["updates"] + 1 and any(not torch.equal(p, q) for p, q in zip(a.ps, before["p"]))
            continue
        for i, p in enumerate(a.ps):
            assert torch.equal(p, before["p"][i]), (step, i)
            if before["buf"][i] is not None:
                assert torch.equal(oa.state[p]["momentum_buffer"], before["buf"][i]), (step, i)
        if before["written"] is not None:
            assert torch.equal(oa._tables[0].written, before["written"]), step
        else:
            assert int(oa._tables[0].written.sum()) == 0
        for k, v in ema.module.state_dict().items():
            assert torch.equal(v, before["shadow"][k]), (step, k)
        assert ema.updates == before["updates"]
    assert scales == [512.0, 512.0, 256.0]


def test_planted_inf_without_a_scaler_gives_what_torch_gives(yt):
    cfg = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    a, b = Bag(), Bag()
    oa, ob = yt.SGD(a.parameters(), max_grad_norm=1.0, **cfg), torch.optim.SGD(b.parameters(), **cfg)
    for step in range(2):
        _set_grads((a, b), step)
        for m in (a, b):
            m.ps[3].grad[7, 100] = float("inf")
        oa.step()
        assert float(oa.grad_norm) == INF and float(oa.clip_coef) == 0.0
        torch.nn.utils.clip_grads_with_norm_(list(b.parameters()), 1.0, oa.grad_norm)
        ob.step()
        _assert_same_state(a, oa, b, ob, step, eq=_same_or_both_nan)
        assert bool(a.ps[3].isnan().sum() == 1) and bool(a.ps[3].isnan()[7, 100])


def test_inf_norm_step_and_reassigned_attributes(yt):
    """norm_type inf through the optimizer, two parameter groups, and max_grad_norm / grad_norm_type reassigned between steps
    (a number to another number, to None and back)."""
    a, b = Bag(), Bag()
    def groups(m):
        ps = list(m.parameters())
        return [dict(params=ps[:3]), dict(params=ps[3:], lr=0.02)]
    oa = yt.SGD(groups(a), lr=0.01, momentum=0.9, max_grad_norm=0.25, grad_norm_type=INF)
    ob = torch.optim.SGD(groups(b), lr=0.01, momentum=0.9)
    plan = [(0.25, INF), (2.0, 2.0), (None, 2.0), (0.5, INF)]
    for step, (max_norm, kind) in enumerate(plan):
        oa.max_grad_norm, oa.grad_norm_type = max_norm, kind
        _set_grads((a, b), step)
        grads = [p.grad.cpu().numpy() for p in a.ps if p.grad is not None]
        oa.step()
        if max_norm is not None:
            want = clip_ref.total_norm(grads, None, kind)
            if kind == INF:
                assert _bits(float(oa.grad_norm)) == _bits(want)
            else:
                assert abs(float(oa.grad_norm) - want) <= clip_ref.BOUND * want
            assert float(oa.clip_coef) < 1.0
            torch.nn.utils.clip_grads_with_norm_(list(b.parameters()), max_norm, oa.grad_norm)
        ob.step()
        _assert_same_state(a, oa, b, ob, step)


# ---- 4. the free function ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm,kind", [(1.0, 2.0), (1e4, 2.0), (0.5, INF)])
def test_free_function_is_torchs_clip_fed_the_returned_norm(yt, max_norm, kind):
    a, b = Bag(), Bag()
    _set_grads((a, b), 2)
    for m in (a, b):                                                     # one gradient 4 bytes into its allocation: the scalar path
        base = torch.zeros(m.ps[1].numel() + 1).cuda()
        base[1:] = m.ps[1].grad
        m.ps[1].grad = base[1:]
    assert a.ps[1].grad.data_ptr() % 16 == 4
    grads = [p.grad.cpu().numpy() for p in a.ps if p.grad is not None]
    total = yt.clip_grad_norm_(a.parameters(), max_norm, norm_type=kind)
    assert total.is_cuda and total.dim() == 0 and total.dtype == torch.float32
    want = clip_ref.total_norm(grads, None, kind)
    assert abs(float(total) - want) <= clip_ref.BOUND * want
    torch.nn.utils.clip_grads_with_norm_(list(b.parameters()), max_norm, total)
    for i, (p, q) in enumerate(zip(a.ps, b.ps)):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), i
    again = yt.clip_grad_norm_(a.parameters(), max_norm, norm_type=kind, error_if_nonfinite=True)       # the cached tables
    if max_norm < want:
        assert abs(float(again) - max_norm) <= 4 * clip_ref.BOUND * max_norm and again.data_ptr() != total.data_ptr()


def test_free_function_refuses_what_it_cannot_do(yt):
    a = Bag()
    _set_grads((a,), 2)
    with pytest.raises(ValueError, match="norm_type"):
        yt.clip_grad_norm_(a.parameters(), 1.0, norm_type=3)
    h = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16).cuda())
    h.grad = torch.ones(8, dtype=torch.float16).cuda()
    with pytest.raises(TypeError, match="fp32"):
        yt.clip_grad_norm_(list(a.parameters()) + [h], 1.0)
    a.ps[3].grad[7, 100] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        yt.clip_grad_norm_(a.parameters(), 1.0, error_if_nonfinite=True)
    assert math.isnan(float(yt.clip_grad_norm_(a.parameters(), 1.0)))
    # a single tensor, as PyTorch allows
    p = torch.nn.Parameter(torch.zeros(5).cuda())
    p.grad = torch.full((5,), 2.0).cuda()
    assert float(yt.clip_grad_norm_(p, 1.0)) == float(np.float32(math.sqrt(20.0)))
    assert torch.equal(p.grad, torch.full((5,), 2.0).cuda() * torch.tensor(_torch_coef(np.float32(math.sqrt(20.0)), 1.0)).cuda())


# ---- 5. the network, eager and as one graph ---------------------------------------------------------------------------------------

def test_network_one_graph_clips_like_eager_steps(yt):
    sd, x, tg, sa = _case(311)
    lf = yt.FusedYOLOLoss()
    warm, replays = 3, 3

    def setup(max_norm):
        net = _net(yt, sd)
        opt = yt.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
        return net, opt, yt.GradScaler(init_scale=256.0), yt.ModelEMA(net, decay=0.9998, warmup=True)

    def eager(net, opt, scaler):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            preds = net(x)
            loss = sum(sum(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3))
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    # a dry run for the first step's norm: clipping at half of it bites
    dry, od, sdry, _ = setup(INF)
    eager(dry, od, sdry)
    first = float(od.grad_norm)
    assert math.isfinite(first) and first > 0 and float(od.clip_coef) == 1.0
    max_norm = 0.5 * first
    del dry, od, sdry
    m, om, sm, ema = setup(max_norm)
    twin, ot, st, ema_t = setup(max_norm)
    ema_t.attach(ot)

    def same(where):
        a, b = m.state_dict(), twin.state_dict()
        for k in a:
            assert torch.equal(a[k], b[k]), (where, k)
        a, b = ema.module.state_dict(), ema_t.module.state_dict()
        for k in a:
            assert torch.equal(a[k], b[k]), (where, "shadow", k)
        for pa, pb in zip(m.parameters(), twin.parameters()):
            assert torch.equal(om.state[pa]["momentum_buffer"], ot.state[pb]["momentum_buffer"]), where
        assert _bits(float(om.grad_norm)) == _bits(float(ot.grad_norm)) and _bits(float(om.clip_coef)) == _bits(float(ot.clip_coef)), where
        assert sm.get_scale() == st.get_scale() and ema.updates == ema_t.updates, where
    step = yt.GraphedTrainStep(m, om, sa, x, tg, autocast_dtype=torch.float16, grad_scaler=sm, warmup=warm, ema=ema)
    for k in range(warm):
        eager(twin, ot, st)
        if k == 0:
            assert float(ot.grad_norm) > max_norm and float(ot.clip_coef) < 1.0, "clipping bites"
    same("after the warm-up steps")
    for k in range(replays):
        step(x, tg)
        eager(twin, ot, st)
        same(k)
        print(f"replay {k}: grad_norm {float(om.grad_norm)!r} max {max_norm!r} coef {float(om.clip_coef)!r}")
    assert ema.updates > 0
    om.max_grad_norm = ot.max_grad_norm = 1e9                            # a changed number reaches the captured finalize
    step(x, tg)
    eager(twin, ot, st)
    same("after max_grad_norm = 1e9")
    assert float(om.clip_coef) == 1.0
    om.max_grad_norm = ot.max_grad_norm = 1.0                            # ... and back to one that bites inside a replay
    step(x, tg)
    eager(twin, ot, st)
    same("after max_grad_norm = 1")
    assert float(om.clip_coef) < 1.0
    om.max_grad_norm = None
    with pytest.raises(RuntimeError, match="clipping"):
        step(x, tg)
