"""GPU tests (``-m gpu``) of `yt.Adam` / `yt.AdamW` (`yolo_for_turbines_amd/optim.py`, `csrc/optim_adam.hip`): the per-step words
of `yolo_adam_prepare` against the Python-double expressions of `tests/adam_ref.py`, the step against `torch.optim.Adam` /
`AdamW` (foreach) on the same GPU - plain, loss-scaled with skipped steps, clipped, with the weight average - the network as one
captured graph under an LR schedule, the checkpoint in both directions, and the refusals. Everything is compared bit for bit."""
import copy

import numpy as np
import pytest
import torch

from tests import adam_ref, clip_ref, ema_ref
from tests.test_gpu_ema import SHAPES, Bag, _case, _net, _set_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return pkg


def _count(state):
    """Steps a parameter has taken: 0 without state (PyTorch) and for state a skipped step allocated (here)."""
    return int(state["step"]) if "step" in state else 0


def _assert_same_state(a, oa, b, ob, where):
    for i, (p, q) in enumerate(zip(a.ps, b.ps)):
        assert torch.equal(p, q), (where, i, "p")
        sa, sb = oa.state.get(p, {}), ob.state.get(q, {})
        assert _count(sa) == _count(sb), (where, i, "step")
        if _count(sb):
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]), (where, i, "exp_avg")
            assert torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (where, i, "exp_avg_sq")
        elif "exp_avg" in sa:                                             # allocated by a skipped step: still zeros
            assert not bool(sa["exp_avg"].any()) and not bool(sa["exp_avg_sq"].any()), (where, i)


# ---- 1. the per-step words ----------------------------------------------------------------------------------------------------------

TS = (1, 2, 3, 10, 100, 1000, 2000, 20000)


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("lr", [1e-3, 3e-4])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.937, 0.999), (0.4, 0.9)])
def test_prepare_words_same_bits_as_python_doubles(yt, betas, lr, wd):
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    n = len(TS) + 1                                                       # one item per t, and one without a gradient
    g = torch.zeros(4, device="cuda")                                     # never read: the kernel only asks whether there is one
    table = torch.zeros(5 * n, dtype=torch.int64)
    table[:4 * n].view(n, 4)[:len(TS), 1] = g.data_ptr()
    table = table.cuda()
    hyper = torch.tensor([lr, betas[0], betas[1], 1e-8, wd], dtype=torch.float64).cuda()
    start = torch.tensor([t - 1 for t in TS] + [7], dtype=torch.int32).cuda()
    steps = start.clone()
    words = torch.full((n, 8), -1.0, device="cuda")
    flag = torch.ones((), device="cuda")
    L.check(lib.yolo_adam_prepare(table.data_ptr(), n, hyper.data_ptr(), steps.data_ptr(), words.data_ptr(), flag.data_ptr(), L.current_stream()))
    assert torch.equal(steps, start) and bool((words == -1.0).all()), "found_inf set: nothing moved"
    flag.zero_()
    L.check(lib.yolo_adam_prepare(table.data_ptr(), n, hyper.data_ptr(), steps.data_ptr(), words.data_ptr(), flag.data_ptr(), L.current_stream()))
    assert steps.tolist() == list(TS) + [7]
    got = words.cpu().numpy()
    assert (got[-1] == -1.0).all(), "an item without a gradient: nothing moved"
    for k, t in enumerate(TS):
        want = adam_ref.words(t, lr, betas, 1e-8, wd)
        print(f"t={t} betas={betas} lr={lr} wd={wd}: got {got[k, :7].tolist()} want {want.tolist()}")
        assert np.array_equal(got[k, :7].view(np.int32), want.view(np.int32)), (t, got[k, :7].tolist(), want.tolist())
        assert got[k, 7] == np.float32(wd)
    # without a flag (NULL): a plain step
    L.check(lib.yolo_adam_prepare(table.data_ptr(), n, hyper.data_ptr(), steps.data_ptr(), words.data_ptr(), 0, L.current_stream()))
    assert steps.tolist() == [t + 1 for t in TS] + [7]


# ---- 2. the step against PyTorch ----------------------------------------------------------------------------------------------------

CFGS = [("Adam", dict(lr=1e-3)), ("Adam", dict(lr=1e-3, weight_decay=5e-4)), ("AdamW", dict(lr=1e-3, weight_decay=0.05)),
        ("AdamW", dict(lr=2e-3, weight_decay=0.05, maximize=True)), ("Adam", dict(lr=1e-3, betas=(0.4, 0.9))),
        ("AdamW", dict(lr=1e-3, eps=1e-3))]
FILLS = {"randn": None, "zeros": 0.0, "1e-20": 1e-20}                      # (1e-20)^2 is an fp32 denormal


def _fill_grads(models, step, fill):
    _set_grads(models, step)
    if FILLS[fill] is not None:
        for m in models:
            for p in m.ps:
                if p.grad is not None:
                    p.grad = torch.full_like(p.grad, FILLS[fill])


@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("name,cfg", CFGS)
def test_step_same_bits_as_torch(yt, name, cfg, fill):
    a, b = Bag(), Bag()
    oa, ob = getattr(yt, name)(a.parameters(), **cfg), getattr(torch.optim, name)(b.parameters(), foreach=True, **cfg)
    assert len(a.ps) == len(SHAPES) + 1 and a.ps[-1].data_ptr() % 16 != 0, "the view takes the scalar path"
    for step in range(6):
        _fill_grads((a, b), step, fill)
        oa.step()
        ob.step()
        _assert_same_state(a, oa, b, ob, step)
        for o in (oa, ob):                                                # as LinearLR would
            o.param_groups[0]["lr"] = cfg["lr"] * (1.0 - 0.1 * (step + 1))
    counts = [_count(oa.state.get(p, {})) for p in a.ps]
    assert counts[2] == 0 and counts[4] == 4 and counts[0] == 6, "per-parameter step counts"
    assert oa.state[a.ps[0]]["step"].is_cuda and oa.state_dict()["state"][0]["step"].device.type == "cpu"
    if fill == "1e-20" and (name == "AdamW" or not cfg.get("weight_decay")):      # (coupled decay adds wd * p to the gradient)
        v = oa.state[a.ps[0]]["exp_avg_sq"]
        assert bool((v > 0).all()) and bool((v < 1.2e-38).all()), "denormal second moments are kept, as PyTorch keeps them"


# ---- 3. loss-scaled, skipped steps included -------------------------------------------------------------------------------------------

def test_loss_scaled_steps_and_skips_same_bits_as_torch(yt):
    cfg = dict(lr=1e-3, weight_decay=0.05)
    a, b = Bag(), Bag()
    oa, ob = yt.AdamW(a.parameters(), **cfg), torch.optim.AdamW(b.parameters(), foreach=True, **cfg)
    sa, sb = yt.GradScaler(init_scale=1024.0), torch.amp.GradScaler(init_scale=1024.0)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa)
    ref = ema_ref.EmaRef(b.state_dict(), decay=0.5, warmup=True)
    inf_steps = (0, 4)
    for step in range(8):
        fa, fb = sa.scale(torch.ones((), device="cuda")), sb.scale(torch.ones((), device="cuda"))
        assert float(fa) == float(fb)
        _set_grads((a, b), step, scale=fa)
        if step in inf_steps:
            for m in (a, b):
                m.ps[3].grad = m.ps[3].grad.clone()
                m.ps[3].grad[7, 100] = float("inf")
        for m in (a, b):
            m.touch_buffers(step)
        before = dict(p=[p.detach().clone() for p in a.ps], shadow={k: v.clone() for k, v in ema.module.state_dict().items()},
                      m=[oa.state[p]["exp_avg"].clone() if "exp_avg" in oa.state.get(p, {}) else None for p in a.ps],
                      v=[oa.state[p]["exp_avg_sq"].clone() if "exp_avg" in oa.state.get(p, {}) else None for p in a.ps],
                      t=[_count(oa.state.get(p, {})) for p in a.ps], updates=ema.updates)
        sa.step(oa)
        sa.update()
        sb.step(ob)
        sb.update()
        assert sa.get_scale() == sb.get_scale()
        if step in inf_steps:                                            # a skipped step touches nothing
            for i, p in enumerate(a.ps):
                assert torch.equal(p, before["p"][i]) and _count(oa.state.get(p, {})) == before["t"][i], (step, i)
                if before["m"][i] is not None:
                    assert torch.equal(oa.state[p]["exp_avg"], before["m"][i]) and torch.equal(oa.state[p]["exp_avg_sq"], before["v"][i]), (step, i)
            for k, v in ema.module.state_dict().items():
                assert torch.equal(v, before["shadow"][k]), (step, k)
            assert ema.updates == before["updates"]
        else:
            ref.update(b.state_dict())
        if step == 0:
            assert oa.state_dict()["state"] == {} == ob.state_dict()["state"], "never stepped: no entry, like PyTorch"
        _assert_same_state(a, oa, b, ob, step)
        for k, v in ema.module.state_dict().items():
            assert torch.equal(v, ref.shadow[k]), (step, k)
    assert ema.updates == 6 == ref.updates
    assert sorted(oa.state_dict()["state"]) == sorted(ob.state_dict()["state"])


# ---- 4. clipped, with and without the average -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [1.0, 1e4])
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_clipped_step_same_bits_as_unscale_clip_step_on_torch(yt, scaled, with_ema, max_norm):
    cfg = dict(lr=1e-3, weight_decay=0.05)
    a, b = Bag(), Bag()
    oa, ob = yt.AdamW(a.parameters(), max_grad_norm=max_norm, **cfg), torch.optim.AdamW(b.parameters(), foreach=True, **cfg)
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
        assert oa.grad_norm.data_ptr() == norm_at
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
            for k, v in ema.module.state_dict().items():
                assert torch.equal(v, ref.shadow[k]), (step, k)
        want = clip_ref.total_norm([g.cpu().numpy() for g in put if g is not None], float(factor) if scaled else None)
        assert abs(float(oa.grad_norm) - want) <= clip_ref.BOUND * want
        coef = float(oa.clip_coef)
        assert coef < 1.0 if max_norm == 1.0 else coef == 1.0
        for p, g in zip(a.ps, put):                                      # the gradient is never written
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
    if with_ema:
        assert ema.updates == 3


# ---- 5. the network as one graph ------------------------------------------------------------------------------------------------------

def _same(a, b):
    """Equal bits, a NaN counting as equal to a NaN (BatchNorm's running statistics after a batch that holds an inf)."""
    return torch.equal(a, b) or (a.dtype.is_floating_point and bool(((a == b) | (a.isnan() & b.isnan())).all()))


def _assert_same_network(m, om, twin, ot, where, ema=None, ema_t=None):
    a, b = m.state_dict(), twin.state_dict()
    for k in a:
        assert _same(a[k], b[k]), (where, k)
    for pa, pb in zip(m.parameters(), twin.parameters()):
        sa, sb = om.state[pa], ot.state[pb]
        assert int(sa["step"]) == int(sb["step"]), where
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), where
    if ema is not None:
        a, b = ema.module.state_dict(), ema_t.module.state_dict()
        for k in a:
            assert _same(a[k], b[k]), (where, "shadow", k)
        assert ema.updates == ema_t.updates, where


def test_network_one_graph_with_scaler_average_clip_and_schedule(yt):
    sd, x, tg, sa = _case(311)
    lf = yt.FusedYOLOLoss()
    warm, replays = 3, 3

    def setup():
        net = _net(yt, sd)
        opt = yt.AdamW(net.parameters(), lr=1e-3, weight_decay=0.05, max_grad_norm=10.0)
        sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, total_iters=10)
        return net, opt, sched, yt.GradScaler(init_scale=256.0), yt.ModelEMA(net, decay=0.9998, warmup=True)
    m, om, lm, sm, ema = setup()
    twin, ot, lt, st, ema_t = setup()
    ema_t.attach(ot)

    def eager(xb):
        ot.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            preds = twin(xb)
            loss = sum(sum(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3))
        st.scale(loss).backward()
        st.step(ot)
        st.update()
    step = yt.GraphedTrainStep(m, om, sa, x, tg, autocast_dtype=torch.float16, grad_scaler=sm, warmup=warm, ema=ema)
    assert ema._attached is om
    for _ in range(warm):
        eager(x)
    _assert_same_network(m, om, twin, ot, "after the warm-up steps", ema, ema_t)
    lrs = []
    for k in range(replays):
        step(x, tg)
        eager(x)
        _assert_same_network(m, om, twin, ot, k, ema, ema_t)
        assert sm.get_scale() == st.get_scale()
        lrs.append(om.param_groups[0]["lr"])
        lm.step()
        lt.step()
    assert len(set(lrs)) == replays, "the learning rate moved between the replays"
    assert float(om.grad_norm) == float(ot.grad_norm) and ema.updates > 0
    # an inf planted in the input: the replay skips, like the eager step, and the scale is halved
    bad = x.clone()
    bad[0, 0, 0, 0] = float("inf")
    before = {k: v.clone() for k, v in m.state_dict().items() if v.dtype == torch.float32 and "running" not in k}
    counts = [int(om.state[p]["step"]) for p in m.parameters()]
    scale = sm.get_scale()
    step(bad, tg)
    twin._engine.nan_check = False                                       # the eager forward's guard would raise on this batch
    eager(bad)
    twin._engine.nan_check = True
    assert sm.get_scale() == 0.5 * scale == st.get_scale()
    now = m.state_dict()
    assert all(torch.equal(now[k], v) for k, v in before.items()) and counts == [int(om.state[p]["step"]) for p in m.parameters()]
    _assert_same_network(m, om, twin, ot, "after the skipped replay", ema, ema_t)
    step(x, tg)
    eager(x)
    _assert_same_network(m, om, twin, ot, "after the replay that follows the skip", ema, ema_t)
    assert all(bool(p.isfinite().all()) for p in m.parameters()) and any(not torch.equal(before[k], v) for k, v in m.state_dict().items() if k in before)


def test_network_one_graph_follows_a_changed_lr_without_a_scaler(yt):
    sd, x, tg, sa = _case(311)
    lf = yt.FusedYOLOLoss()
    m, twin = _net(yt, sd), _net(yt, sd)
    om, ot = (yt.AdamW(n.parameters(), lr=1e-3, weight_decay=0.05) for n in (m, twin))

    def eager():
        ot.zero_grad(set_to_none=True)
        preds = twin(x)
        sum(sum(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3)).backward()
        ot.step()
    step = yt.GraphedTrainStep(m, om, sa, x, tg, warmup=2)
    for _ in range(2):
        eager()
    for k, lr in enumerate((1e-3, 4e-4, 2e-3)):
        om.param_groups[0]["lr"] = ot.param_groups[0]["lr"] = lr
        step(x, tg)                                                      # followed, not refused
        eager()
        _assert_same_network(m, om, twin, ot, (k, lr))


# ---- 6. checkpoint ----------------------------------------------------------------------------------------------------------------------

def test_checkpoint_round_trips_with_torch_adamw_and_itself(yt, tmp_path):
    cfg = dict(lr=1e-3, weight_decay=0.05)
    a = Bag()
    oa = yt.AdamW(a.parameters(), **cfg)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa)
    for step in range(3):
        _set_grads((a,), step)
        a.touch_buffers(step)
        oa.step()
    path = str(tmp_path / "ck.pth.tar")
    yt.save_checkpoint(a, oa, filename=path, ema=ema)
    ck = torch.load(path)
    assert sorted(ck["optimizer"]["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    t0 = ck["optimizer"]["state"][0]["step"]
    assert t0.dtype == torch.float32 and t0.device.type == "cpu" and float(t0) == 3.0 and float(ck["optimizer"]["state"][4]["step"]) == 1.0
    assert 2 not in ck["optimizer"]["state"]
    # into plain PyTorch
    b = Bag()
    b.load_state_dict(ck["state_dict"])
    ob = torch.optim.AdamW(b.parameters(), foreach=True, lr=0.5)
    ob.load_state_dict(ck["optimizer"])
    # into a fresh native optimizer, through load_checkpoint
    c = Bag()
    oc = yt.AdamW(c.parameters(), lr=0.5, weight_decay=0.3)
    ema_c = yt.ModelEMA(c, decay=0.9, warmup=False).attach(oc)
    yt.load_checkpoint(c, oc, lr=cfg["lr"], filename=path, ema=ema_c)
    assert ob.param_groups[0]["lr"] == cfg["lr"] == oc.param_groups[0]["lr"] and oc.param_groups[0]["weight_decay"] == 0.05
    for step in (3, 4):
        _set_grads((a, b, c), step)
        for mod in (a, b, c):
            mod.touch_buffers(step)
        for o in (oa, ob, oc):
            o.step()
        _assert_same_state(a, oa, b, ob, ("torch", step))
        _assert_same_state(a, oa, c, oc, ("native", step))
        for k, v in ema.module.state_dict().items():
            assert torch.equal(v, ema_c.module.state_dict()[k]), (step, k)
    assert ema_c.updates == ema.updates == 5
    # and back: what torch.optim.AdamW saves loads into the native optimizer
    d = Bag()
    d.load_state_dict(b.state_dict())
    od = yt.AdamW(d.parameters(), lr=0.5)
    od.load_state_dict(copy.deepcopy(ob.state_dict()))
    for step in (5, 6):
        _set_grads((b, d), step)
        ob.step()
        od.step()
        _assert_same_state(d, od, b, ob, ("from torch", step))
    assert [_count(od.state.get(p, {})) for p in d.ps][:5] == [7, 7, 0, 7, 5]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(yt):
    h = torch.nn.Parameter(torch.zeros(8, dtype=torch.float16).cuda())
    h.grad = torch.ones(8, dtype=torch.float16).cuda()
    with pytest.raises(TypeError, match="fp32"):
        yt.AdamW([h]).step()
    p = torch.nn.Parameter(torch.zeros(6, 4).cuda())
    opt = yt.Adam([p], lr=1e-3)
    p.grad = torch.ones(4, 6).cuda().t()
    with pytest.raises(TypeError, match="contiguous"):
        opt.step()
    p.grad = torch.ones(6, 4).cuda().to_sparse()
    with pytest.raises(TypeError, match="dense"):
        opt.step()
    assert not bool(p.any()) and opt.state_dict()["state"] == {}
    for bad in (dict(lr=torch.tensor(1e-3)), dict(betas=(torch.tensor(0.9), torch.tensor(0.999)))):
        q = torch.nn.Parameter(torch.zeros(4).cuda())
        q.grad = torch.ones(4).cuda()
        with pytest.raises(TypeError, match="tensors"):
            yt.AdamW([q], **bad).step()
    # a capture before any eager step would have to allocate the tables and the moments
    q = torch.nn.Parameter(torch.zeros(4).cuda())
    q.grad = torch.ones(4).cuda()
    fresh = yt.AdamW([q], lr=1e-3)
    with pytest.raises(RuntimeError, match="take one eager step before capturing"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            q.grad * 1.0                                                 # (so that the abandoned capture is not an empty graph)
            fresh.step()
    fresh.step()                                                         # and eagerly it works
    assert int(fresh.state[q]["step"]) == 1 and bool((q < 0).all())
    a = Bag()
    with pytest.raises(TypeError, match="yolo_for_turbines_amd.SGD"):
        yt.ModelEMA(a).attach(torch.optim.Adam(a.parameters()))
    x = torch.zeros(1, 3, 32, 32).cuda()
    with pytest.raises(TypeError, match="yolo_for_turbines_amd.SGD"):
        yt.GraphedTrainStep(None, torch.optim.AdamW(a.parameters()), None, x, None, grad_scaler=yt.GradScaler())
