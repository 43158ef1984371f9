"""GPU tests (``-m gpu``) of the weight average (`yolo_for_turbines_amd/ema.py`, the `*_ema` kernels of `csrc/optim.hip`):
the standalone launch, the launch fused into the SGD step (plain and loss-scaled, skipped steps included), the network
eagerly and as one captured graph, and the checkpoint. The reference everywhere is `tests/ema_ref.py`
(``e.mul_(d).add_(p, alpha=1 - d)`` with the coefficients formed in numpy.float32), compared bit for bit."""
import numpy as np
import pytest
import torch

from oracle import net as onet
from tests import ema_ref
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu
NC, S, B = 2, 96, 2
SHAPES = [(64, 32, 3, 3), (32,), (1,), (255, 1024, 1, 1), (4097,), (3, 5, 7), (1030,)]     # test_sgd_step_same_bits_as_torch


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return pkg


class Bag(torch.nn.Module):
    """The parameter set of test_sgd_step_same_bits_as_torch as a module: chunk tails, counts that are no multiple of four, a
    single element, a view 4 bytes into its allocation (the scalar path); plus a float and an integer buffer, which no
    optimizer owns."""

    def __init__(self):
        super().__init__()
        ps = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i)).cuda()) for i, s in enumerate(SHAPES)]
        base = torch.randn(1031, generator=torch.Generator().manual_seed(5)).cuda()
        ps.append(torch.nn.Parameter(base[1:]))
        self.ps = torch.nn.ParameterList(ps)
        self.register_buffer("stat", torch.randn(37, generator=torch.Generator().manual_seed(50)).cuda())
        self.register_buffer("count", torch.tensor(0, dtype=torch.int64).cuda())

    def touch_buffers(self, step):
        """What a train-mode forward does to BatchNorm buffers: new statistics, one more batch counted."""
        self.stat.copy_(torch.randn(37, generator=torch.Generator().manual_seed(60 + step)).cuda())
        self.count += 1


def _set_grads(models, step, scale=None):
    """The gradient pattern of that test: parameter 2 never gets one, parameter 4 from the third step on."""
    for i in range(len(SHAPES) + 1):
        for m in models:
            p = m.ps[i]
            if i == 2 or (i == 4 and step < 2):
                p.grad = None
                continue
            gr = torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * step + i)).cuda()
            p.grad = gr.clone() if scale is None else gr * scale


def _assert_shadow(ema, ref, where):
    got = ema.module.state_dict()
    assert list(got) == list(ref.shadow)
    for k, v in got.items():
        assert v.dtype == ref.shadow[k].dtype and torch.equal(v, ref.shadow[k]), (where, k)


# ---- 1. the standalone kernel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("warmup", [True, False])
def test_standalone_kernel_same_bits_as_the_reference(yt, warmup):
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    ce = lib.yolo_sgd_chunk_elems()
    decay = 0.5                                                          # the schedule crosses from quotient to constant at t = 8
    gen = torch.Generator().manual_seed(3)
    base_s, base_d = torch.randn(1031, generator=gen).cuda(), torch.randn(1031, generator=gen).cuda()
    src = {f"f{i}": torch.randn(s, generator=gen).cuda() for i, s in enumerate(SHAPES)}
    src["view"] = base_s[1:]
    src["int"] = torch.tensor((1 << 40) + 5, dtype=torch.int64).cuda()
    dst = {k: (base_d[1:] if k == "view" else torch.randn(v.shape, generator=gen).cuda().to(v.dtype)) for k, v in src.items()}
    assert src["view"].data_ptr() % 16 == 4 and dst["view"].data_ptr() % 16 == 4
    ref = ema_ref.EmaRef(dst, decay=decay, warmup=warmup)
    counts = [v.numel() if v.dtype == torch.float32 else -2 * v.numel() for v in src.values()]
    rows = torch.tensor([[s.data_ptr(), d.data_ptr(), n] for s, d, n in zip(src.values(), dst.values(), counts)], dtype=torch.int64).cuda()
    chunks = torch.tensor([(i, s) for i, n in enumerate(counts) for s in range(0, abs(n), ce)], dtype=torch.int32).reshape(-1, 2).cuda()
    assert chunks.shape[0] > len(counts)                                 # more than one block for some entry
    state = torch.tensor([0, int(np.array([decay], np.float32).view(np.int32)[0]), int(warmup), 0], dtype=torch.int32).cuda()
    for k in range(12):
        for name, v in src.items():                                      # the source moves every update
            if v.dtype == torch.float32:
                v.copy_(torch.randn(v.shape, generator=gen).cuda())
            else:
                v.fill_((1 << 40) + 7 * k)
        L.check(lib.yolo_ema_update(rows.data_ptr(), chunks.data_ptr(), chunks.shape[0], state.data_ptr(), 0, 1, L.current_stream()))
        ref.update(src)
        for name in src:
            assert torch.equal(dst[name], ref.shadow[name]), (k, name)
        assert int(state[0]) == k + 1 == ref.updates
        assert state[1:].tolist() == [int(np.array([decay], np.float32).view(np.int32)[0]), int(warmup), 0]
    # a raised flag: nothing written, nothing counted
    flag = torch.ones((), device="cuda")
    before = {k: v.clone() for k, v in dst.items()}
    L.check(lib.yolo_ema_update(rows.data_ptr(), chunks.data_ptr(), chunks.shape[0], state.data_ptr(), flag.data_ptr(), 1, L.current_stream()))
    assert all(torch.equal(dst[k], before[k]) for k in dst) and int(state[0]) == 12


# ---- 2. fused into the SGD step ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [dict(lr=1e-4, momentum=0.9, weight_decay=5e-4), dict(lr=0.01),
                                 dict(lr=0.02, momentum=0.9, weight_decay=1e-3, nesterov=True)])
def test_fused_step_same_bits_as_torch_sgd_then_the_reference(yt, cfg):
    a, b = Bag(), Bag()
    oa, ob = yt.SGD(a.parameters(), **cfg), torch.optim.SGD(b.parameters(), **cfg)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa)
    ref = ema_ref.EmaRef(b.state_dict(), decay=0.5, warmup=True)
    assert ema.module.ps[-1].data_ptr() % 16 != 0 or a.ps[-1].data_ptr() % 16 != 0    # the scalar path of the fused kernel
    _assert_shadow(ema, ref, "start")
    assert not any(p.requires_grad for p in ema.module.parameters())
    with pytest.raises(RuntimeError, match="twice"):
        ema.update()
    for step in range(4):
        _set_grads((a, b), step)
        for m in (a, b):
            m.touch_buffers(step)
        oa.step()
        ob.step()
        ref.update(b.state_dict())
        for i, (p, q) in enumerate(zip(a.ps, b.ps)):
            assert torch.equal(p, q), (step, i)
            ba, bb = oa.state[p].get("momentum_buffer"), ob.state[q].get("momentum_buffer")
            assert (ba is None) == (bb is None) and (ba is None or torch.equal(ba, bb)), (step, i)
        _assert_shadow(ema, ref, step)                                   # ps.2 (never a gradient) and the buffers included
        assert ema.updates == step + 1
    assert int(ema.module.count) == 4


def test_standalone_update_for_any_other_optimizer(yt):
    a, b = Bag(), Bag()
    oa, ob = torch.optim.SGD(a.parameters(), lr=0.01, momentum=0.9), torch.optim.SGD(b.parameters(), lr=0.01, momentum=0.9)
    ema = yt.ModelEMA(a, decay=0.5, warmup=False)
    ref = ema_ref.EmaRef(b.state_dict(), decay=0.5, warmup=False)
    with pytest.raises(TypeError, match="yolo_for_turbines_amd.SGD"):
        ema.attach(oa)
    for step in range(3):
        _set_grads((a, b), step)
        for m in (a, b):
            m.touch_buffers(step)
        oa.step()
        ob.step()
        ema.update()
        ref.update(b.state_dict())
        _assert_shadow(ema, ref, step)
    assert ema.updates == 3
    half = Bag().half()
    with pytest.raises(TypeError, match="fp32"):
        yt.ModelEMA(half)


# ---- 3. loss-scaled steps, skips included ----------------------------------------------------------------------------------------

def test_loss_scaled_steps_skip_the_average_too(yt):
    cfg = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    a, b = Bag(), Bag()
    oa, ob = yt.SGD(a.parameters(), **cfg), torch.optim.SGD(b.parameters(), **cfg)
    sa, sb = yt.GradScaler(init_scale=1024.0), torch.amp.GradScaler(init_scale=1024.0)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa)
    ref = ema_ref.EmaRef(b.state_dict(), decay=0.5, warmup=True)
    inf_steps = (0, 2)                                                   # the first step skipped: no momentum buffer written yet
    for step in range(5):
        fa, fb = sa.scale(torch.ones((), device="cuda")), sb.scale(torch.ones((), device="cuda"))
        assert float(fa) == float(fb)
        _set_grads((a, b), step, scale=fa)
        if step in inf_steps:
            for m in (a, b):
                m.ps[3].grad = m.ps[3].grad.clone()
                m.ps[3].grad[7, 100] = float("inf")
        for m in (a, b):
            m.touch_buffers(step)
        before = [q.detach().clone() for q in b.ps]
        sa.step(oa)
        sa.update()
        sb.step(ob)
        sb.update()
        applied = any(not torch.equal(q, r) for q, r in zip(b.ps, before))
        assert applied == (step not in inf_steps)
        if applied:                                                      # the reference average moves only with an applied step
            ref.update(b.state_dict())
        for i, (p, q) in enumerate(zip(a.ps, b.ps)):
            assert torch.equal(p, q), (step, i)
        _assert_shadow(ema, ref, step)
        assert sa.get_scale() == sb.get_scale()
    assert ema.updates == 3 == ref.updates


# ---- 4. the network ----------------------------------------------------------------------------------------------------------

def _case(seed):
    anchors = gi.TRAIN_CASE["anchors"]
    sd = onet.synth_state_dict(seed, 3, NC, gain=gi.NET_GAIN)
    x = onet.synth_input(seed + 1, B, S).cuda()
    tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(B, S, NC, anchors, seed + 2)]
    sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).cuda()
    return sd, x, tg, sa


def _net(yt, sd):
    m = yt.YOLOv3(num_classes=NC, activation="leaky_relu")
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.cuda().train()


def _assert_forward_current(yt, ema, fresh, x, where):
    """The averaged model's forward uses the averaged weights as they are NOW: equal to a model that packs them anew."""
    fresh.load_state_dict(ema.module.state_dict())                       # invalidates every packed weight of `fresh`
    with torch.no_grad():
        got, want = ema.module(x), fresh(x)
    assert not ema.module.training
    for g, w in zip(got, want):
        assert torch.equal(g, w), where


def test_network_eager_steps_average_every_entry(yt):
    sd, x, tg, sa = _case(311)
    lf = yt.FusedYOLOLoss()
    m, twin = _net(yt, sd), _net(yt, sd)
    om, ot = (yt.SGD(n.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4) for n in (m, twin))
    ema = yt.ModelEMA(m, decay=0.9998, warmup=True).attach(om)
    ref = ema_ref.EmaRef(twin.state_dict(), decay=0.9998, warmup=True)
    assert len(ref.shadow) == 438 and sum(v.dtype == torch.float32 for v in ref.shadow.values()) == 366
    fresh = yt.YOLOv3(num_classes=NC, activation="leaky_relu").cuda().eval()
    _assert_forward_current(yt, ema, fresh, x, "start")
    for step in range(3):
        for net, opt in ((m, om), (twin, ot)):
            opt.zero_grad(set_to_none=True)
            preds = net(x)
            sum(sum(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3)).backward()
            opt.step()
        ref.update(twin.state_dict())
        tsd = twin.state_dict()
        for k, v in m.state_dict().items():
            assert torch.equal(v, tsd[k]), (step, k)
        _assert_shadow(ema, ref, step)                                   # running statistics and num_batches_tracked included
        assert int(ema.module.state_dict()["layers.0.batch_norm.num_batches_tracked"]) == step + 1
        _assert_forward_current(yt, ema, fresh, x, step)                 # fails when the version counters are not moved
    assert ema.updates == 3


def test_network_one_graph_follows_the_device_counter(yt):
    sd, x, tg, sa = _case(311)
    lf = yt.FusedYOLOLoss()
    warm, replays = 3, 3

    def setup():
        net = _net(yt, sd)
        opt = yt.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
        return net, opt, yt.GradScaler(init_scale=256.0), yt.ModelEMA(net, decay=0.9998, warmup=True)
    m, om, sm, ema = setup()
    twin, ot, st, ema_t = setup()
    ema_t.attach(ot)

    def eager():
        ot.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            preds = twin(x)
            loss = sum(sum(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3))
        st.scale(loss).backward()
        st.step(ot)
        st.update()

    def same(where):
        a, b = ema.module.state_dict(), ema_t.module.state_dict()
        for k in a:
            assert torch.equal(a[k], b[k]), (where, k)
        assert ema.updates == ema_t.updates, where
    step = yt.GraphedTrainStep(m, om, sa, x, tg, autocast_dtype=torch.float16, grad_scaler=sm, warmup=warm, ema=ema)
    assert ema._attached is om                                           # attached by the constructor, before the warm-up steps
    for _ in range(warm):
        eager()
    same("after the warm-up steps")
    for k in range(replays):
        step(x, tg)
        eager()
        same(k)
    # all of these steps lie inside the warm-up of the decay (d = (1 + t) / (10 + t) < 0.9998): a d baked in at the capture
    # (t = 3) gives other bits from the second replay on
    assert 0 < ema.updates <= warm + replays and sm.get_scale() == st.get_scale()
    assert ema_ref.coeffs(warm + replays, 0.9998, True)[0] < float(np.float32(0.9998))
    fresh = yt.YOLOv3(num_classes=NC, activation="leaky_relu").cuda().eval()
    _assert_forward_current(yt, ema, fresh, x, "after the last replay")


# ---- 5. checkpoint -----------------------------------------------------------------------------------------------------------

def test_checkpoint_round_trip_with_the_average(yt, tmp_path):
    cfg = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    a = Bag()
    oa = yt.SGD(a.parameters(), **cfg)
    ema = yt.ModelEMA(a, decay=0.5, warmup=True).attach(oa)
    for step in range(3):
        _set_grads((a,), step)
        a.touch_buffers(step)
        oa.step()
    path = str(tmp_path / "ck.pth.tar")
    yt.save_checkpoint(a, oa, filename=path, ema=ema)
    assert set(torch.load(path).keys()) == {"state_dict", "optimizer", "ema"}
    b = Bag()
    with torch.no_grad():
        for p in b.parameters():
            p.zero_()
    ob = yt.SGD(b.parameters(), lr=0.5, momentum=0.9, weight_decay=5e-4)
    ema2 = yt.ModelEMA(b, decay=0.9, warmup=False).attach(ob)
    yt.load_checkpoint(b, ob, lr=cfg["lr"], filename=path, ema=ema2)
    assert ema2.updates == ema.updates == 3 and ema2.decay == 0.5 and ema2.warmup is True
    _set_grads((a, b), 3)
    for m in (a, b):
        m.touch_buffers(3)
    oa.step()
    ob.step()
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    for k, v in ema.module.state_dict().items():
        assert torch.equal(v, ema2.module.state_dict()[k]), k
    assert ema2.updates == ema.updates == 4
    yt.save_checkpoint(a, oa, filename=path)
    with pytest.raises(KeyError, match="ema"):
        yt.load_checkpoint(b, ob, lr=0.05, filename=path, ema=ema2)
