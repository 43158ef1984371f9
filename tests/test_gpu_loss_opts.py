"""GPU tests (``-m gpu``) of the loss options of ``FusedYOLOLoss`` (`csrc/loss_iou.hip`: GIoU / DIoU / CIoU box terms, BCE
objectness, the focal no-object term, label smoothing, free weights). The reference everywhere is `tests/loss_ref.py`, the
formulae in fp64 on the CPU under torch autograd. Bars, those of ``test_fused_loss_values_and_gradients_vs_oracle``:
the four parts at rtol = 2e-5, atol = 1e-7, and max|dgrad| / max|grad| < 2e-5 over every element of dL/dpred. (torch's own
fp32 autograd of the same formulae on these inputs is within 1.4e-7 / 3.2e-7 of fp64: the bars leave about 60 x.)"""
import math

import numpy as np
import pytest
import torch

from oracle import net as onet
from tests import golden_inputs as gi
from tests import loss_ref

pytestmark = pytest.mark.gpu
ANCHORS = gi.TRAIN_CASE["anchors"]
W = [1.0, 0.7, 1.3, 0.9]                                     # weights of the four parts in the scalar that is differentiated
RTOL, ATOL, GRAD_BAR = 2e-5, 1e-7, 2e-5
BOX_KINDS, OBJ_KINDS = ("mse", "giou", "diou", "ciou"), ("mse", "bce")
FULL = dict(box_loss="ciou", obj_loss="bce", focal_gamma=1.5, label_smoothing=0.1)
SMALL_ANCHORS = torch.tensor([[1.0, 2.0], [2.5, 1.5], [4.0, 3.0]])


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return pkg


def _ref(p_cpu, t, anc, **kw):
    """(parts, dL/dpred) of the fp64 reference at the values of ``p_cpu``; L = sum_k W[k] parts[k]."""
    p = p_cpu.detach().double().requires_grad_(True)
    parts = torch.stack(loss_ref.yolo_loss_opts(p, t.clone(), anc, **kw))
    (parts * torch.tensor(W, dtype=torch.float64)).sum().backward()
    return parts.detach(), p.grad


def _gpu(yt, p_cpu, t, anc, view=None, **kw):
    """The same from the kernels; ``view`` maps the leaf to what the loss is given (a strided view, another dtype)."""
    leaf = p_cpu.detach().cuda().requires_grad_(True)
    t_gpu = t.clone().cuda()
    t_before, p_before = t_gpu.clone(), leaf.detach().clone()
    parts = torch.stack(yt.FusedYOLOLoss(**kw)(leaf if view is None else view(leaf), t_gpu, anc.cuda()))
    (parts * torch.tensor(W, device="cuda")).sum().backward()
    assert torch.equal(t_gpu, t_before) and torch.equal(leaf.detach(), p_before)       # no side effects
    return parts.detach().cpu(), leaf.grad.cpu()


def _assert_close(got, want, where):
    (gp, gg), (wp, wg) = got, want
    print(where, "parts", gp.tolist(), "ref", wp.tolist())
    err = float((gg.double() - wg).abs().max() / wg.abs().max())
    print(where, "grad rel err %.3e (max|grad| %.3e)" % (err, float(wg.abs().max())))
    np.testing.assert_allclose(gp.numpy(), wp.numpy(), rtol=RTOL, atol=ATOL, err_msg=str(where))
    assert gg.shape == wg.shape and err < GRAD_BAR, f"{where}: grad rel err {err}"
    return err


def _scaled_anchors(S):
    return torch.tensor(ANCHORS) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)


def _rand_case(B, gh, gw, nc, seed, n_obj):
    """Predictions and targets on a small grid: n_obj object cells with continuous random boxes (no tie of a min / max pair
    but by a measure-zero accident), two ignored cells, no-object cells everywhere else."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = torch.from_numpy(rng.standard_normal((B, 3, gh, gw, 5 + nc), dtype=np.float32))
    t = torch.zeros((B, 3, gh, gw, 6))
    flat = t.view(-1, 6)
    cells = rng.permutation(flat.shape[0])[:n_obj + 2]
    for c in cells[:n_obj]:
        flat[c] = torch.tensor([rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95), rng.uniform(0.3, 3.0), rng.uniform(0.3, 3.0), 1.0,
                                float(rng.integers(nc))])
    flat[cells[n_obj:], 4] = -1.0
    return p, t


# ---- 1. random inputs, as in test_fused_loss_values_and_gradients_vs_oracle ------------------------------------------------------

@pytest.mark.parametrize("gamma,eps", [(0.0, 0.0), (1.5, 0.1)])
@pytest.mark.parametrize("obj_loss", OBJ_KINDS)
@pytest.mark.parametrize("box_loss", BOX_KINDS)
@pytest.mark.parametrize("nc,S,B", [(2, 96, 4), (80, 64, 2)])
def test_values_and_gradients_vs_fp64_reference(yt, nc, S, B, box_loss, obj_loss, gamma, eps):
    tg = [torch.from_numpy(t) for t in gi.synth_targets(B, S, nc, ANCHORS, 77)]
    sa = _scaled_anchors(S)
    rng = np.random.Generator(np.random.PCG64(5))
    kw = dict(box_loss=box_loss, obj_loss=obj_loss, focal_gamma=gamma, label_smoothing=eps)
    for i, g in enumerate([S // 32, S // 16, S // 8]):
        p = torch.from_numpy(rng.standard_normal((B, 3, g, g, 5 + nc), dtype=np.float32))
        assert int((tg[i][..., 4] == 1).sum()) > 0
        _assert_close(_gpu(yt, p, tg[i], sa[i], **kw), _ref(p, tg[i], sa[i], **kw), (kw, "scale", i))


# ---- 2. crafted geometry -----------------------------------------------------------------------------------------------------------

#            where (anchor, y, x)   target (cx, cy, w, h)      decoded prediction (cx, cy, w, h)
CRAFTED = {
    "disjoint":           ((0, 0, 0), (0.2, 0.2, 0.2, 0.2), (0.8, 0.7, 0.15, 0.25)),
    "prediction inside":  ((1, 0, 1), (0.5, 0.5, 3.0, 2.0), (0.4, 0.6, 1.0, 0.7)),
    "target inside":      ((2, 0, 2), (0.45, 0.55, 0.8, 0.6), (0.5, 0.4, 2.5, 3.0)),
    "corner ++":          ((0, 1, 3), (0.5, 0.5, 1.0, 1.0), (0.8, 0.75, 1.2, 0.9)),
    "corner -+":          ((1, 2, 0), (0.5, 0.5, 1.0, 1.0), (0.2, 0.75, 1.2, 0.9)),
    "corner +-":          ((2, 2, 1), (0.5, 0.5, 1.0, 1.0), (0.8, 0.25, 1.2, 0.9)),
    "corner --":          ((0, 3, 2), (0.5, 0.5, 1.0, 1.0), (0.2, 0.25, 1.2, 0.9)),
}
IGNORED = (1, 3, 3)


def _crafted_case():
    nc = 3
    rng = np.random.Generator(np.random.PCG64(21))
    p = torch.from_numpy(rng.standard_normal((1, 3, 4, 4, 5 + nc), dtype=np.float32))
    t = torch.zeros((1, 3, 4, 4, 6))
    for k, ((a, y, x), g, b) in enumerate(CRAFTED.values()):
        aw, ah = SMALL_ANCHORS[a].tolist()
        t[0, a, y, x] = torch.tensor([*g, 1.0, float(k % nc)])
        p[0, a, y, x, :4] = torch.tensor([math.log(b[0] / (1 - b[0])), math.log(b[1] / (1 - b[1])), math.log(b[2] / aw), math.log(b[3] / ah)])
    t[0][IGNORED][4] = -1.0
    return p, t


def test_crafted_case_has_no_tie_within_1e3():
    """What the fp32 logits decode to, in fp64: every min / max pair of corners, and every clamp at 0, is decided by more than 1e-3."""
    p, t = _crafted_case()
    assert float(t[0][IGNORED][4]) == -1.0 and int((t[..., 4] == 1).sum()) == len(CRAFTED) and int((t[..., 4] == 0).sum()) == 48 - 8
    for name, ((a, y, x), _, _) in CRAFTED.items():
        q, g = p[0, a, y, x].double(), t[0, a, y, x].double()
        anc = SMALL_ANCHORS[a].double()
        b = torch.cat([torch.sigmoid(q[:2]), torch.exp(q[2:4]) * anc])
        for ax in (0, 1):
            b1, g1 = b[ax] - b[2 + ax] / 2, g[ax] - g[2 + ax] / 2
            b2, g2 = b1 + b[2 + ax], g1 + g[2 + ax]
            assert min(abs(b1 - g1), abs(b2 - g2), abs(min(b2, g2) - max(b1, g1))) > 1e-3, (name, ax)
    iou = loss_ref.box_geometry(torch.tensor([CRAFTED["disjoint"][2]]), torch.tensor([CRAFTED["disjoint"][1]]))[0]
    assert float(iou) == 0.0


@pytest.mark.parametrize("obj_loss", OBJ_KINDS)
@pytest.mark.parametrize("box_loss", ("giou", "diou", "ciou"))
def test_crafted_geometry_row_by_row(yt, box_loss, obj_loss):
    p, t = _crafted_case()
    kw = dict(box_loss=box_loss, obj_loss=obj_loss, focal_gamma=1.5, label_smoothing=0.1)
    got, want = _gpu(yt, p, t, SMALL_ANCHORS, **kw), _ref(p, t, SMALL_ANCHORS, **kw)
    _assert_close(got, want, kw)
    for name, ((a, y, x), _, _) in CRAFTED.items():
        gr, wr = got[1][0, a, y, x].double(), want[1][0, a, y, x]
        for cols, what in ((slice(0, 4), "box"), (slice(0, None), "row")):
            err = float((gr[cols] - wr[cols]).abs().max() / wr[cols].abs().max())
            print(name, what, "rel err %.3e" % err)
            assert err < GRAD_BAR, (name, what, err)
    a, y, x = CRAFTED["disjoint"][0]
    assert float(got[1][0, a, y, x, :4].abs().min()) > 0.0          # no overlap: the gradient still pulls all four coordinates
    assert not got[1][0][IGNORED].any() and not want[1][0][IGNORED].any()


# ---- 3. identical boxes: every min / max pair at its tie ----------------------------------------------------------------------------

@pytest.mark.parametrize("box_loss", ("giou", "diou", "ciou"))
def test_identical_boxes(yt, box_loss):
    p, t = _rand_case(1, 4, 4, 3, 31, 0)
    t[..., 4] = 0.0
    for a, (y, x), g in ((0, (1, 2), (0.5, 0.5, 1.0, 2.0)), (1, (3, 0), (0.4, 0.6, 1.5, 2.0)), (2, (0, 3), (0.25, 0.75, 0.5, 6.0))):
        aw, ah = SMALL_ANCHORS[a].tolist()
        t[0, a, y, x] = torch.tensor([*g, 1.0, 1.0])
        p[0, a, y, x, :4] = torch.tensor([math.log(g[0] / (1 - g[0])), math.log(g[1] / (1 - g[1])), math.log(g[2] / aw), math.log(g[3] / ah)])
    parts, grad = _gpu(yt, p, t, SMALL_ANCHORS, box_loss=box_loss, obj_loss="bce", focal_gamma=1.5, label_smoothing=0.1)
    want = _ref(p, t, SMALL_ANCHORS, box_loss=box_loss, obj_loss="bce", focal_gamma=1.5, label_smoothing=0.1)[0]
    print(box_loss, parts.tolist(), want.tolist())
    assert abs(float(parts[0])) < 1e-5 and abs(float(want[0])) < 1e-5
    np.testing.assert_allclose(parts[1:].numpy(), want[1:].numpy(), rtol=RTOL, atol=ATOL)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(parts).all())


# ---- 4. no object cell ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box_loss,obj_loss", [("ciou", "bce"), ("giou", "mse"), ("mse", "bce")])
def test_empty_object_set(yt, box_loss, obj_loss):
    p, t = _rand_case(2, 7, 7, 3, 9, 0)
    kw = dict(box_loss=box_loss, obj_loss=obj_loss, focal_gamma=1.5, label_smoothing=0.1)
    got, want = _gpu(yt, p, t, SMALL_ANCHORS, **kw), _ref(p, t, SMALL_ANCHORS, **kw)
    _assert_close(got, want, kw)
    assert got[0][[0, 1, 3]].tolist() == [0.0, 0.0, 0.0] and float(got[0][2]) > 0.0
    assert not got[1][..., :4].any() and not got[1][..., 5:].any() and int((got[1][..., 4] != 0).sum()) == 2 * 3 * 49 - 2


# ---- 5. layout ------------------------------------------------------------------------------------------------------------------------

def test_reference_permuted_view(yt):
    nc, g, B = 3, 7, 2
    p, t = _rand_case(B, g, g, nc, 41, 9)
    raw = p.permute(0, 1, 4, 2, 3).contiguous()                  # (B,3,5+nc,g,g), as the reference's heads leave it
    got = _gpu(yt, raw, t, SMALL_ANCHORS, view=lambda leaf: leaf.permute(0, 1, 3, 4, 2), **FULL)
    want = _ref(p, t, SMALL_ANCHORS, **FULL)
    _assert_close((got[0], got[1].permute(0, 1, 3, 4, 2)), want, "permuted view")


@pytest.mark.parametrize("box_loss", ("giou", "diou", "ciou"))
def test_rectangular_grid(yt, box_loss):
    p, t = _rand_case(2, 3, 5, 3, 43, 6)
    kw = dict(FULL, box_loss=box_loss)
    _assert_close(_gpu(yt, p, t, SMALL_ANCHORS, **kw), _ref(p, t, SMALL_ANCHORS, **kw), ("3x5", box_loss))


def test_one_class_with_label_smoothing(yt):
    p, t = _rand_case(2, 4, 4, 1, 45, 7)
    got, want = _gpu(yt, p, t, SMALL_ANCHORS, **FULL), _ref(p, t, SMALL_ANCHORS, **FULL)
    _assert_close(got, want, "nc = 1")
    assert float(got[0][3]) == 0.0                                # log softmax of one logit is 0, whatever the smoothing


# ---- 6. / 10. launch geometry and determinism ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_case():
    """B = 9 at 104 x 104: 292,032 cells, above the 1,024 x 256 = 262,144 of the block cap (a second trip through the
    grid-stride loop for some threads only) and no multiple of 256."""
    B, g, nc = 9, 104, 2
    assert B * 3 * g * g == 292032 > 1024 * 256 and 292032 % 256 != 0
    t = torch.from_numpy(gi.synth_targets(B, 832, nc, ANCHORS, 61)[2])
    p = torch.from_numpy(np.random.Generator(np.random.PCG64(62)).standard_normal((B, 3, g, g, 5 + nc), dtype=np.float32))
    sa = _scaled_anchors(832)[2]
    return p, t, sa, _ref(p, t, sa, **FULL)


def test_launch_geometry_above_the_block_cap(yt, big_case):
    p, t, sa, want = big_case
    assert int((t[..., 4] == 1).sum()) > 9 and int((t.view(-1, 6)[262144:, 4] == 1).sum()) > 0      # objects in the second trip too
    _assert_close(_gpu(yt, p, t, sa, **FULL), want, "292,032 cells")


def test_two_runs_give_the_same_bits(yt, big_case):
    p, t, sa, _ = big_case
    a, b = _gpu(yt, p, t, sa, **FULL), _gpu(yt, p, t, sa, **FULL)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 7. the defaults -------------------------------------------------------------------------------------------------------------------

def test_defaults_are_the_same_bits(yt):
    from oracle import loss as oloss
    p, t = _rand_case(2, 7, 7, 3, 47, 9)
    a = _gpu(yt, p, t, SMALL_ANCHORS)
    b = _gpu(yt, p, t, SMALL_ANCHORS, box_loss="mse", obj_loss="mse", focal_gamma=0.0, label_smoothing=0.0, lambdas=(5, 1, 0.5, 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ref = torch.stack(oloss.yolo_loss(p.double(), t.double(), SMALL_ANCHORS.double()))
    np.testing.assert_allclose(a[0].numpy(), ref.numpy(), rtol=RTOL, atol=ATOL)


# ---- 8. weights ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(FULL), dict(box_loss="giou"), dict()])
def test_custom_lambdas(yt, kw):
    """``dict()``: the reference's terms through the option kernels (only the weights differ from the defaults)."""
    p, t = _rand_case(2, 7, 7, 3, 49, 9)
    lambdas = (2.0, 0.3, 1.7, 0.6)
    got, want = _gpu(yt, p, t, SMALL_ANCHORS, lambdas=lambdas, **kw), _ref(p, t, SMALL_ANCHORS, lambdas=lambdas, **kw)
    _assert_close(got, want, (kw, lambdas))
    unit = _ref(p, t, SMALL_ANCHORS, lambdas=(1, 1, 1, 1), **kw)[0]
    np.testing.assert_allclose(got[0].numpy(), (unit * torch.tensor(lambdas, dtype=torch.float64)).numpy(), rtol=RTOL, atol=ATOL)


# ---- 9. bf16 predictions ---------------------------------------------------------------------------------------------------------------

def _loss_node(fn):
    """The backward node of the fused loss below ``fn``: its hook sees the fp32 dL/dpred before autograd rounds it to bf16."""
    seen, todo = set(), [fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if "FusedLoss" in type(n).__name__:
            return n
        todo += [f for f, _ in n.next_functions]
    raise AssertionError("no fused loss node in the graph")


@pytest.mark.parametrize("box_loss", ("giou", "diou", "ciou"))
def test_bf16_predictions(yt, box_loss):
    """Autocast heads: the terms are evaluated in fp32 at the bf16 values, so the reference is evaluated at those values."""
    p, t = _rand_case(2, 7, 7, 3, 51, 9)
    kw = dict(FULL, box_loss=box_loss)
    leaf = p.cuda().bfloat16().requires_grad_(True)
    parts = torch.stack(yt.FusedYOLOLoss(**kw)(leaf, t.cuda(), SMALL_ANCHORS.cuda()))
    assert parts.dtype == torch.float32
    grads = []
    _loss_node(parts.grad_fn).register_hook(lambda gin, gout: grads.append(gin[0].detach().clone()))
    (parts * torch.tensor(W, device="cuda")).sum().backward()
    assert len(grads) == 1 and grads[0].dtype == torch.float32 and leaf.grad.dtype == torch.bfloat16
    want = _ref(leaf.detach().cpu().float(), t, SMALL_ANCHORS, **kw)
    _assert_close((parts.detach().cpu(), grads[0].cpu()), want, ("bf16", box_loss))
    assert torch.equal(leaf.grad, grads[0].bfloat16())


# ---- 11. the whole step ----------------------------------------------------------------------------------------------------------------

def _train_case():
    c = gi.TRAIN_CASE
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    x = onet.synth_input(c["xseed"], c["batch"], c["size"]).cuda()
    tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(c["batch"], c["size"], c["nc"], c["anchors"], c["tseed"])]
    sa = _scaled_anchors(c["size"]).cuda()
    return c, sd, x, tg, sa


def _net(yt, c, sd):
    m = yt.YOLOv3(num_classes=c["nc"], activation=c["act"])
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.cuda().train()


@pytest.mark.parametrize("ac", [None, torch.bfloat16])
def test_graph_replays_equal_eager_steps(yt, ac):
    """Three warm-up steps and three replays of the captured step against six eager steps from the same start: every
    parameter and BatchNorm buffer bit-equal after each replay, as tests/test_gpu_state.py demands of the default loss."""
    c, sd, x, tg, sa = _train_case()
    lf = yt.FusedYOLOLoss("ciou", "bce", 1.5, 0.1)
    cfg = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4)

    def eager(m, opt, loss_fn):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=ac or torch.bfloat16, enabled=ac is not None):
            po = m(x)
            loss = sum(sum(loss_fn(po[i], tg[i], sa[i])) for i in range(3))
        loss.backward()
        opt.step()

    m1, m2, m3 = (_net(yt, c, sd) for _ in range(3))
    o1, o2, o3 = (yt.SGD(m.parameters(), **cfg) for m in (m1, m2, m3))
    step = yt.GraphedTrainStep(m2, o2, sa, x, tg, autocast_dtype=ac, loss_fn=lf, warmup=3)
    for _ in range(3):
        eager(m1, o1, lf)
    for k in range(3):
        eager(m1, o1, lf)
        step(x, tg)
        for (key, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
            assert torch.equal(a, b), (k, key)
    assert all(bool(torch.isfinite(v).all()) for v in m2.state_dict().values())
    for _ in range(6):                                               # the same six steps with the default loss end elsewhere
        eager(m3, o3, yt.FusedYOLOLoss())
    differ = [k for (k, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()) if not torch.equal(a, b)]
    assert len(differ) > 222 // 2, len(differ)                       # of 222 parameter tensors


def test_step_gradients_vs_the_torch_composition(yt):
    """One fp32 step's parameter gradients with the kernels against the same model under the PyTorch composition of the
    terms (`tests/loss_ref.py` on the GPU in fp32, boolean masks and all). Both backpropagate through the same network
    kernels, so they differ by what enters them: dL/dpred, where the two are each within the bar of fp64. The bar is that of
    the module, taken as it is defined there - over the whole gradient, here all 222 parameter tensors as one vector; the
    worst single tensor is printed."""
    c, sd, x, tg, sa = _train_case()
    grads = []
    for loss_fn in (yt.FusedYOLOLoss(**FULL), lambda p, t, a: loss_ref.yolo_loss_opts(p, t, a, **FULL)):
        m = _net(yt, c, sd)
        po = m(x)
        sum(sum(loss_fn(po[i], tg[i], sa[i])) for i in range(3)).backward()
        grads.append({k: p.grad.detach().double() for k, p in m.named_parameters()})
    got, want = grads
    assert len(want) == len(got) == 222
    top = max(float(v.abs().max()) for v in want.values())
    worst = max(float((got[k] - want[k]).abs().max()) for k in want)
    per_tensor = max((float((got[k] - want[k]).abs().max() / want[k].abs().max()), k) for k in want if float(want[k].abs().max()) > 0)
    print("max|dgrad| %.3e, max|grad| %.3e, ratio %.3e; worst single tensor %.3e (%s)" % (worst, top, worst / top, *per_tensor))
    assert top > 0 and worst / top < GRAD_BAR
