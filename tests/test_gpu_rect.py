"""GPU tests (``-m gpu``) of rectangular inputs (H != W, each a multiple of 32): the whole network in eval and train mode
against outputs of the imported reference (``tests/golden/net_rect.npz``, made by ``tests/gen_golden_rect.py``), every conv
kernel family on odd rectangular grids against an fp64 convolution, and the ``_hw`` post-processing / loss / metric kernels
against CPU restatements (with the square case through the ``_hw`` entry points bit-equal to the square entry points)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import loss as oloss
from oracle import net as onet
from oracle import postprocess as opp
from tests import golden_inputs as gi
from tests import rect_inputs as ri

pytestmark = pytest.mark.gpu
FWD_ATOL = 1e-3
TIGHT_ATOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHORS = gi.TRAIN_CASE["anchors"]


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return pkg


def _model(yt, nc, act, wseed, train=False):
    m = yt.YOLOv3(num_classes=nc, activation=act)
    m.load_state_dict(onet.synth_state_dict(wseed, 3, nc, gain=gi.NET_GAIN))
    m = m.cuda()
    return m.train() if train else m.eval()


# ------------------------------------------------------------------------------------------- whole network
@pytest.mark.parametrize("name", list(ri.RECT_NET_CASES))
def test_network_forward_rect_vs_golden(yt, golden, name):
    g = golden("net_rect")
    c = ri.RECT_NET_CASES[name]
    m = _model(yt, c["nc"], c["act"], c["wseed"])
    x = ri.rect_input(c["xseed"], c["batch"], c["H"], c["W"])
    with torch.no_grad():
        preds = m(x.cuda())
    assert len(preds) == 3
    for i, (p, s) in enumerate(zip(preds, (32, 16, 8))):
        assert tuple(p.shape) == (c["batch"], 3, c["H"] // s, c["W"] // s, 5 + c["nc"]) and p.dtype == torch.float32
        if f"{name}/p{i}" in g.files:
            got, ref = p.cpu().numpy(), g[f"{name}/p{i}"]
        else:
            got, ref = p.cpu().reshape(-1)[::3].numpy(), g[f"{name}/p{i}_every3"]
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        assert err <= FWD_ATOL, f"scale {i}: max abs err {err}"
        assert err <= TIGHT_ATOL, f"scale {i}: fp32 path should be well inside tolerance, got {err}"


def test_input_shape_errors_kept(yt):
    m = _model(yt, 2, "leaky_relu", 1)
    for shape in ((1, 3, 96, 100), (1, 3, 80, 96), (1, 4, 96, 160)):
        with pytest.raises(ValueError, match="^input must be"):
            with torch.no_grad():
                m(torch.zeros(shape, device="cuda"))
    m.train()
    with pytest.raises(ValueError, match="^input must be"):
        m(torch.zeros((2, 3, 96, 100), device="cuda"))


def _train_setup(yt, act, g, batch=None):
    c = ri.RECT_TRAIN_CASE
    m = _model(yt, c["nc"], act, c["wseed"], train=True)
    x = ri.rect_input(c["xseed"], batch or c["batch"], c["H"], c["W"]).cuda()
    tg = [torch.from_numpy(g[f"train{'_b4' if batch == 4 else ''}/target{i}"]).cuda() for i in range(3)]
    sa = ri.rect_scaled_anchors(c["anchors"], c["H"], c["W"]).cuda()
    return c, m, x, tg, sa


@pytest.mark.parametrize("tag,act", [("leaky", "leaky_relu"), ("mish", "mish")])
def test_network_train_step_rect_vs_golden(yt, golden, tag, act):
    """test_network_train_step_vs_golden at 96 x 160: loss parts, gradient norms of every parameter, sampled gradients (Mish:
    elementwise), running statistics and the SGD-updated first-layer weights against the reference's step."""
    g = golden("net_rect")
    c, m, x, tg, sa = _train_setup(yt, act, g)
    lf = yt.YOLOLoss()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    opt.zero_grad()
    preds = m(x)
    assert [tuple(p.shape) for p in preds] == [(2, 3, 3, 5, 7), (2, 3, 6, 10, 7), (2, 3, 12, 20, 7)]
    sums = np.stack([[float(p.detach().double().sum()), float(p.detach().double().abs().sum())] for p in preds])
    np.testing.assert_allclose(sums[:, 1], g[f"{tag}/pred_sums"][:, 1], rtol=1e-4)
    parts = torch.stack([torch.stack(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3)])
    np.testing.assert_allclose(parts.detach().cpu().numpy(), g[f"{tag}/loss_parts"], rtol=5e-4, atol=1e-5)
    parts.sum().backward()
    named = dict(m.named_parameters())
    for key in [k[len(tag) + 6:] for k in g.files if k.startswith(f"{tag}/grad/")]:
        got = named[key].grad.cpu()
        want = g[f"{tag}/grad/{key}"]
        got = got.reshape(-1)[::gi.TRAIN_GRAD_STRIDE].numpy() if got.numel() > 4096 else got.numpy()
        scale = max(1e-7, float(np.abs(want).max()))
        if act == "mish":                     # LeakyReLU: branch flips, see test_network_train_step_vs_golden
            assert float(np.abs(got - want).max()) <= 1e-3 * scale, key
    norms = np.array([float(p.grad.double().norm()) for p in m.parameters()])
    ref = g[f"{tag}/gradnorm_all"]
    np.testing.assert_allclose(norms, ref, rtol=5e-3, atol=1e-6 * float(ref.max()))
    np.testing.assert_allclose(m.state_dict()["layers.0.batch_norm.running_mean"].cpu().numpy(), g[f"{tag}/rm0"], atol=1e-5)
    np.testing.assert_allclose(m.state_dict()["layers.0.batch_norm.running_var"].cpu().numpy(), g[f"{tag}/rv0"], rtol=1e-4, atol=1e-6)
    opt.step()
    g0 = float(np.abs(g[f"{tag}/grad/layers.0.conv.weight"]).max())
    np.testing.assert_allclose(m.state_dict()["layers.0.conv.weight"].cpu().numpy(), g[f"{tag}/w0_after_sgd"], rtol=0,
                               atol=1e-3 * (1e-3 if act == "mish" else 5e-2) * g0 + 2e-6)


# Layer 0's BatchNorm gradients are sums of dy * zhat over every pixel of the batch: in bf16 (8-bit mantissa) their direction
# moves with the sample - cos 0.944 / 0.970 on this batch-4 rectangular step, 0.983 on the square golden step - while fp16,
# the same 16-bit kernels with an 11-bit mantissa, agrees to cos >= 0.9992 on both shapes (so the arithmetic is right and the
# spread is bf16 rounding). Those two vectors get 0.93 in bf16; every other key keeps the square bar.
BF16_LAYER0_BN = {"layers.0.batch_norm.weight", "layers.0.batch_norm.bias"}


@pytest.mark.parametrize("dtype,cos_min,norm_tol", [("fp16", 0.995, 0.03), ("bf16", 0.95, 0.12)])
def test_network_train_step_rect_16bit_vs_golden(yt, golden, dtype, cos_min, norm_tol):
    """The 16-bit autocast step (Mish) at 96 x 160 with the bars of test_network_train_step_16bit_vs_golden, at that test's
    batch of 4 (the golden's mish_b4 step)."""
    g = golden("net_rect")
    tag = "mish_b4"
    c, m, x, tg, sa = _train_setup(yt, "mish", g, batch=4)
    lf = yt.YOLOLoss()
    ac_dtype = torch.float16 if dtype == "fp16" else torch.bfloat16
    with torch.autocast("cuda", dtype=ac_dtype):
        preds = m(x)
        assert all(p.dtype == ac_dtype for p in preds)
        parts = torch.stack([torch.stack([t.float() for t in lf(preds[i], tg[i].clone(), sa[i])]) for i in range(3)])
    np.testing.assert_allclose(parts.detach().cpu().numpy(), g[f"{tag}/loss_parts"], rtol=norm_tol, atol=1e-3)
    parts.sum().backward()
    named = dict(m.named_parameters())
    for key in [k[len(tag) + 6:] for k in g.files if k.startswith(f"{tag}/grad/")]:
        got = named[key].grad.cpu()
        want = g[f"{tag}/grad/{key}"]
        got = got.reshape(-1)[::gi.TRAIN_GRAD_STRIDE].numpy() if got.numel() > 4096 else got.numpy()
        if np.abs(want).max() < 1e-12:
            continue
        cos = float((got.astype(np.float64) * want).sum() / (np.linalg.norm(got.astype(np.float64)) * np.linalg.norm(want) + 1e-30))
        bar = 0.93 if (dtype == "bf16" and key in BF16_LAYER0_BN) else cos_min
        assert cos >= bar, f"{dtype} {key}: cos {cos}"
    norms = np.array([float(p.grad.double().norm()) for p in m.parameters()])
    ref = g[f"{tag}/gradnorm_all"]
    big = ref > 1e-3 * ref.max()
    ratio = norms[big] / ref[big]
    assert np.all(np.abs(ratio - 1) <= norm_tol), f"{dtype}: gradient-norm ratio range {ratio.min():.3f} .. {ratio.max():.3f}"
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_graphed_train_step_rect_equals_eager(yt):
    """GraphedTrainStep captured at 96 x 160 walks the eager steps' parameter trajectory bit for bit (the square test's
    protocol: 3 warm-up steps on batch 0, then two replays, against 5 eager steps)."""
    nc, H, W, B = 2, 96, 160, 2
    sd = onet.synth_state_dict(71, 3, nc, gain=gi.NET_GAIN)
    sa = ri.rect_scaled_anchors(ANCHORS, H, W).cuda()
    batches = []
    for k in range(3):
        tg, _, _ = ri.rect_targets(B, H, W, nc, ANCHORS, 90 + k)
        batches.append((ri.rect_input(80 + k, B, H, W).cuda(), [torch.from_numpy(t).cuda() for t in tg]))

    def make():
        m = yt.YOLOv3(num_classes=nc, activation="mish")
        m.load_state_dict(sd)
        m = m.cuda().train()
        return m, torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    m1, o1 = make()
    lf = yt.FusedYOLOLoss()
    eager_losses = []
    for x, tg in [batches[0]] * 3 + [batches[1], batches[2]]:
        o1.zero_grad(set_to_none=True)
        preds = m1(x)
        loss = sum(sum(lf(preds[i], tg[i], sa[i])) for i in range(3))
        loss.backward()
        o1.step()
        eager_losses.append(float(loss.detach()))
    m2, o2 = make()
    step = yt.GraphedTrainStep(m2, o2, sa, batches[0][0], batches[0][1])
    l1 = float(step(*batches[1]))
    l2 = float(step(*batches[2]))
    assert l1 == eager_losses[3] and l2 == eager_losses[4]
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


# --------------------------------------------------------------------------------------- conv kernel families
def _check_blocks(worst):
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"beyond the bar (ratio): {bad}"
    assert len(worst) > 40


def test_conv_families_rect_vs_fp64(yt):
    from tests.workers import rect_blocks
    _check_blocks(rect_blocks.run())


@pytest.mark.parametrize("env", [{"YOLO_NO_WINOGRAD": "1"}, {"YOLO_WINO2_MAXPIX": "0"}])
def test_conv_families_rect_vs_fp64_switches(env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workers", "rect_blocks.py")], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_blocks(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))


# ------------------------------------------------------------------------- decode, loss, accuracy, targets
def _heads(B, gh, gw, nc, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((B, 3, gh, gw, 5 + nc), generator=gen) * 1.5


def _decode_cpu(p, anchors):
    """cells_to_boxes (utils.py:86-148) restated per axis in fp32."""
    B, _, gh, gw, D = p.shape
    a = anchors.reshape(1, 3, 1, 1, 2)
    col = torch.arange(gw, dtype=torch.float32).view(1, 1, 1, gw)
    row = torch.arange(gh, dtype=torch.float32).view(1, 1, gh, 1)
    inv_w, inv_h = np.float32(1.0 / gw), np.float32(1.0 / gh)
    cx = inv_w * (torch.sigmoid(p[..., 0]) + col)
    cy = inv_h * (torch.sigmoid(p[..., 1]) + row)
    w = inv_w * (torch.exp(p[..., 2]) * a[..., 0])
    h = inv_h * (torch.exp(p[..., 3]) * a[..., 1])
    obj = torch.sigmoid(p[..., 4])
    cls = torch.argmax(p[..., 5:], dim=-1).float()
    return torch.stack([cx, cy, w, h, obj, cls], -1).reshape(B, -1, 6)


@pytest.mark.parametrize("gh,gw", [(11, 19), (19, 11), (3, 5)])
def test_decode_hw_vs_cpu(yt, gh, gw):
    p = _heads(2, gh, gw, 4, gh * 100 + gw)
    anc = torch.tensor(ANCHORS[0]) * max(gh, gw)
    got = yt.decode_boxes(p.cuda(), anc, (gh, gw), mutate=False).cpu()
    ref = _decode_cpu(p, anc)
    assert got.shape == (2, 3 * gh * gw, 6)
    np.testing.assert_allclose(got[..., :5].numpy(), ref[..., :5].numpy(), rtol=2e-6, atol=1e-7)
    assert torch.equal(got[..., 5], ref[..., 5])
    lists = yt.cells_to_boxes(p.cuda(), anc, (gh, gw))
    assert len(lists) == 2 and len(lists[0]) == 3 * gh * gw


def test_square_through_hw_entry_points_is_bit_equal(yt):
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    g, B, nc = 13, 2, 5
    p = _heads(B, g, g, nc, 7).cuda()
    anc = (torch.tensor(ANCHORS[0]) * g).cuda().contiguous()
    st = (C.c_int64 * 5)(*p.stride())
    outs = []
    for hw in (False, True):
        b = torch.empty((B, 3 * g * g, 6), device="cuda")
        q = p.clone()
        if hw:
            L.check(lib.yolo_decode_hw(q.data_ptr(), st, anc.data_ptr(), B, g, g, nc, 1, b.data_ptr(), b.shape[1], 0, L.current_stream()))
        else:
            L.check(lib.yolo_decode(q.data_ptr(), st, anc.data_ptr(), B, g, nc, 1, b.data_ptr(), b.shape[1], 0, L.current_stream()))
        outs.append((b, q))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # loss forward / backward and accuracy
    t = torch.from_numpy(gi.synth_targets(B, 32 * g, nc, ANCHORS, 3)[0]).cuda()
    ws = torch.empty(lib.yolo_loss_workspace_bytes(B, g), dtype=torch.uint8, device="cuda")
    assert lib.yolo_loss_workspace_bytes(B, g) == lib.yolo_loss_workspace_bytes_hw(B, g, g)
    res = []
    for hw in (False, True):
        l4, c2 = torch.empty(4, device="cuda"), torch.empty(2, device="cuda")
        dp = torch.empty_like(p)
        go = torch.ones(4, device="cuda")
        cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
        if hw:
            L.check(lib.yolo_loss_fwd_hw(p.data_ptr(), st, t.data_ptr(), anc.data_ptr(), B, g, g, nc, l4.data_ptr(), c2.data_ptr(),
                                         ws.data_ptr(), ws.numel(), L.current_stream()))
            L.check(lib.yolo_loss_bwd_hw(p.data_ptr(), st, t.data_ptr(), anc.data_ptr(), B, g, g, nc, c2.data_ptr(), go.data_ptr(),
                                         dp.data_ptr(), L.current_stream()))
            L.check(lib.yolo_accuracy_counts_hw(p.data_ptr(), st, t.data_ptr(), B, g, g, nc, 0.5, cnt.data_ptr(), L.current_stream()))
        else:
            L.check(lib.yolo_loss_fwd(p.data_ptr(), st, t.data_ptr(), anc.data_ptr(), B, g, nc, l4.data_ptr(), c2.data_ptr(),
                                      ws.data_ptr(), ws.numel(), L.current_stream()))
            L.check(lib.yolo_loss_bwd(p.data_ptr(), st, t.data_ptr(), anc.data_ptr(), B, g, nc, c2.data_ptr(), go.data_ptr(),
                                      dp.data_ptr(), L.current_stream()))
            L.check(lib.yolo_accuracy_counts(p.data_ptr(), st, t.data_ptr(), B, g, nc, 0.5, cnt.data_ptr(), L.current_stream()))
        res.append((l4, c2, dp, cnt))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # head gradient to NHWC
    for dt in (0, 1, 2):
        ld = 32
        o1 = torch.empty(B * g * g * ld * 4, dtype=torch.uint8, device="cuda")
        o2 = torch.empty_like(o1)
        L.check(lib.yolo_head_grad_to_nhwc(p.data_ptr(), st, o1.data_ptr(), B, g, 5 + nc, ld, dt, L.current_stream()))
        L.check(lib.yolo_head_grad_to_nhwc_hw(p.data_ptr(), st, o2.data_ptr(), B, g, g, 5 + nc, ld, dt, L.current_stream()))
        n = B * g * g * ld * (4 if dt == 0 else 2)
        assert torch.equal(o1[:n], o2[:n])


def test_head_grad_to_nhwc_hw_layout(yt):
    from yolo_for_turbines_amd import _lib as L
    B, gh, gw, D, ld = 2, 5, 9, 7, 32
    p = torch.randn((B, 3, gh, gw, D), device="cuda").permute(0, 1, 3, 2, 4).contiguous().permute(0, 1, 3, 2, 4)   # strided view
    out = torch.empty((B, gh, gw, ld), device="cuda")
    st = (C.c_int64 * 5)(*p.stride())
    L.check(L.lib().yolo_head_grad_to_nhwc_hw(p.data_ptr(), st, out.data_ptr(), B, gh, gw, D, ld, 0, L.current_stream()))
    want = torch.zeros((B, gh, gw, ld), device="cuda")
    want[..., :3 * D] = p.permute(0, 2, 3, 1, 4).reshape(B, gh, gw, 3 * D)
    assert torch.equal(out, want)


@pytest.mark.parametrize("gh,gw", [(6, 10), (10, 6)])
def test_fused_loss_and_accuracy_hw_vs_cpu(yt, gh, gw):
    B, nc = 2, 3
    p = _heads(B, gh, gw, nc, gh + 31 * gw)
    tg, _, _ = ri.rect_targets(B, gh * 16, gw * 16, nc, ANCHORS, 17, mean_boxes=12)
    t = torch.from_numpy(tg[1])                          # the stride-16 scale: (B, 3, gh, gw, 6)
    assert tuple(t.shape[2:4]) == (gh, gw) and int((t[..., 4] == 1).sum()) > 0
    anc = ri.rect_scaled_anchors(ANCHORS, gh * 16, gw * 16)[1]
    pc = p.clone().requires_grad_(True)
    ref = oloss.yolo_loss(pc * 1.0, t.clone(), anc)
    sum(ref).backward()
    pg = p.cuda().requires_grad_(True)
    got = yt.FusedYOLOLoss()(pg, t.cuda(), anc.cuda())
    sum(got).backward()
    np.testing.assert_allclose(torch.stack(got).detach().cpu().numpy(), torch.stack(ref).detach().numpy(), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(pg.grad.cpu().numpy(), pc.grad.numpy(), rtol=1e-4, atol=1e-6)
    mirror = yt.YOLOLoss()(p.cuda().clone(), t.cuda().clone(), anc.cuda())
    np.testing.assert_allclose(torch.stack(mirror).cpu().numpy(), torch.stack(ref).detach().numpy(), rtol=2e-5, atol=1e-6)
    # accuracy counters (utils.py:355-372) restated
    cnt = yt.accuracy_counts([p.cuda()], [t.cuda()], 0.5).cpu().tolist()
    obj, noobj = t[..., 4] == 1, t[..., 4] == 0
    objp = torch.sigmoid(p[..., 4]) > 0.5
    want = [int((torch.argmax(p[..., 5:][obj], -1) == t[..., 5][obj].long()).sum()), int(obj.sum()), int(objp[obj].sum()),
            int((~objp[noobj]).sum()), int(noobj.sum())]
    assert cnt == want


def test_build_targets_hw_vs_restatement(yt):
    H, W, nc, B = 352, 608, 80, 3
    tg, boxes, counts = ri.rect_targets(B, H, W, nc, gi.COCO_ANCHORS, 29, mean_boxes=20)
    got = yt.build_targets(torch.from_numpy(boxes).cuda(), gi.COCO_ANCHORS, (H, W), counts=torch.from_numpy(counts))
    for k, (a, b) in enumerate(zip(got, tg)):
        assert tuple(a.shape) == (B, 3, H // (32 >> k), W // (32 >> k), 6)
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    # square (S, S) is image_size=S bit for bit
    S = 416
    _, boxes, counts = ri.rect_targets(B, S, S, nc, gi.COCO_ANCHORS, 31, mean_boxes=20)
    a = yt.build_targets(torch.from_numpy(boxes).cuda(), gi.COCO_ANCHORS, S, counts=torch.from_numpy(counts))
    b = yt.build_targets(torch.from_numpy(boxes).cuda(), gi.COCO_ANCHORS, (S, S), counts=torch.from_numpy(counts))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------- letterbox
def test_letterbox_rect(yt):
    gen = np.random.Generator(np.random.PCG64(5))
    ims = [gen.integers(0, 256, (1080, 1920, 3), dtype=np.uint8), gen.integers(0, 256, (300, 700, 3), dtype=np.uint8)]
    sq, msq = yt.letterbox(ims, 608)
    rc, mrc = yt.letterbox(ims, 608, rect=True)
    assert tuple(sq.shape) == (2, 3, 608, 608)
    assert tuple(rc.shape) == (2, 3, 352, 608)         # 342 and 261 rows -> 352
    for i, (a, b) in enumerate(zip(msq, mrc)):
        assert a[:4] == b[:4]                           # same resized size
        oh, ow, nh, nw, pt, pl = b
        assert pt == (352 - nh) // 2 and pl == (608 - nw) // 2
        pt0, pl0 = a[4], a[5]
        assert torch.equal(rc[i, :, pt:pt + nh, pl:pl + nw], sq[i, :, pt0:pt0 + nh, pl0:pl0 + nw])   # interior: same bits
        pad = torch.ones_like(rc[i], dtype=torch.bool)
        pad[:, pt:pt + nh, pl:pl + nw] = False
        assert float(rc[i][pad].abs().max()) == 0.0
        # round trip: a box in original coordinates -> canvas -> unletterbox_boxes(meta=) recovers it
        box = [0.3, 0.6, 0.2, 0.1, 0.9, 1.0]
        cx = (box[0] * nw + pl) / 608
        cy = (box[1] * nh + pt) / 352
        lb = [[cx, cy, box[2] * nw / 608, box[3] * nh / 352, 0.9, 1.0]]
        back = yt.unletterbox_boxes(lb, (oh, ow), (352, 608), meta=b)[0]
        np.testing.assert_allclose(back[:4], box[:4], rtol=1e-9, atol=1e-12)
    # the canvas comes from one query: a batch of one exact 16:9 frame resized to 608 x 342
    one, m1 = yt.letterbox([ims[0]], 608, rect=True)
    assert tuple(one.shape) == (1, 3, 352, 608) and m1[0][2:4] == (342, 608)


def test_unletterbox_reference_formula_vs_meta(yt):
    """The reference's formula re-derives the resize from the canvas: exact on a square canvas, not in general on a
    rectangular one (documented in unletterbox_boxes); meta= is exact for every aspect ratio."""
    gen = np.random.Generator(np.random.PCG64(9))
    for h, w in ((1080, 1920), (600, 800), (640, 608), (352, 1000)):
        im = gen.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for rect in (False, True):
            out, meta = yt.letterbox([im], 416, rect=rect)
            Hc, Wc = out.shape[2:]
            oh, ow, nh, nw, pt, pl = meta[0]
            box = [0.5, 0.5, 0.4, 0.3, 1.0, 0.0]
            lb = [[(box[0] * nw + pl) / Wc, (box[1] * nh + pt) / Hc, box[2] * nw / Wc, box[3] * nh / Hc, 1.0, 0.0]]
            back = yt.unletterbox_boxes(lb, (oh, ow), (Hc, Wc), meta=meta[0])[0]
            np.testing.assert_allclose(back[:4], box[:4], rtol=1e-9)
            plain = yt.unletterbox_boxes(lb, (oh, ow), (Hc, Wc))[0]       # the reference's call form still works
            assert len(plain) == 6


# ------------------------------------------------------------------------------------------ detection
def test_detect_images_rect_equals_decode_plus_nms(yt):
    nc, B, H, W = 4, 3, 160, 288
    m = _model(yt, nc, "leaky_relu", 21)
    x = ri.rect_input(22, B, H, W).cuda()
    sa = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, H, W)]
    boxes, keep, count = yt.detect_images(m, x, sa, 0.45, 0.5, "center")
    with torch.no_grad():
        preds = m(x)
    assert [tuple(p.shape[2:4]) for p in preds] == [(5, 9), (10, 18), (20, 36)]
    parts = [yt.decode_boxes(p.clone(), a, mutate=False) for p, a in zip(preds, sa)]
    ref = torch.cat(parts, 1)
    assert torch.equal(boxes, ref)
    for b in range(B):
        want = opp.nms_indices_c(ref[b].cpu().numpy(), 0.45, 0.5, "center")
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)


def test_full_size_fp16_608x352(yt):
    """Config-5 shape on a 16:9 canvas: fp16, B=16, 352 x 608 against the fp32 forward of the same model (2e-2 of max|fp32|,
    the fp16 bar of the square full-size checks); detect_images boxes have the rectangular count."""
    nc, B, H, W = 80, 16, 352, 608
    m = _model(yt, nc, "leaky_relu", 51)
    x = ri.rect_input(52, B, H, W).cuda()
    with torch.no_grad():
        ref = m(x)
        m._engine.compute_dtype = "fp16"
        got = m(x)
    for o, r in zip(got, ref):
        assert o.shape == r.shape
        assert float((o - r).abs().max()) <= 2e-2 * float(r.abs().max())
    sa = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, H, W)]
    boxes, keep, count = yt.detect_images(m, x, sa, 0.45, 0.5, "center")
    assert boxes.shape == (B, 3 * (11 * 19 + 22 * 38 + 44 * 76), 6)
    assert torch.isfinite(boxes).all() and int(count.min()) >= 0
