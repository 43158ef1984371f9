"""GPU parity tests (``-m gpu``): the HIP path, called through the C-ABI library, against
(1) the golden vectors generated from the imported reference and (2) the CPU oracle on the
same seeded inputs.  Tolerances: forward fp32 <= 1e-3 absolute (BASELINE.json north_star);
decode 2e-6 relative (device expf vs host); NMS kept indices bit-exact."""
import numpy as np
import pytest
import torch

from oracle import net as onet
from oracle import postprocess as opp
from tests import golden_inputs as gi

pytestmark = pytest.mark.gpu
F32 = np.float32
FWD_ATOL = 1e-3          # north-star tolerance
TIGHT_ATOL = 1e-4        # what the fp32 MFMA path actually achieves on these magnitudes


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as pkg
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return pkg


def _block(yt, i, act):
    cin, cout, k, s, bn, h = gi.BLOCK_CONFIGS[i]
    p = gi.block_params(i, cin, cout, k, bn)
    blk = yt.CNNBlock(cin, cout, batch_norm_act=bn, activation=act, kernel_size=k, stride=s, padding=1 if k == 3 else 0)
    blk.conv.weight.data.copy_(torch.from_numpy(p["w"]))
    if bn:
        blk.batch_norm.weight.data.copy_(torch.from_numpy(p["gamma"]))
        blk.batch_norm.bias.data.copy_(torch.from_numpy(p["beta"]))
        blk.batch_norm.running_mean.data.copy_(torch.from_numpy(p["mean"]))
        blk.batch_norm.running_var.data.copy_(torch.from_numpy(p["var"]))
    else:
        blk.conv.bias.data.copy_(torch.from_numpy(p["bias"]))
    return blk.cuda().eval(), torch.from_numpy(gi.block_input(i, cin, h))


@pytest.mark.parametrize("i", range(len(gi.BLOCK_CONFIGS)))
def test_conv_block_eval_vs_golden(yt, golden, i):
    g = golden("blocks")
    bn = gi.BLOCK_CONFIGS[i][4]
    for act in (("leaky_relu", "mish") if bn else ("leaky_relu",)):
        blk, x = _block(yt, i, act)
        with torch.no_grad():
            y = blk(x.cuda()).cpu()
        ref = g[f"cfg{i}/{act}/eval"]
        np.testing.assert_allclose(y.reshape(-1)[::gi.BLOCK_STRIDE].numpy(), ref, rtol=0, atol=TIGHT_ATOL)
        s = g[f"cfg{i}/{act}/eval_sums"]
        assert abs(float(y.double().abs().sum()) - s[1]) <= 1e-5 * s[1]


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("i", [0, 1, 2, 3, 7, 9, 10, 11, 15, 16, 18, 21, 22, 24])
def test_conv_block_every_tile_vs_oracle(yt, i, tile):
    """Full-tensor check of each tile shape against the oracle (not only the sampled golden)."""
    from yolo_for_turbines_amd import engine
    cin, cout, k, s, bn, h = gi.BLOCK_CONFIGS[i]
    blk, x = _block(yt, i, "leaky_relu")
    engine.module_state(blk).tile_override = tile          # per-module knob: no process-wide state is touched
    try:
        if tile >= 5 and (s != 1 or cin % 32):          # patch kernel: stride 1, cin % 32 == 0 only
            from yolo_for_turbines_amd._lib import YoloLibError
            with pytest.raises(YoloLibError, match="stride 1"):
                blk(x.cuda())
            return
        with torch.no_grad():
            y = blk(x.cuda()).cpu()
    finally:
        engine.module_state(blk).tile_override = None
    p = gi.block_params(i, cin, cout, k, bn)
    sd = {"b.conv.weight": torch.from_numpy(p["w"])}
    if bn:
        sd.update({"b.batch_norm.weight": torch.from_numpy(p["gamma"]), "b.batch_norm.bias": torch.from_numpy(p["beta"]),
                   "b.batch_norm.running_mean": torch.from_numpy(p["mean"]), "b.batch_norm.running_var": torch.from_numpy(p["var"])})
    else:
        sd["b.conv.bias"] = torch.from_numpy(p["bias"])
    with torch.no_grad():
        ref = onet.cnn_block(sd, dict(prefix="b", cin=cin, cout=cout, k=k, stride=s, bn=bn), x, "leaky_relu")
    assert y.shape == ref.shape
    np.testing.assert_allclose(y.numpy(), ref.numpy(), rtol=0, atol=TIGHT_ATOL)


def test_residual_and_head_blocks_vs_golden(yt, golden):
    g = golden("blocks")
    rb = yt.ResidualBlock(64, num_blocks=2)
    rb.load_state_dict({k[len("res64x2/sd/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("res64x2/sd/")})
    sp = yt.ScalePredictionBlock(128, num_classes=2)
    sp.load_state_dict({k[len("head128/sd/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("head128/sd/")})
    with torch.no_grad():
        yr = rb.cuda().eval()(torch.from_numpy(g["res64x2/x"]).cuda()).cpu().numpy()
        ys = sp.cuda().eval()(torch.from_numpy(g["head128/x"]).cuda()).cpu().numpy()
    np.testing.assert_allclose(yr, g["res64x2/y"], rtol=0, atol=TIGHT_ATOL)
    assert ys.shape == g["head128/y"].shape == (2, 3, 6, 6, 7)
    np.testing.assert_allclose(ys, g["head128/y"], rtol=0, atol=TIGHT_ATOL)


def _model(yt, c):
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=c["nc"], activation=c["act"])
    m.load_state_dict(sd)
    return m.cuda().eval()


@pytest.mark.parametrize("name", ["nc80_s96_b2_leaky", "nc2_s128_b1_leaky", "nc80_s96_b1_mish"])
def test_network_forward_full_vs_golden(yt, golden, name):
    g = golden("net_fwd")
    c = gi.NET_CASES[name]
    m = _model(yt, c)
    x = onet.synth_input(c["xseed"], c["batch"], c["size"])
    with torch.no_grad():
        preds = m(x.cuda())
    assert len(preds) == 3
    for i, p in enumerate(preds):
        ref = g[f"{name}/p{i}"]
        assert tuple(p.shape) == ref.shape and p.dtype == torch.float32
        err = np.abs(p.cpu().numpy() - ref).max()
        assert err <= FWD_ATOL, f"scale {i}: max abs err {err}"
        assert err <= TIGHT_ATOL, f"scale {i}: fp32 MFMA path should be well inside tolerance, got {err}"


@pytest.mark.parametrize("name", ["nc80_s416_b1_leaky", "nc80_s608_b1_leaky"])
def test_network_forward_sampled_vs_golden(yt, golden, name):
    g = golden("net_fwd")
    c = gi.NET_CASES[name]
    m = _model(yt, c)
    x = onet.synth_input(c["xseed"], c["batch"], c["size"])
    with torch.no_grad():
        preds = m(x.cuda())
    for i, p in enumerate(preds):
        flat = p.reshape(-1).cpu()
        np.testing.assert_allclose(flat[::gi.SAMPLE_STRIDE].numpy(), g[f"{name}/p{i}_sample"], rtol=0, atol=FWD_ATOL)
        s = g[f"{name}/p{i}_sums"]
        assert abs(float(flat.double().sum()) - s[0]) <= 2e-5 * s[1]
        assert abs(float(flat.double().abs().sum()) - s[1]) <= 2e-5 * s[1]


def test_network_batch_independence_and_determinism(yt):
    """Size-independent properties at the bench shape family: each image's output does not
    depend on its batch neighbours, and two runs are bitwise identical."""
    c = gi.NET_CASES["nc80_s96_b2_leaky"]
    m = _model(yt, c)
    x = onet.synth_input(123, 5, 160).cuda()
    with torch.no_grad():
        a = m(x)
        b = m(x)
        single = m(x[3:4])
    for pa, pb, ps in zip(a, b, single):
        assert torch.equal(pa, pb)
        assert torch.equal(pa[3:4], ps)


def test_nan_guards(yt):
    c = gi.NET_CASES["nc2_s128_b1_leaky"]
    m = _model(yt, c)
    x = onet.synth_input(5, 1, 64).cuda()
    x[0, 1, 3, 3] = float("nan")
    with pytest.raises(AssertionError):
        m(x)
    x = onet.synth_input(5, 1, 64).cuda()
    m.layers[4].layers[1][1].batch_norm.bias.data[3] = float("nan")
    m._engine.invalidate()
    with pytest.raises(ValueError, match="Nan in layer"):
        m(x)


def test_nan_guard_modes_in_train_mode(yt):
    """Train-mode forward: the guards of model.py:175,183-184 raise inside the forward by default; with
    ``nan_check = "deferred"`` the same exception comes from the next forward (train or eval) or from ``flush_nan()``, and a
    clean step in between raises nothing."""
    c = gi.NET_CASES["nc2_s128_b1_leaky"]
    m = _model(yt, c).train()
    good = onet.synth_input(5, 2, 64).cuda()
    bad = good.clone()
    bad[1, 2, 7, 9] = float("nan")
    with pytest.raises(AssertionError, match="NaN in the input"):
        m(bad)
    m._engine.nan_check = "deferred"
    m(good)
    m(good)
    m._engine.flush_nan()                                 # nothing to report
    preds = m(bad)                                        # returns; the guard is queued
    assert len(preds) == 3
    torch.cuda.synchronize()                              # (the poll of a later forward never waits: let the event complete)
    with pytest.raises(AssertionError, match="NaN in the input"):
        m(good)
    m(good)                                               # the report was consumed
    m(bad)
    with pytest.raises(AssertionError, match="NaN in the input"):
        m._engine.flush_nan()
    m._engine.flush_nan()                                 # idempotent
    for _ in range(12):                                   # more clean steps than slots without a sync in between
        m(good)
    m._engine.flush_nan()
    m(bad)
    m.eval()
    with torch.no_grad(), pytest.raises(AssertionError, match="NaN in the input"):
        m(good)                                           # an eval forward flushes (and waits)


def test_outputs_are_writable_and_fresh(yt):
    c = gi.NET_CASES["nc2_s128_b1_leaky"]
    m = _model(yt, c)
    x = onet.synth_input(5, 1, 64).cuda()
    with torch.no_grad():
        a = m(x)
        keep = [t.clone() for t in a]
        a[0][..., 0:2] = 0                    # callers mutate predictions in place (utils.py:106, loss.py:71)
        b = m(x)
    for k, t in zip(keep, b):
        assert torch.equal(k, t)


# ------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("name", list(gi.DECODE_CASES))
@pytest.mark.parametrize("layout", ["contiguous", "reference_view"])
def test_decode_vs_golden(yt, golden, name, layout):
    g = golden("decode")
    pred, anchors = gi.decode_input(name)
    grid = gi.DECODE_CASES[name]["g"]
    p = torch.from_numpy(pred.copy()).cuda()
    if layout == "reference_view":            # (B,3,D,g,g) memory viewed as (B,3,g,g,D), like model.py:147-148
        p = p.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
        assert not p.is_contiguous()
    boxes = yt.decode_boxes(p, torch.from_numpy(anchors), grid)
    ref = g[f"{name}/boxes"]
    got = boxes.cpu().numpy()
    np.testing.assert_allclose(got[..., :5], ref[..., :5], rtol=2e-6, atol=1e-7)
    np.testing.assert_array_equal(got[..., 5], ref[..., 5])
    np.testing.assert_allclose(p.cpu().numpy(), g[f"{name}/mutated"], rtol=2e-6, atol=1e-7)     # in-place side effect
    as_list = yt.cells_to_boxes(torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(anchors), grid)
    assert len(as_list) == pred.shape[0] and len(as_list[0]) == 3 * grid * grid and len(as_list[0][0]) == 6


def test_decode_targets_path(yt, golden):
    g = golden("decode")
    t = torch.from_numpy(gi.synth_targets(2, 96, 2, gi.TRAIN_CASE["anchors"], 55)[2]).cuda()
    boxes = yt.decode_boxes(t, torch.zeros(3, 2), 12, is_pred=False)
    np.testing.assert_array_equal(boxes.cpu().numpy(), g["targets_g12/boxes"])


# ---------------------------------------------------------------------------------- NMS
@pytest.mark.parametrize("name", list(gi.NMS_CASES))
def test_nms_indices_bit_exact_vs_golden(yt, golden, name):
    g = golden("nms")
    boxes, iou_thr, obj_thr, fmt = gi.nms_boxes(name)
    if len(boxes) == 0:
        assert yt.non_max_suppression([], iou_thr, obj_thr, fmt) == []
        return
    keep, count = yt.nms_indices(torch.from_numpy(boxes).cuda(), iou_thr, obj_thr, fmt)
    k = int(count)
    np.testing.assert_array_equal(keep[:k].cpu().numpy().astype(np.int64), g[f"{name}/keep"])


def test_nms_batched_ragged_thresholds(yt):
    """Several images at once, each with a different number of above-threshold boxes, against the
    C oracle; also the list wrapper returns the reference's rows."""
    rng = np.random.Generator(np.random.PCG64(4242))
    imgs = []
    for b in range(7):
        bx = gi.boxes_clustered(700, 5, 500 + b, n_gt=9, jitter=0.25)
        bx[:, 4] = rng.random(700).astype(F32) * (0.3 + 0.1 * b)        # image 0: almost nothing passes 0.25
        imgs.append(bx)
    batch = np.stack(imgs)
    keep, count = yt.nms_indices(torch.from_numpy(batch).cuda(), 0.4, 0.25, "center")
    for b in range(7):
        want = opp.nms_indices_c(batch[b], 0.4, 0.25, "center")
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)
    rows = yt.non_max_suppression(batch[3].tolist(), 0.4, 0.25, "center")
    np.testing.assert_array_equal(np.asarray(rows, F32), batch[3][opp.nms_indices_c(batch[3], 0.4, 0.25, "center")])


def test_nms_full_size_properties(yt):
    """BASELINE Config-5 size (10,000 post-threshold boxes x 16 images): idempotence (running NMS
    on the kept boxes keeps all of them, same order), score-sortedness, and exact agreement with
    the C oracle on every image."""
    B, N = 16, 10000
    batch = np.stack([gi.boxes_uniform(N, 80, 9000 + b) if b % 2 == 0 else gi.boxes_clustered(N, 80, 9000 + b, jitter=0.15)
                      for b in range(B)])
    t = torch.from_numpy(batch).cuda()
    keep, count = yt.nms_indices(t, 0.45, 0.5, "center")
    for b in range(B):
        k = int(count[b])
        idx = keep[b, :k].cpu().numpy()
        np.testing.assert_array_equal(idx, opp.nms_indices_c(batch[b], 0.45, 0.5, "center"))
        scores = batch[b][idx, 4]
        assert np.all(scores[:-1] >= scores[1:])
        again, c2 = yt.nms_indices(t[b, keep[b, :k].long()], 0.45, 0.5, "center")
        assert int(c2) == k and np.array_equal(again[:k].cpu().numpy(), np.arange(k))


def test_nms_class_sorted_path_awkward_classes(yt):
    """n >= 2048 takes the class-sorted path: class values that are fractional, negative, huge, -0.0 vs 0.0 and NaN
    (a NaN class never equals itself, so such a box never suppresses nor is suppressed), few and many classes, ragged
    numbers of valid boxes per image (including none and a single one) - exact indices against the C oracle."""
    rng = np.random.Generator(np.random.PCG64(777))
    palette = np.array([0.0, -0.0, 1.0, 2.0, 2.5, 0.5, -1.0, -3.0, 1e9, 4093.0, 4094.0, 4095.0, 5000.0, np.nan, 79.0, 3.0], F32)
    imgs = []
    for b in range(6):
        n = 3000
        bx = gi.boxes_clustered(n, 4, 600 + b, n_gt=12, jitter=0.2)
        if b < 4:
            bx[:, 5] = palette[rng.integers(0, len(palette), n)]
        elif b == 4:
            bx[:, 5] = 7.0                                   # one class: the dense O(n^2) case
        bx[:, 4] = rng.random(n).astype(F32)
        imgs.append(bx)
    imgs[1][:, 4] *= 0.2                                     # nothing above 0.25 -> no valid boxes
    imgs[2][:, 4] *= 0.2
    imgs[2][1234, 4] = 0.9                                   # exactly one valid box
    imgs[3][::3, 4] = 0.75                                   # many equal scores: index order breaks ties
    batch = np.stack(imgs)
    keep, count = yt.nms_indices(torch.from_numpy(batch).cuda(), 0.4, 0.25, "center")
    for b in range(6):
        want = opp.nms_indices_c(batch[b], 0.4, 0.25, "center")
        assert int(count[b]) == len(want)
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)
    assert int(count[1]) == 0 and int(count[2]) == 1
    keep, count = yt.nms_indices(torch.from_numpy(batch[0]).cuda(), 0.0, -1.0, "corner")     # thr 0: everything overlaps
    np.testing.assert_array_equal(keep[:int(count)].cpu().numpy(), opp.nms_indices_c(batch[0], 0.0, -1.0, "corner"))


@pytest.mark.parametrize("case", ["skewed", "one_class", "two_classes_32768", "three_classes", "tiny_ranges"])
def test_nms_class_scan_wave_teams(yt, case):
    """With at most 8 class ranges per image the class scan gives every range a team of waves (a leader on the serial chain,
    helpers for the far pushes): one class (15 helpers), 2 classes at 32,768 boxes (two column slices per helper pass), 3
    classes (teams of 5), a skewed histogram (one class with 90 % of the boxes, the rest sharing multi-class ranges, so the
    never-written-word checks of the team path are live), and ranges of one or two 64-row blocks. Dense overlap (clustered
    boxes) so that most rows are suppressed through far pushes. Kept indices exactly the C oracle's."""
    rng = np.random.Generator(np.random.PCG64(len(case) * 1009))
    if case == "skewed":
        imgs = []
        for b in range(3):
            bx = gi.boxes_clustered(6000, 1, 800 + b, n_gt=40, jitter=0.3)
            bx[:, 5] = np.where(rng.random(6000) < 0.9, 0.0, rng.integers(1, 6, 6000)).astype(F32)
            imgs.append(bx)
    elif case == "one_class":
        imgs = [gi.boxes_clustered(5000, 1, 810, n_gt=25, jitter=0.4), gi.boxes_uniform(5000, 1, 811)]
    elif case == "two_classes_32768":
        imgs = [gi.boxes_clustered(32768, 2, 820, n_gt=400, jitter=0.3)]
    elif case == "three_classes":
        imgs = [gi.boxes_clustered(7000, 3, 830 + b, n_gt=30, jitter=0.3) for b in range(2)]
    else:
        imgs = []
        for b in range(4):                                   # 2 .. 5 classes, 70 .. 200 valid boxes each among 2,048
            bx = gi.boxes_clustered(2048, 2 + b, 840 + b, n_gt=10, jitter=0.3)
            bx[:, 4] = np.where(rng.random(2048) < 0.06 + 0.05 * b, 0.6 + 0.4 * rng.random(2048), 0.1).astype(F32)
            imgs.append(bx)
    for bx in imgs:
        bx[:, 4] = np.maximum(bx[:, 4], F32(0.05))
    batch = np.stack(imgs)
    keep, count = yt.nms_indices(torch.from_numpy(batch).cuda(), 0.45, 0.5, "center")
    for b in range(len(imgs)):
        want = opp.nms_indices_c(batch[b], 0.45, 0.5, "center")
        assert int(count[b]) == len(want)
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)


@pytest.mark.parametrize("thr", [0.05, 0.3, 0.45, 0.5, 0.75, 0.95])
@pytest.mark.parametrize("scale", [1.0, 416.0, 1.0e4])
def test_nms_candidate_bounds_pairs_at_the_threshold(yt, thr, scale):
    """The mask kernel's first pass only admits pairs whose overlap is wide and high enough to reach the threshold at all
    (per-row bounds derived from thr); the exact pass decides the rest. Pairs built to sit within 1e-3 .. 1e-7 of the threshold
    - shifted copies, shifted along both axes, contained boxes, extreme aspect ratios, boxes a few ulps wide at the given
    coordinate scale - in two classes (class-uniform 64-blocks, the fast path) and n >= 2048 (the class-sorted path):
    kept indices exactly the C oracle's."""
    rng = np.random.Generator(np.random.PCG64(int(thr * 1000) + int(scale)))
    n_pairs = 2048
    w = scale * 10.0 ** rng.uniform(-4.0, -0.5, n_pairs)
    h = w * 10.0 ** rng.uniform(-1.5, 1.5, n_pairs)
    cx, cy = scale * rng.random(n_pairs), scale * rng.random(n_pairs)
    eps = rng.choice([1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 0.0], n_pairs) * rng.choice([-1.0, 1.0], n_pairs)
    t = np.clip(thr * (1.0 + eps), 1e-3, 0.999)
    kind = rng.integers(0, 4, n_pairs)
    px, py, pw, ph = cx.copy(), cy.copy(), w.copy(), h.copy()
    d = (1.0 - t) / (1.0 + t)                        # equal boxes shifted by d * extent along one axis: IoU = t
    px = np.where(kind == 0, cx + d * w, px)
    py = np.where(kind == 1, cy + d * h, py)
    s = 1.0 - np.sqrt(2.0 * t / (1.0 + t))          # shifted by s * extent along both: overlap (1 - s)^2 = 2 t / (1 + t)
    px = np.where(kind == 2, cx + s * w, px)
    py = np.where(kind == 2, cy - s * h, py)
    pw = np.where(kind == 3, w * t, pw)              # contained: IoU = area ratio = t
    cls = rng.integers(0, 2, n_pairs).astype(np.float64)
    score_a = 0.6 + 0.4 * rng.random(n_pairs)
    score_b = score_a - 0.05 * rng.random(n_pairs) - 1e-3
    a = np.stack([cx, cy, w, h, score_a, cls], 1)
    b = np.stack([px, py, pw, ph, score_b, cls], 1)
    boxes = np.concatenate([a, b]).astype(F32)
    boxes = boxes[rng.permutation(len(boxes))]
    keep, count = yt.nms_indices(torch.from_numpy(boxes).cuda(), thr, 0.5, "center")
    want = opp.nms_indices_c(boxes, thr, 0.5, "center")
    assert int(count) == len(want)
    np.testing.assert_array_equal(keep[:int(count)].cpu().numpy(), want)
    assert 32 < 2 * n_pairs - len(want) < 2 * n_pairs - 32             # both outcomes occur (at scale 1 the + 1e-6 of the denominator rescues tiny boxes)


@pytest.mark.parametrize("n,nc", [(2048, 80), (4096, 3), (4097, 80), (12288, 20), (22743, 80), (32768, 80), (33000, 80), (65537, 80)])
def test_nms_ordering_kernels_chunk_counts(yt, n, nc):
    """The hand-written ordering (2,048-key chunks sorted in LDS + rank merge) for 1 .. 33 chunks per image, chunk
    boundaries exactly at n, the largest grid of a forward (22,743 boxes at 608x608) and sizes that need several ranking
    rounds of 15 chunks (> 32,768 boxes; the class-sorted path and with it this ordering end at 163,456, which
    test_nms_routing_edge covers): kept indices bit-exact against the C oracle, images with different numbers of candidates
    (none, all, ties in the scores)."""
    rng = np.random.Generator(np.random.PCG64(n + nc))
    imgs = [gi.boxes_uniform(n, nc, 4000 + n), gi.boxes_clustered(n, nc, 4001 + n, jitter=0.15), gi.boxes_uniform(n, nc, 4002 + n)]
    imgs[1][:, 4] = 0.5 + 0.5 * rng.random(n).astype(F32)          # every box is a candidate
    imgs[1][::5, 4] = 0.875                                        # with many equal scores (index order decides)
    imgs[2][:, 4] *= 0.4                                           # no candidate at all
    batch = np.stack(imgs)
    keep, count = yt.nms_indices(torch.from_numpy(batch).cuda(), 0.45, 0.5, "center")
    assert int(count[2]) == 0
    for b in range(2):
        want = opp.nms_indices_c(batch[b], 0.45, 0.5, "center")
        assert int(count[b]) == len(want)
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)


# The class-sorted path needs one removed[] array of W = ceil(n / 64) words per wave beside the scan's fixed 16 W + 128 bytes
# in 60 KiB of LDS (nms_host.hip): K = (61,440 - 16 W - 128) / (8 W) >= 1 <=> 24 W + 128 <= 61,440 <=> W <= 2,554 <=> n <= 163,456.
NMS_LAST_CLASS_SORTED_N = ((60 * 1024 - 128) // 24) * 64


@pytest.mark.parametrize("n", [NMS_LAST_CLASS_SORTED_N, NMS_LAST_CLASS_SORTED_N + 1])
def test_nms_routing_edge(yt, n):
    """The two sizes either side of the cut between the class-sorted and the score-only path: n = 163,456 (W = 2,554, one
    wave per image in the class scan, 80 chunks, so the rank merges run six rounds of 15 chunks) and n = 163,457 (one
    library sort, then the plain mask and scan at W = 2,555). One image, about 2 % candidates, a block of tied scores:
    kept indices and count exactly the C oracle's. The workspace is the test's own (3.4 GB, freed at the end)."""
    from yolo_for_turbines_amd import _lib as L
    assert n in (163456, 163457)
    rng = np.random.Generator(np.random.PCG64(n))
    boxes = gi.boxes_uniform(n, 80, 5000 + n)
    boxes[:, 4] = rng.random(n).astype(F32)
    boxes[::100, 4] = 0.99                                         # equal scores: index order decides
    obj_thr = 0.98
    candidates = int(np.count_nonzero(boxes[:, 4].astype(np.float64) > obj_thr))
    assert 2000 <= candidates <= 6000
    want = opp.nms_indices_c(boxes, 0.45, obj_thr, "center")
    t = torch.from_numpy(boxes).cuda().unsqueeze(0).contiguous()
    keep = torch.empty((1, n), dtype=torch.int32, device="cuda")
    count = torch.empty((1,), dtype=torch.int32, device="cuda")
    lib = L.lib()
    ws = torch.empty(lib.yolo_nms_workspace_bytes(1, n), dtype=torch.uint8, device="cuda")
    try:
        L.check(lib.yolo_nms(t.data_ptr(), 1, n, 0.45, obj_thr, 1, keep.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                             L.current_stream()), "yolo_nms")
        got = keep[0, :int(count[0])].cpu().numpy()
    finally:
        del ws
        torch.cuda.empty_cache()
    assert int(count[0]) == len(want)
    np.testing.assert_array_equal(got, want)


def test_detect_pipeline_vs_oracle(yt):
    """forward -> decode (3 scales, reference concatenation order) -> NMS, against the oracle's
    decode of the oracle's forward; thresholds chosen so a few hundred boxes survive."""
    c = gi.NET_CASES["nc80_s96_b2_leaky"]
    m = _model(yt, c)
    x = onet.synth_input(77, 3, 128)
    with torch.no_grad():
        preds = m(x.cuda())
    anchors = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
               [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]
    sa = [torch.tensor(a) * p.shape[2] for a, p in zip(anchors, preds)]
    pc = [p.clone() for p in preds]
    boxes, keep, count = yt.detect(preds, sa, 0.45, 0.5, "center")
    for p, q in zip(preds, pc):                # the detect path leaves the prediction tensors alone (no caller reads them again) ...
        assert torch.equal(p, q)
    pm = [p.clone() for p in pc]
    boxes_m, keep_m, count_m = yt.detect(pm, sa, 0.45, 0.5, "center", mutate=True)
    assert torch.equal(boxes, boxes_m) and torch.equal(count, count_m)
    for b in range(3):                         # (entries of keep beyond count are unspecified)
        assert torch.equal(keep[b, :int(count[b])], keep_m[b, :int(count_m[b])])
    pcpu = [p.cpu() for p in pc]
    ref_boxes = torch.cat([opp.cells_to_boxes(p, a, p.shape[2]) for p, a in zip(pcpu, sa)], dim=1).numpy()
    for p, q in zip(pm, pcpu):                 # ... and mutate=True reproduces cells_to_boxes' in-place side effect (utils.py:106-110)
        np.testing.assert_allclose(p.cpu().numpy(), q.numpy(), rtol=3e-6, atol=1e-7)
    got = boxes.cpu().numpy()
    np.testing.assert_allclose(got[..., :5], ref_boxes[..., :5], rtol=3e-6, atol=1e-7)
    np.testing.assert_array_equal(got[..., 5], ref_boxes[..., 5])
    for b in range(3):                        # NMS exactness is defined on the boxes it was given
        want = opp.nms_indices_c(got[b], 0.45, 0.5, "center")
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)


# ------------------------------------------------------------------------- training path
def _train_block_check(yt, g, i, act, rel=2e-3):
    cin, cout, k, s, bn, h = gi.BLOCK_CONFIGS[i]
    blk, x = _block(yt, i, act)
    blk.train()
    tag = f"cfg{i}/{act}"
    xg = x.cuda().requires_grad_(True)
    y = blk(xg)
    gy = torch.from_numpy(np.random.Generator(np.random.PCG64(3000 + i)).standard_normal(tuple(y.shape), dtype=np.float32))
    y.backward(gy.cuda())
    yc = y.detach().cpu()
    np.testing.assert_allclose(yc.reshape(-1)[::gi.BLOCK_STRIDE].numpy(), g[f"{tag}/train"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(blk.batch_norm.running_mean.cpu().numpy(), g[f"{tag}/new_mean"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(blk.batch_norm.running_var.cpu().numpy(), g[f"{tag}/new_var"], rtol=1e-4, atol=1e-5)

    def close(got, want, what):
        scale = max(1e-6, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        assert err <= rel * scale, f"{tag} {what}: max err {err} vs scale {scale}"
    close(xg.grad.cpu().reshape(-1)[::gi.BLOCK_STRIDE].numpy(), g[f"{tag}/dx"], "dx")
    close(blk.conv.weight.grad.cpu().reshape(-1)[::gi.BLOCK_DW_STRIDE].numpy(), g[f"{tag}/dw"], "dw")
    close(blk.batch_norm.weight.grad.cpu().numpy(), g[f"{tag}/dgamma"], "dgamma")
    close(blk.batch_norm.bias.grad.cpu().numpy(), g[f"{tag}/dbeta"], "dbeta")
    s_dx = g[f"{tag}/dx_sums"]
    assert abs(float(xg.grad.double().abs().sum().cpu()) - s_dx[1]) <= 2e-3 * s_dx[1]
    s_dw = g[f"{tag}/dw_sums"]
    assert abs(float(blk.conv.weight.grad.double().abs().sum().cpu()) - s_dw[1]) <= 2e-3 * s_dw[1]


@pytest.mark.parametrize("i", [i for i, c in enumerate(gi.BLOCK_CONFIGS) if c[4]])
def test_block_train_forward_backward_vs_golden(yt, golden, i):
    """BatchNorm(train) forward + running stats, and dx / dW / dgamma / dbeta for a fixed upstream
    gradient, for every BN conv configuration (stride 1 and 2, 1x1 and 3x3, cin = 3 .. 1024)."""
    g = golden("blocks")
    for act in ("leaky_relu", "mish"):
        _train_block_check(yt, g, i, act)


@pytest.mark.parametrize("tag,act", [("leaky", "leaky_relu"), ("mish", "mish")])
def test_network_train_step_vs_golden(yt, golden, tag, act):
    """One fine-tune step (train.py:41-69 sequence: forward in train mode, 3 x YOLOLoss, backward,
    SGD) against the reference: loss parts, sampled gradients, per-parameter gradient norms of ALL
    366 parameters, updated running statistics and the SGD-updated first-layer weights."""
    g = golden("train_step")
    c = gi.TRAIN_CASE
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=c["nc"], activation=act)
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = onet.synth_input(c["xseed"], c["batch"], c["size"]).cuda()
    tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(c["batch"], c["size"], c["nc"], c["anchors"], c["tseed"])]
    grids = [c["size"] // 32, c["size"] // 16, c["size"] // 8]
    sa = (torch.tensor(c["anchors"]) * torch.tensor(grids).view(3, 1, 1)).cuda()
    lf = yt.YOLOLoss()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    opt.zero_grad()
    preds = m(x)
    sums = np.stack([[float(p.detach().double().sum()), float(p.detach().double().abs().sum())] for p in preds])
    np.testing.assert_allclose(sums[:, 1], g[f"{tag}/pred_sums"][:, 1], rtol=1e-4)
    parts = torch.stack([torch.stack(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3)])
    np.testing.assert_allclose(parts.detach().cpu().numpy(), g[f"{tag}/loss_parts"], rtol=5e-4, atol=1e-5)
    total = parts.sum()
    total.backward()
    named = dict(m.named_parameters())
    for key in [k[len(tag) + 6:] for k in g.files if k.startswith(f"{tag}/grad/")]:
        got = named[key].grad.cpu()
        want = g[f"{tag}/grad/{key}"]
        got = got.reshape(-1)[::gi.TRAIN_GRAD_STRIDE].numpy() if got.numel() > 4096 else got.numpy()
        scale = max(1e-7, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        # Elementwise bar against the reference's fp32 run: Mish only (smooth: fp32 implementations agree to ~5e-5 of
        # max|g|). LeakyReLU's derivative jumps 0.1 -> 1 at u = 0: the reference's own fp32 run takes a handful of
        # branches differently from its float64 run (tests/golden/train_step_fp64.npz: single gradient entries of the early
        # layers move by 1.5e-3 of max|g|), and another fp32 implementation takes a different handful. The LeakyReLU
        # elementwise bar is therefore enforced against a float64 run ON THE SAME BRANCHES in
        # test_network_train_step_leaky_vs_fp64_on_matched_branches (1e-3 of max|g|, every parameter); here the leaky case
        # keeps the loss parts above and the 366 per-parameter gradient norms below.
        if act == "mish":
            assert err <= 1e-3 * scale, f"{key}: max err {err} vs scale {scale}"
    norms = np.array([float(p.grad.double().norm()) for p in m.parameters()])
    ref = g[f"{tag}/gradnorm_all"]
    assert norms.shape == ref.shape
    np.testing.assert_allclose(norms, ref, rtol=5e-3, atol=1e-6 * float(ref.max()))
    np.testing.assert_allclose(m.state_dict()["layers.0.batch_norm.running_mean"].cpu().numpy(), g[f"{tag}/rm0"], atol=1e-5)
    np.testing.assert_allclose(m.state_dict()["layers.0.batch_norm.running_var"].cpu().numpy(), g[f"{tag}/rv0"], rtol=1e-4, atol=1e-6)
    opt.step()
    g0 = float(np.abs(g[f"{tag}/grad/layers.0.conv.weight"]).max())      # update = lr * (momentum-free first step)
    np.testing.assert_allclose(m.state_dict()["layers.0.conv.weight"].cpu().numpy(), g[f"{tag}/w0_after_sgd"], rtol=0,
                               atol=1e-3 * (1e-3 if act == "mish" else 5e-2) * g0 + 2e-6)
    # the packed weights follow the optimizer: a second forward must see the updated parameters
    m.eval()
    with torch.no_grad():
        a = m(x)
    assert all(torch.isfinite(t).all() for t in a)


@pytest.mark.parametrize("tag,act", [("leaky", "leaky_relu"), ("mish", "mish")])
@pytest.mark.parametrize("opt_kind", ["yt", "torch"])
def test_network_train_trajectory_vs_golden(yt, golden, tag, act, opt_kind):
    """THREE iterations of the reference's loop body (train.py:41-82: zero_grad, forward, 3 x YOLOLoss, backward,
    optimizer.step, LinearLR.step) against the trajectory the imported reference walked (tests/golden/train_traj.npz):
    loss parts of every step (step 2+ see weights re-packed after optimizer.step, momentum, weight decay, the moving
    learning rate), gradient norms of all 366 parameters at step 3, accumulated running statistics,
    num_batches_tracked, parameter / momentum-buffer norms and two sampled weight tensors after step 3."""
    g = golden("train_traj")
    c = gi.TRAIN_CASE
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=c["nc"], activation=act)
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = onet.synth_input(c["xseed"], c["batch"], c["size"]).cuda()
    tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(c["batch"], c["size"], c["nc"], c["anchors"], c["tseed"])]
    grids = [c["size"] // 32, c["size"] // 16, c["size"] // 8]
    sa = (torch.tensor(c["anchors"]) * torch.tensor(grids).view(3, 1, 1)).cuda()
    lf = yt.YOLOLoss()
    opt = (yt.SGD if opt_kind == "yt" else torch.optim.SGD)(m.parameters(), **gi.TRAJ_OPT)
    sched = torch.optim.lr_scheduler.LinearLR(opt, **gi.TRAJ_SCHED)
    # Conditioning (tests/golden/train_traj.npz */perturbed_totals = the REFERENCE's own code on inputs perturbed by 1e-6): with
    # Mish the summed loss of every step moves by ~1e-5, so the trajectory is pinned elementwise. With LeakyReLU it moves by
    # 0.9 % at step 2 and 5 % at step 3 (the deepest BatchNorm layers normalise over 36 values per channel at this size; a
    # handful of |u| ~ 1e-6 elements on the other side of the kink re-route whole channels), so no fp32 implementation with a
    # different accumulation order can follow the reference's run closer than that: steps 2+ are bounded by twice the
    # reference's own spread, step 1 (same weights, no dynamics yet) stays elementwise.
    smooth = act == "mish"
    ref_tot = g[f"{tag}/loss_parts"].sum(axis=(1, 2))
    spread = np.abs(g[f"{tag}/perturbed_totals"] - ref_tot[None]).max(axis=0)
    for step in range(gi.TRAJ_STEPS):
        opt.zero_grad()
        preds = m(x)
        parts = torch.stack([torch.stack(lf(preds[i], tg[i].clone(), sa[i])) for i in range(3)])
        got = parts.detach().cpu().numpy()
        if smooth or step == 0:
            np.testing.assert_allclose(got, g[f"{tag}/loss_parts"][step], rtol=1e-3, atol=2e-5)
        else:
            assert abs(float(got.sum()) - ref_tot[step]) <= 2.0 * spread[step], (step, float(got.sum()), ref_tot[step], spread[step])
        parts.sum().backward()
        assert abs(opt.param_groups[0]["lr"] - g[f"{tag}/lrs"][step]) < 1e-12
        opt.step()
        sched.step()
    st = m.state_dict()
    assert int(st["layers.0.batch_norm.num_batches_tracked"]) == int(g[f"{tag}/nbt0"]) == gi.TRAJ_STEPS
    # (LeakyReLU: the first layer's weights have walked a slightly different path by step 3, so its batch statistics are only
    #  a sanity bound there: 3 x momentum 0.1 x the ~1e-2 the batch mean can move)
    np.testing.assert_allclose(st["layers.0.batch_norm.running_mean"].cpu().numpy(), g[f"{tag}/rm0"], atol=1e-5 if smooth else 5e-3)
    np.testing.assert_allclose(st["layers.0.batch_norm.running_var"].cpu().numpy(), g[f"{tag}/rv0"], rtol=1e-4 if smooth else 5e-2, atol=1e-6)
    pn = np.array([float(p.detach().double().norm()) for p in m.parameters()])
    np.testing.assert_allclose(pn, g[f"{tag}/param_norms"], rtol=2e-5 if smooth else 2e-2, atol=0 if smooth else 1e-3)
    if smooth:
        norms = np.array([float(p.grad.double().norm()) for p in m.parameters()])
        ref = g[f"{tag}/gradnorm_step3"]
        np.testing.assert_allclose(norms, ref, rtol=5e-3, atol=1e-6 * float(ref.max()))
        np.testing.assert_allclose(st["layers.28.batch_norm.running_var"].cpu().numpy(), g[f"{tag}/rv_last"], rtol=5e-3, atol=1e-5)
        mn = np.array([float(opt.state[p]["momentum_buffer"].double().norm()) for p in m.parameters()])
        refm = g[f"{tag}/momentum_norms"]
        np.testing.assert_allclose(mn, refm, rtol=5e-3, atol=1e-6 * float(refm.max()))
        for k in gi.TRAJ_WEIGHT_KEYS:
            want = g[f"{tag}/w/{k}"]
            got = st[k].reshape(-1)[::7].cpu().numpy()
            # the weights moved by sum(lr_t * update_t) ~ 6e-3 * |g|: compare the MOVEMENT, not the (much larger) weights
            w0 = sd[k].reshape(-1)[::7].numpy()
            moved = float(np.abs(want - w0).max())
            assert moved > 0
            assert float(np.abs(got - want).max()) <= 2e-3 * moved + 1e-7, k


def test_network_forward_in_channels_1_vs_golden(yt, golden):
    """A network built with in_channels=1 (model.py:151): no 3-channel stem kernel applies, the first block goes through
    the NHWC boundary copy and the generic convolution kernels. fp32 against the reference's outputs, 16-bit against the
    same numbers at the 16-bit network tolerance."""
    g = golden("net_in1")
    c = gi.NET_IN1
    sd = onet.synth_state_dict(c["wseed"], c["in_channels"], c["nc"], gain=gi.NET_GAIN)
    m = yt.YOLOv3(in_channels=c["in_channels"], num_classes=c["nc"], activation=c["act"])
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = onet.synth_input(c["xseed"], c["batch"], c["size"], c["in_channels"]).cuda()
    with torch.no_grad():
        preds = m(x)
    for i, p in enumerate(preds):
        ref = g[f"p{i}"]
        assert tuple(p.shape) == ref.shape
        np.testing.assert_allclose(p.cpu().numpy(), ref, rtol=0, atol=1e-4)
    with pytest.raises(ValueError, match="input must be"):
        m(torch.zeros(2, 3, 96, 96, device="cuda"))
    m.train()                                     # and one fine-tune step runs (gradients finite, first-layer dW has 1 input channel)
    po = m(x)
    sum(p.float().square().mean() for p in po).backward()
    assert m.layers[0].conv.weight.grad.shape == (32, 1, 3, 3)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_network_train_step_leaky_vs_fp64_on_matched_branches(yt, golden):
    """The LeakyReLU fine-tune step against FLOAT64, elementwise, every parameter.

    A LeakyReLU network's gradient is discontinuous in the pre-activations: an element with |u| ~ 1e-6 whose sign two
    implementations disagree on changes its dz by 0.9 dy, and ONE such element in a 3x3x1024 map shifts every gradient
    below it by ~1e-2 of its scale. So the float64 oracle is evaluated on the branches the GPU forward actually took
    (`leaky_masks`, from the saved pre-activations) — then nothing discontinuous is left and the bar is the Mish bar,
    1e-3 of max|g| — and, separately, the number of branches that differ from the float64 run's own is bounded: it
    must be a handful out of 8.6 M, of the order of what the reference's fp32 run shows (train_step_fp64.npz vs
    train_step.npz). Also reports the judge's metric |ours - fp64| vs |reference fp32 - fp64| on the golden samples."""
    from oracle import loss as oloss
    c = gi.TRAIN_CASE
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=c["nc"], activation="leaky_relu")
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = onet.synth_input(c["xseed"], c["batch"], c["size"])
    tg = [torch.from_numpy(t) for t in gi.synth_targets(c["batch"], c["size"], c["nc"], c["anchors"], c["tseed"])]
    grids = [c["size"] // 32, c["size"] // 16, c["size"] // 8]
    sa = torch.tensor(c["anchors"]) * torch.tensor(grids).view(3, 1, 1)
    lf = yt.YOLOLoss()
    preds = m(x.cuda())
    sum(sum(lf(preds[i], tg[i].clone().cuda(), sa[i].cuda())) for i in range(3)).backward()
    # branches taken by the GPU forward: u = (z - mean) * (gamma * invstd) + beta from the saved raw conv outputs
    plan = [p for k, p in m._engine._plans.items() if k[0] == "train"][-1]
    names = {id(mod): name for name, mod in m.named_modules()}
    masks, B = {}, c["batch"]
    for i, op in enumerate(plan.prog.ops):
        if plan.z[i] is None:
            continue
        st, cout = plan.stats[i], op["block"].conv.out_channels
        z = plan.z[i].view(B, op["Ho"], op["Wo"], cout)
        u = (z - st[0]) * st[2] + st[3]
        masks[names[id(op["block"])]] = (u > 0).permute(0, 3, 1, 2).cpu()
    # float64 oracle: (a) its own branches (how many differ?), (b) the GPU's branches (gradients)
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    taps = {}
    with torch.no_grad():
        onet.forward(sd64, x.double(), c["nc"], "leaky_relu", training=True, new_stats={}, taps=taps)
    differ = 0
    for cv in onet.conv_list(3, c["nc"]):
        if cv["bn"]:                                              # the tap is y = leaky(u): same sign as u
            differ += int(((taps[cv["prefix"]] > 0) != masks[cv["prefix"]]).sum())
    total = sum(int(v.numel()) for v in masks.values())
    par = {k: v.clone().requires_grad_(True) for k, v in sd64.items() if v.dtype.is_floating_point and "running" not in k}
    full = dict(sd64)
    full.update(par)
    pr = onet.forward(full, x.double(), c["nc"], "leaky_relu", training=True, new_stats={}, leaky_masks=masks)
    sum(sum(oloss.yolo_loss(pr[i], tg[i].clone().double(), sa[i].double())) for i in range(3)).backward()
    worst, worst_key = 0.0, None
    for k, p in m.named_parameters():
        ref = par[k].grad
        e = float((p.grad.cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-30))
        if e > worst:
            worst, worst_key = e, k
    g64, g32 = golden("train_step_fp64"), golden("train_step")
    named = dict(m.named_parameters())
    ratios = {}
    for key in [k[len("leaky/grad/"):] for k in g64.files if k.startswith("leaky/grad/")]:
        got = named[key].grad.cpu().double()
        got = got.reshape(-1)[::gi.TRAIN_GRAD_STRIDE].numpy() if got.numel() > 4096 else got.numpy()
        w64, w32 = g64[f"leaky/grad/{key}"], g32[f"leaky/grad/{key}"]
        ratios[key] = float(np.abs(got - w64).max() / max(np.abs(w32 - w64).max(), 1e-30))
    print(f"leaky train step: {differ} of {total} branches differ from the float64 run; on matched branches max elementwise "
          f"gradient error {worst:.2e} of max|g| ({worst_key}); unmatched |ours-fp64| / |reference fp32-fp64| per golden sample: "
          + ", ".join(f"{k.split('.conv')[0].split('.batch')[0]}={v:.1f}" for k, v in ratios.items()))
    assert differ <= 64, differ                                   # a handful of |u| ~ 1e-6 elements out of ~8.6 M
    assert worst <= 1e-3, (worst_key, worst)
    # Un-matched comparison, asserted where it can be: the head convolutions sit behind at most one LeakyReLU whose flipped
    # elements reach them, so there |ours - fp64| stays within a small multiple of the reference's own fp32 error
    # (measured 0.7 - 1.7; the early layers, where a flipped branch moves a whole gradient column, read 7 - 15 and are
    # covered by the matched-branch bound above)
    for key, v in ratios.items():
        if ".pred_block.1." in key:
            assert v <= 3.0, (key, v)


# ------------------------------------------------------------- multi-scale sizes (train.py:45-46)
@pytest.mark.parametrize("size,batch", [(32, 3), (64, 1), (320, 2), (352, 1), (480, 1), (608, 1)])
def test_network_forward_multiscale_vs_oracle(yt, size, batch):
    """Every S that multi-scale training / Config 5 uses gives odd grid widths (10, 11, 15, 19, 38, 76 ...):
    tile selection and halo handling must be shape-generic. Oracle = CPU restatement on the same input."""
    nc = 2
    sd = onet.synth_state_dict(31, 3, nc, gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=nc)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = onet.synth_input(size, batch, size)
    with torch.no_grad():
        ref = onet.forward(sd, x, nc)
        out = m(x.cuda())
    for o, r in zip(out, ref):
        assert tuple(o.shape) == tuple(r.shape)
        err = float((o.cpu() - r).abs().max())
        assert err <= TIGHT_ATOL, f"S={size}: max abs err {err}"


def test_network_train_step_multiscale_vs_oracle(yt):
    """Gradients at S = 160 (grids 5/10/20, batch 3) against the oracle under autograd (Mish: smooth, so the
    elementwise comparison is meaningful — see test_network_train_step_vs_golden)."""
    from oracle import loss as oloss
    nc, S, B = 2, 160, 3
    sd = onet.synth_state_dict(41, 3, nc, gain=gi.NET_GAIN)
    x = onet.synth_input(42, B, S)
    anchors = gi.TRAIN_CASE["anchors"]
    tg = [torch.from_numpy(t) for t in gi.synth_targets(B, S, nc, anchors, 43)]
    grids = [S // 32, S // 16, S // 8]
    sa = torch.tensor(anchors) * torch.tensor(grids).view(3, 1, 1)
    par = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    full = dict(sd)
    full.update(par)
    pr = onet.forward(full, x, nc, "mish", training=True, new_stats={})
    sum(sum(oloss.yolo_loss(pr[i], tg[i].clone(), sa[i])) for i in range(3)).backward()
    m = yt.YOLOv3(num_classes=nc, activation="mish")
    m.load_state_dict(sd)
    m = m.cuda().train()
    lf = yt.YOLOLoss()
    po = m(x.cuda())
    sum(sum(lf(po[i], tg[i].clone().cuda(), sa[i].cuda())) for i in range(3)).backward()
    for k, p in m.named_parameters():
        ref_g = par[k].grad
        rel = float((p.grad.cpu() - ref_g).abs().max() / (ref_g.abs().max() + 1e-12))
        assert rel < 2e-3, f"{k}: {rel}"


# ------------------------------------------------------------- bf16 / fp16 path (BASELINE configs 4-5)
H16_TOL = {"bf16": 2.5e-2, "fp16": 4e-3}       # block level, relative to max|y|: one rounding of x, w and y to 8 / 11 bits


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("i", [i for i, c in enumerate(gi.BLOCK_CONFIGS) if c[0] % 32 == 0])
def test_conv_block_16bit_vs_oracle(yt, i, dtype):
    """Every 16-bit-eligible conv config (1x1, 3x3 stride 1 and 2, bare heads) against the fp32 oracle;
    the tolerance is the rounding of inputs / weights / outputs to the 16-bit format, not more."""
    from yolo_for_turbines_amd import engine
    cin, cout, k, s, bn, h = gi.BLOCK_CONFIGS[i]
    blk, x = _block(yt, i, "leaky_relu")
    p = gi.block_params(i, cin, cout, k, bn)
    sd = {"b.conv.weight": torch.from_numpy(p["w"])}
    if bn:
        sd.update({"b.batch_norm.weight": torch.from_numpy(p["gamma"]), "b.batch_norm.bias": torch.from_numpy(p["beta"]),
                   "b.batch_norm.running_mean": torch.from_numpy(p["mean"]), "b.batch_norm.running_var": torch.from_numpy(p["var"])})
    else:
        sd["b.conv.bias"] = torch.from_numpy(p["bias"])
    with torch.no_grad():
        ref = onet.cnn_block(sd, dict(prefix="b", cin=cin, cout=cout, k=k, stride=s, bn=bn), x, "leaky_relu")
    engine.module_state(blk).compute_dtype = dtype
    try:
        with torch.no_grad():
            y = blk(x.cuda()).cpu()
    finally:
        engine.module_state(blk).compute_dtype = None
    assert y.shape == ref.shape and y.dtype == torch.float32
    err = float((y - ref).abs().max() / ref.abs().max())
    assert err <= H16_TOL[dtype], f"cfg {i} {dtype}: rel err {err}"


@pytest.mark.parametrize("dtype,tol", [("fp16", 2e-2), ("bf16", 1.2e-1)])
def test_network_forward_16bit_vs_oracle(yt, dtype, tol):
    """Whole forward in fp16 / bf16 (explicit compute dtype and through torch.autocast) against the fp32
    oracle, next to what the oracle itself loses under CPU autocast(bf16) on the same weights."""
    c = gi.NET_CASES["nc80_s96_b2_leaky"]
    m = _model(yt, c)
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    x = onet.synth_input(c["xseed"], 2, 160)
    with torch.no_grad():
        ref = onet.forward(sd, x, c["nc"])
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref_bf16 = onet.forward(sd, x, c["nc"])
        m._engine.compute_dtype = dtype
        out = m(x.cuda())
        m._engine.compute_dtype = None
        ac_dtype = torch.float16 if dtype == "fp16" else torch.bfloat16
        with torch.autocast("cuda", dtype=ac_dtype):
            out_ac = m(x.cuda())                                    # heads in the autocast dtype, like the reference's (model.py:145-148)
            m._engine.autocast_heads = False
            out_ac32 = m(x.cuda())
            m._engine.autocast_heads = True
    for o, oa, oa32, r, rb in zip(out, out_ac, out_ac32, ref, ref_bf16):
        assert o.dtype == torch.float32 and tuple(o.shape) == tuple(r.shape)
        assert oa.dtype == ac_dtype and oa32.dtype == torch.float32
        assert torch.equal(o, oa32)                                 # autocast selects the same kernels ...
        assert torch.equal(o.to(ac_dtype), oa)                      # ... and hands the fp32 heads out rounded once
        scale = float(r.abs().max())
        err = float((o.cpu() - r).abs().max()) / scale
        err_cpu_bf16 = float((rb.float() - r).abs().max()) / scale
        assert err <= tol, f"{dtype}: rel err {err} (CPU autocast bf16 loses {err_cpu_bf16})"
        if dtype == "bf16":
            assert err <= 3 * err_cpu_bf16 + 1e-2


def test_config5_shape_fp16_forward_decode_nms(yt):
    """BASELINE config 5 per-GPU shape family: 608x608 fp16 forward (grids 19/38/76 -> 22,743 boxes per
    image), device decode in the reference's concatenation order, per-image NMS. Forward vs the fp32 oracle
    within the fp16 tolerance; NMS kept indices bit-exact against the C oracle ON THE BOXES IT WAS GIVEN."""
    nc, S, B = 80, 608, 2
    sd = onet.synth_state_dict(51, 3, nc, gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=nc)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    m._engine.compute_dtype = "fp16"
    x = onet.synth_input(52, B, S)
    with torch.no_grad():
        ref = onet.forward(sd, x[:1], nc)
        preds = m(x.cuda())
    for o, r in zip(preds, ref):
        assert tuple(o.shape[1:]) == tuple(r.shape[1:])
        assert float((o[:1].cpu() - r).abs().max()) <= 2e-2 * float(r.abs().max())
    anchors = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
               [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]
    sa = [torch.tensor(a) * p.shape[2] for a, p in zip(anchors, preds)]
    boxes, keep, count = yt.detect(preds, sa, 0.45, 0.5, "center")
    assert boxes.shape == (B, 22743, 6)
    bh = boxes.cpu().numpy()
    for b in range(B):
        want = opp.nms_indices_c(bh[b], 0.45, 0.5, "center")
        np.testing.assert_array_equal(keep[b, :int(count[b])].cpu().numpy(), want)


# ------------------------------------------------------------- 16-bit fine-tune step (Config 4 arithmetic)
H16_TRAIN_TOL = {"bf16": 4e-2, "fp16": 6e-3}    # block level, relative to max|reference|
# Gradient bar (relative L2). Mish is smooth: the error is the operand rounding. LeakyReLU's derivative jumps at
# u = 0: rounding z to b bits flips the branch of a fraction ~2^-b of the elements and each flip moves du by
# 0.9|dy|, so the L2 error is ~sqrt(2^-b) — 2 % in fp16, 6 % in bf16 — for ANY 16-bit implementation.
H16_GRAD_L2 = {("mish", "bf16"): 2.5e-2, ("mish", "fp16"): 4e-3, ("leaky_relu", "bf16"): 9e-2, ("leaky_relu", "fp16"): 6e-2}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["mish", "leaky_relu"])
@pytest.mark.parametrize("i", [i for i, c in enumerate(gi.BLOCK_CONFIGS) if c[4] and c[0] % 32 == 0])
def test_block_train_16bit_vs_golden(yt, golden, i, act, dtype):
    """Train-mode block in bf16 / fp16 storage (what torch.autocast gives the reference, train.py:53):
    BatchNorm(train) output and running stats, dx / dW / dgamma / dbeta against the fp32 reference,
    within the rounding of activations and gradients to the 16-bit format."""
    from yolo_for_turbines_amd import engine
    g = golden("blocks")
    cin, cout, k, s, bn, h = gi.BLOCK_CONFIGS[i]
    blk, x = _block(yt, i, act)
    blk.train()
    tag = f"cfg{i}/{act}"
    xg = x.cuda().requires_grad_(True)
    engine.module_state(blk).compute_dtype = dtype
    try:
        y = blk(xg)
        gy = torch.from_numpy(np.random.Generator(np.random.PCG64(3000 + i)).standard_normal(tuple(y.shape), dtype=np.float32))
        y.backward(gy.cuda())
    finally:
        engine.module_state(blk).compute_dtype = None
    tol = H16_TRAIN_TOL[dtype]

    def close(got, want, what, t=tol):
        scale = max(1e-6, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        assert err <= t * scale, f"{tag} {dtype} {what}: max err {err} vs scale {scale} ({err / scale:.3g})"

    def close_l2(got, want, what):
        # gradients: a 16-bit rounding of z flips LeakyReLU's branch on the few elements with |u| ~ 0 and moves
        # single entries by O(|dy|), so the bar is the relative L2 error, not the max
        err = float(np.linalg.norm(got.astype(np.float64) - want) / (np.linalg.norm(want) + 1e-30))
        assert err <= H16_GRAD_L2[(act, dtype)], f"{tag} {dtype} {what}: relative L2 error {err:.3g}"
    close(y.detach().cpu().reshape(-1)[::gi.BLOCK_STRIDE].numpy(), g[f"{tag}/train"], "y")
    close(blk.batch_norm.running_mean.cpu().numpy(), g[f"{tag}/new_mean"], "running_mean", 1e-2)
    close(blk.batch_norm.running_var.cpu().numpy(), g[f"{tag}/new_var"], "running_var", 1e-2)
    close_l2(xg.grad.cpu().reshape(-1)[::gi.BLOCK_STRIDE].numpy(), g[f"{tag}/dx"], "dx")
    close_l2(blk.conv.weight.grad.cpu().reshape(-1)[::gi.BLOCK_DW_STRIDE].numpy(), g[f"{tag}/dw"], "dw")
    close_l2(blk.batch_norm.weight.grad.cpu().numpy(), g[f"{tag}/dgamma"], "dgamma")
    close_l2(blk.batch_norm.bias.grad.cpu().numpy(), g[f"{tag}/dbeta"], "dbeta")


@pytest.mark.parametrize("dtype,cos_min,norm_tol", [("fp16", 0.995, 0.03), ("bf16", 0.95, 0.12)])
def test_network_train_step_16bit_vs_golden(yt, golden, dtype, cos_min, norm_tol):
    """One fine-tune step under torch.autocast (the reference's train.py:53 context) on the 16-bit kernels,
    Mish network (smooth, see test_network_train_step_vs_golden): loss parts and the direction / size of
    every parameter gradient against the fp32 reference."""
    g = golden("train_step")
    tag = "mish"
    c = gi.TRAIN_CASE
    sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=c["nc"], activation="mish")
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = onet.synth_input(c["xseed"], c["batch"], c["size"]).cuda()
    tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(c["batch"], c["size"], c["nc"], c["anchors"], c["tseed"])]
    grids = [c["size"] // 32, c["size"] // 16, c["size"] // 8]
    sa = (torch.tensor(c["anchors"]) * torch.tensor(grids).view(3, 1, 1)).cuda()
    lf = yt.YOLOLoss()
    ac_dtype = torch.float16 if dtype == "fp16" else torch.bfloat16
    with torch.autocast("cuda", dtype=ac_dtype):                   # loss inside the autocast block, as train.py:53-65 has it
        preds = m(x)
        assert all(p.dtype == ac_dtype for p in preds)             # what the reference's forward returns under autocast
        parts = torch.stack([torch.stack([t.float() for t in lf(preds[i], tg[i].clone(), sa[i])]) for i in range(3)])
    np.testing.assert_allclose(parts.detach().cpu().numpy(), g[f"{tag}/loss_parts"], rtol=norm_tol, atol=1e-3)
    parts.sum().backward()
    named = dict(m.named_parameters())
    worst_cos, worst_key = 1.0, None
    for key in [k[len(tag) + 6:] for k in g.files if k.startswith(f"{tag}/grad/")]:
        got = named[key].grad.cpu()
        want = g[f"{tag}/grad/{key}"]
        got = got.reshape(-1)[::gi.TRAIN_GRAD_STRIDE].numpy() if got.numel() > 4096 else got.numpy()
        if np.abs(want).max() < 1e-12:
            continue
        cos = float((got.astype(np.float64) * want).sum() / (np.linalg.norm(got.astype(np.float64)) * np.linalg.norm(want) + 1e-30))
        if cos < worst_cos:
            worst_cos, worst_key = cos, key
    assert worst_cos >= cos_min, f"{dtype}: gradient direction of {worst_key}: cos {worst_cos}"
    norms = np.array([float(p.grad.double().norm()) for p in m.parameters()])
    ref = g[f"{tag}/gradnorm_all"]
    big = ref > 1e-3 * ref.max()
    ratio = norms[big] / ref[big]
    assert np.all(np.abs(ratio - 1) <= norm_tol), f"{dtype}: gradient-norm ratio range {ratio.min():.3f} .. {ratio.max():.3f}"
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_transposing_lds_read_semantics(yt):
    """The 16-bit wgrad kernel stages [pixel][channel] tiles and reads them channel-major with gfx950's
    ds_read_b64_tr_b16; pin the lane mapping it relies on: lane l, element e <- image[8*(l/32) + e][l % 32]."""
    from yolo_for_turbines_amd import _lib as L
    for ld in (32, 96, 128):
        img = torch.arange(64 * ld, dtype=torch.int16, device="cuda")
        out = torch.zeros(64 * 8, dtype=torch.int16, device="cuda")
        L.check(L.lib().yolo_debug_tr_probe(img.data_ptr(), out.data_ptr(), ld, L.current_stream()))
        got = out.cpu().numpy().reshape(64, 8)
        lane = np.arange(64)[:, None]
        e = np.arange(8)[None, :]
        np.testing.assert_array_equal(got, ((8 * (lane // 32) + e) * ld + lane % 32).astype(np.int16))


# ------------------------------------------------------------- fused loss kernels (loss.py:29-81)
@pytest.mark.parametrize("nc,S,B", [(2, 96, 4), (80, 64, 2), (2, 416, 2)])
def test_fused_loss_values_and_gradients_vs_oracle(yt, nc, S, B):
    """FusedYOLOLoss (3 HIP kernels per scale) against the oracle restatement of the reference loss under
    CPU autograd: the four weighted parts per scale and dL/dpred for every scale."""
    from oracle import loss as oloss
    anchors = gi.TRAIN_CASE["anchors"]
    tg = [torch.from_numpy(t) for t in gi.synth_targets(B, S, nc, anchors, 77)]
    grids = [S // 32, S // 16, S // 8]
    sa = torch.tensor(anchors) * torch.tensor(grids).view(3, 1, 1)
    rng = np.random.Generator(np.random.PCG64(5))
    fl = yt.FusedYOLOLoss()
    for i, g in enumerate(grids):
        p_cpu = torch.from_numpy(rng.standard_normal((B, 3, g, g, 5 + nc), dtype=np.float32)).requires_grad_(True)
        w = torch.tensor([1.0, 0.7, 1.3, 0.9])
        ref = torch.stack(oloss.yolo_loss(p_cpu * 1.0, tg[i].clone(), sa[i]))
        (ref * w).sum().backward()
        p_gpu = p_cpu.detach().cuda().requires_grad_(True)
        t_gpu = tg[i].clone().cuda()
        t_before = t_gpu.clone()
        got = torch.stack(fl(p_gpu, t_gpu, sa[i].cuda()))
        (got * w.cuda()).sum().backward()
        np.testing.assert_allclose(got.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=1e-7)
        gref = p_cpu.grad
        err = float((p_gpu.grad.cpu() - gref).abs().max() / gref.abs().max())
        assert err < 2e-5, f"scale {i}: grad rel err {err}"
        assert torch.equal(t_gpu, t_before) and torch.equal(p_gpu.detach().cpu(), p_cpu.detach())     # no side effects


def test_fused_loss_reference_view_and_empty_object_set(yt):
    """The reference's permuted prediction view (non-contiguous strides) and a batch without any object."""
    from oracle import loss as oloss
    nc, g, B = 3, 7, 2
    rng = np.random.Generator(np.random.PCG64(9))
    raw = torch.from_numpy(rng.standard_normal((B, 3, 5 + nc, g, g), dtype=np.float32))
    view_cpu = raw.permute(0, 1, 3, 4, 2)
    t = torch.zeros((B, 3, g, g, 6))
    t[0, 1, 2, 3] = torch.tensor([0.4, 0.6, 1.5, 2.0, 1.0, 2.0])
    t[1, 0, 5, 5, 4] = -1.0
    anc = torch.tensor([[1.0, 2.0], [2.5, 1.5], [4.0, 3.0]])
    fl = yt.FusedYOLOLoss()
    for tt in (t, torch.zeros_like(t)):
        ref = torch.stack([torch.as_tensor(v) for v in oloss.yolo_loss(view_cpu.clone(), tt.clone(), anc)])
        got = torch.stack(fl(raw.cuda().permute(0, 1, 3, 4, 2), tt.cuda(), anc.cuda()))
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=1e-7)


def test_plan_cache_is_bounded_across_sizes(yt):
    """Multi-scale training (train.py:45-46) visits many input sizes; each training plan owns all activations of its
    size, so the engine keeps only the most recently used ones (and rebuilding a dropped plan gives the same result)."""
    nc = 2
    sd = onet.synth_state_dict(61, 3, nc, gain=gi.NET_GAIN)
    m = yt.YOLOv3(num_classes=nc)
    m.load_state_dict(sd)
    m = m.cuda().train()
    lf = yt.FusedYOLOLoss()
    anchors = gi.TRAIN_CASE["anchors"]
    first = None
    for S in (64, 96, 128, 160, 64):
        x = onet.synth_input(S, 2, S).cuda()
        tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(2, S, nc, anchors, 5)]
        sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).cuda()
        m.zero_grad(set_to_none=True)
        preds = m(x)
        loss = sum(sum(lf(preds[i], tg[i], sa[i])) for i in range(3))
        loss.backward()
        if S == 64:
            gnorm = float(m.layers[0].conv.weight.grad.double().norm())
            if first is None:
                first = (float(loss), gnorm)
            else:
                assert abs(float(loss) - first[0]) <= 1e-4 * abs(first[0]) + 1e-5     # running stats moved; forward uses batch stats
                assert abs(gnorm - first[1]) <= 1e-3 * first[1]
        n_train = sum(1 for k in m._engine._plans if k[0] == "train")
        assert n_train <= m._engine.max_train_plans
    m.eval()
    with torch.no_grad():
        for S in (32, 64, 96, 128, 160, 192):
            m(onet.synth_input(S, 1, S).cuda())
    assert sum(1 for k in m._engine._plans if k[0] == "eval") <= m._engine.max_eval_plans


# ------------------------------------------------------------- batched target builder (dataset.py:119-161)
@pytest.mark.parametrize("case", list(gi.TARGET_CASES))
def test_build_targets_bit_exact_vs_reference(yt, golden, case):
    """yolo_build_targets for a whole batch against what the reference's YOLODataset.__getitem__ built per image
    (goldens generated by running that code): every element identical, including the empty image, overwritten
    'free-looking' cells (x offset 0) and the ignore (-1) marks."""
    g = golden("targets")
    c = gi.TARGET_CASES[case]
    boxes = gi.target_boxes(case)
    outs = yt.build_targets(boxes, c["anchors"], c["size"])
    grids = [c["size"] // 32, c["size"] // 16, c["size"] // 8]
    for s_i, (o, gg) in enumerate(zip(outs, grids)):
        assert tuple(o.shape) == (len(boxes), 3, gg, gg, 6) and o.dtype == torch.float32
        want = np.stack([g[f"{case}/img{b}/scale{s_i}"] for b in range(len(boxes))])
        np.testing.assert_array_equal(o.cpu().numpy(), want)
    # padded-tensor entry point gives the same tensors
    mb = max(len(b) for b in boxes)
    pad = torch.zeros((len(boxes), mb + 3, 5))
    for i, bl in enumerate(boxes):
        if bl:
            pad[i, :len(bl)] = torch.tensor(bl)
    outs2 = yt.build_targets(pad.cuda(), c["anchors"], c["size"], counts=[len(b) for b in boxes])
    for a, b2 in zip(outs, outs2):
        assert torch.equal(a, b2)


# ------------------------------------------------------------- mAP on the device (utils.py:193-274)
@pytest.mark.parametrize("case", list(gi.MAP_CASES))
def test_map_vs_reference(yt, golden, case):
    """calc_mAP (two stable sorts + matching and AP kernels) against the value the reference's own calc_mAP returned
    for the same seeded detections / ground truths, at IoU 0.5 and 0.75; plus the reference's known-answer test."""
    g = golden("kat")
    pb, tb = gi.map_boxes(case)
    nc = gi.MAP_CASES[case]["nc"]
    for thr, key in ((0.5, f"map_{case}"), (0.75, f"map_{case}_iou75")):
        got = yt.calc_mAP(pb, tb, thr, "center", nc)
        assert got.dim() == 0 and got.dtype == torch.float32
        assert abs(float(got) - float(g[key])) <= 2e-6, f"{case} @{thr}: {float(got)} vs {float(g[key])}"


@pytest.mark.parametrize("n", [1, 5, 2048, 2049, 40000, 262144])
def test_sort_u64_and_stable_two_level_order(yt, n):
    """yolo_sort_u64 (chunk sort + rank merge as a stand-alone entry point) against torch.sort on unique keys, and the
    two-level stable order calc_mAP builds on it against Python's own two stable list sorts (utils.py:206,232) with many ties,
    negative zeros and negative scores."""
    from yolo_for_turbines_amd import _lib as L
    from yolo_for_turbines_amd.metrics import _stable_order
    g = torch.Generator().manual_seed(n)
    keys = (torch.randint(0, 2 ** 62, (n,), generator=g, dtype=torch.int64) & ~0xfffff) | torch.arange(n, dtype=torch.int64)
    kd = keys.cuda()
    out = torch.empty_like(kd)
    lib = L.lib()
    ws = torch.empty(lib.yolo_sort_u64_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    L.check(lib.yolo_sort_u64(kd.data_ptr(), out.data_ptr(), n, ws.data_ptr(), ws.numel(), L.current_stream()))
    assert torch.equal(out.cpu(), torch.sort(keys).values)
    m = min(n, 5000)
    major = torch.randint(0, 7, (m,), generator=g).float()
    minor = (torch.randint(-8, 8, (m,), generator=g).float() / 4.0)
    minor[::7] = -0.0
    for desc in (True, False):
        got = _stable_order(major.cuda(), minor.cuda(), desc).cpu().tolist()
        rows = list(range(m))
        rows.sort(key=lambda i: float(minor[i]), reverse=desc)        # list.sort is stable, also with reverse=True
        rows.sort(key=lambda i: float(major[i]))
        assert got == rows


def test_map_known_answers(yt, golden):
    pb = [[0, 0.5, 0.5, 0.25, 0.25, 0.9, 0], [0, 0.5, 0.5, 0.1, 0.1, 0.6, 0]]
    assert abs(float(yt.calc_mAP(pb, [r[:] for r in pb])) - float(golden("kat")["map_identical"])) <= 1e-6   # utils_test.py:22-32
    with pytest.raises(ZeroDivisionError):
        yt.calc_mAP(pb, [], num_classes=3)
    # a big evaluation set: 128 images x ~80 kept boxes, must agree with the oracle restatement
    from oracle import metrics as om
    rng = np.random.Generator(np.random.PCG64(77))
    preds, trues = [], []
    for img in range(24):
        for _ in range(6):
            cls = int(rng.integers(0, 5))
            b = [float(np.float32(v)) for v in (*rng.uniform(0.2, 0.8, 2), *rng.uniform(0.05, 0.3, 2))]
            trues.append([img, *b, 1.0, cls])
            for _ in range(3):
                preds.append([img, *[float(np.float32(v + 0.02 * rng.standard_normal())) for v in b], float(np.float32(rng.uniform(0.2, 1))), cls])
    assert abs(float(yt.calc_mAP(preds, trues, 0.5, "center", 5)) - float(om.calc_map(preds, trues, 0.5, "center", 5))) <= 2e-6


# ------------------------------------------------------------- whole-step HIP graph
@pytest.mark.parametrize("ac", [None, torch.bfloat16])
def test_graphed_train_step_equals_eager_steps(yt, ac):
    """GraphedTrainStep (forward + 3 fused losses + backward + SGD captured as one HIP graph) must walk the same
    parameter trajectory as the same steps issued eagerly: every kernel is deterministic, so after warm-up (3 steps)
    + 2 replays the weights are compared bit for bit with 5 eager steps on the same batches."""
    nc, S, B = 2, 96, 2
    anchors = gi.TRAIN_CASE["anchors"]
    sd = onet.synth_state_dict(71, 3, nc, gain=gi.NET_GAIN)
    sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).cuda()
    batches = [(onet.synth_input(80 + k, B, S).cuda(), [torch.from_numpy(t).cuda() for t in gi.synth_targets(B, S, nc, anchors, 90 + k)])
               for k in range(3)]

    def make():
        m = yt.YOLOv3(num_classes=nc, activation="mish")
        m.load_state_dict(sd)
        m = m.cuda().train()
        return m, torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    # eager: warm-up uses batch 0 three times, then batches 1 and 2
    m1, o1 = make()
    lf = yt.FusedYOLOLoss()
    seq = [batches[0]] * 3 + [batches[1], batches[2]]
    eager_losses = []
    for x, tg in seq:
        o1.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=ac or torch.bfloat16, enabled=ac is not None):
            preds = m1(x)
        loss = sum(sum(lf(preds[i], tg[i], sa[i])) for i in range(3))
        loss.backward()
        o1.step()
        eager_losses.append(float(loss.detach()))
    m2, o2 = make()
    step = yt.GraphedTrainStep(m2, o2, sa, batches[0][0], batches[0][1], autocast_dtype=ac)
    l1 = float(step(*batches[1]))
    l2 = float(step(*batches[2]))
    assert l1 == eager_losses[3] and l2 == eager_losses[4]
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert m2._engine.nan_check is True
    with pytest.raises(ValueError):
        step(torch.zeros(1, 3, S, S, device="cuda"), batches[1][1])


# ------------------------------------------------------------- check_model_accuracy (utils.py:334-381)
def test_check_model_accuracy_vs_reference(yt, golden, capsys):
    """The mirror (one fused counting kernel per scale) against the three accuracies the reference function returned for
    a stub model replaying the same seeded predictions / targets; counts are integers, so the bar is equality."""
    want = golden("kat")["accuracy"]
    batches = gi.accuracy_batches()

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.k = -1

        def forward(self, x):
            self.k += 1
            return [torch.from_numpy(p.copy()).cuda() for p in batches[self.k][2]]
    stub = Stub().cuda().train()
    loader = [(torch.from_numpy(x), [torch.from_numpy(t.copy()) for t in tg]) for x, tg, _ in batches]
    got = yt.check_model_accuracy(stub, loader, gi.ACC_CASE["thr"])
    assert stub.training                                   # restored
    np.testing.assert_array_equal(np.array([float(a) for a in got], np.float32), want)
    assert "Class accuracy is:" in capsys.readouterr().out
    # the reference's permuted prediction view (non-contiguous) gives the same counters
    x, tg, preds = batches[0]
    a = yt.accuracy_counts([torch.from_numpy(p).cuda() for p in preds], [torch.from_numpy(t) for t in tg], 0.6)
    b = yt.accuracy_counts([torch.from_numpy(np.ascontiguousarray(p.transpose(0, 1, 4, 2, 3))).cuda().permute(0, 1, 3, 4, 2) for p in preds],
                           [torch.from_numpy(t) for t in tg], 0.6)
    assert torch.equal(a, b)


# ------------------------------------------------------------- get_eval_boxes (utils.py:276-332)
def test_get_eval_boxes_vs_reference(yt, golden):
    """Whole evaluation path — forward (stub replaying seeded predictions), decode of three scales, per-image NMS, image
    ids, ground-truth extraction from targets[2] — against the two box lists the reference's get_eval_boxes returned:
    same rows in the same order; then calc_mAP of those lists equals the reference's calc_mAP of its lists."""
    g = golden("kat")
    ec = gi.EVAL_CASE
    batches = gi.eval_batches()

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.k = -1

        def forward(self, x):
            self.k += 1
            return [torch.from_numpy(p.copy()).cuda() for p in batches[self.k][2]]
    stub = Stub().cuda()
    loader = [(torch.from_numpy(x), [torch.from_numpy(t.copy()) for t in tg]) for x, tg, _ in batches]
    pb, tb = yt.get_eval_boxes(loader, stub, ec["iou_thr"], ec["anchors"], ec["obj_thr"], "center")
    want_p, want_t = g["eval_pred_boxes"], g["eval_true_boxes"]
    got_p, got_t = np.asarray(pb, np.float64).reshape(-1, 7), np.asarray(tb, np.float64).reshape(-1, 7)
    assert got_p.shape == want_p.shape and got_t.shape == want_t.shape
    np.testing.assert_array_equal(got_p[:, [0, 6]], want_p[:, [0, 6]])          # image ids and classes: same rows, same order
    np.testing.assert_allclose(got_p, want_p, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got_t, want_t, rtol=1e-6, atol=1e-7)
    assert abs(float(yt.calc_mAP(pb, tb, 0.5, "center", ec["nc"])) - float(g["eval_map"])) <= 1e-6
    assert stub.training                                                          # utils.py:331 leaves the model in train mode


# ------------------------------------------------------------- RCCL path with one rank
def test_bench_runs_over_rccl_with_one_rank(tmp_path):
    """The multi-GPU path (process group over RCCL, bucketed asynchronous gradient all-reduce inside backward,
    barrier + max-over-ranks timing) exercised end to end with a 1-rank group in a child process; the 8-GPU run is
    the driver's. Checks the one-JSON-line contract and that the data-parallel fine-tune leg produced numbers."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, YOLO_FORCE_DIST="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29653", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--size", "160", "--full", "--train-steps", "2", "--no-cpu-baseline", "--no-nms", "--no-config5", "--no-config3"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["train"]["value"] > 0 and d["train"]["bf16_autocast"]["value"] > 0


@pytest.mark.gpu
def test_round3_kernels_agree_with_round2_paths():
    """The same seeded bf16 fine-tune steps (Mish: smooth, so rounding differences stay small) in two child processes: every
    round-3 kernel path on (default), and all of them switched off through their A/B environment switches (weight gradient on
    LDS-DMA, stem weight gradient, gathered-row stride-2 forward / fused stride-2 input gradient, conv3_ws_h16, epilogue
    BatchNorm statistics forward and backward, launch tables). Losses, loss parts, running statistics and the gradients of the
    layers those kernels compute must agree to 16-bit rounding."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    off = dict(YOLO_NO_WGRAD_DMA="1", YOLO_NO_STEM_WGRAD="1", YOLO_NO_S2_DMA="1", YOLO_NO_S2G="1", YOLO_NO_CONV3_WS="1",
               YOLO_BN_FUSED_STATS="0", YOLO_BN_FUSED_BSTATS="0", YOLO_TRAIN_TAPE="0")
    res = []
    for extra in ({}, off, {"AB_FP32": "1"}):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "workers", "ab_step.py")], env=dict(os.environ, **extra), capture_output=True,
                           text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    a, b, f = res
    # Two bf16 evaluations of a 75-layer network that round in different places differ by a few 1e-3 on the loss and by several
    # per cent on loss parts that average a handful of cells; a wrong tap or a missing term is O(1). The yardstick is the fp32
    # run of the same steps: the round-3 paths may not be further from it than round 2's paths (beyond noise), and the two 16-bit
    # runs may not be further apart than their distance to fp32.
    def dist(u, v):
        return np.abs(np.asarray(u, dtype=np.float64) - np.asarray(v, dtype=np.float64))
    for k in ("loss0", "loss1"):
        da, db = abs(a[k] - f[k]), abs(b[k] - f[k])
        assert da <= 1.5 * db + 2e-3 * abs(f[k]), (k, a[k], b[k], f[k])
        assert abs(a[k] - b[k]) <= 1e-2 * abs(f[k]), (k, a[k], b[k], f[k])
    pa, pb = dist(a["parts0"], f["parts0"]), dist(b["parts0"], f["parts0"])
    assert float(pa.sum()) <= 1.5 * float(pb.sum()) + 2e-3 * float(np.sum(f["parts0"])), (a["parts0"], b["parts0"], f["parts0"])
    np.testing.assert_allclose(a["rm0"], b["rm0"], rtol=1e-3, atol=1e-5)
    for n, gf in f["grads"].items():
        ga, gb = a["grads"][n], b["grads"][n]
        da, db = abs(ga["norm"] - gf["norm"]), abs(gb["norm"] - gf["norm"])
        assert da <= 1.5 * db + 2e-2 * gf["norm"], (n, ga["norm"], gb["norm"], gf["norm"])
        ha, hb = dist(ga["head"], gf["head"]).max(), dist(gb["head"], gf["head"]).max()
        assert ha <= 1.5 * hb + 0.05 * (np.abs(gf["head"]).max() + 1e-12) + 1e-3 * gf["norm"], (n, ga["head"], gb["head"], gf["head"])


def test_train_mode_single_value_per_channel_is_rejected(yt):
    """nn.BatchNorm2d refuses batch statistics over one value (B = 1 at S = 32 leaves a 1x1 map): same ValueError."""
    m = yt.YOLOv3(num_classes=2).cuda().train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(torch.rand(1, 3, 32, 32, device="cuda"))


@pytest.mark.parametrize("S,B,nc", [(96, 5, 3), (224, 1, 2)])
def test_network_train_step_odd_shapes_vs_oracle(yt, S, B, nc):
    """Odd batch sizes / a single image / a non-square-of-two grid through the whole fp32 train step (fused loss):
    every parameter gradient within 2e-4 relative L2 of the oracle under CPU autograd."""
    from oracle import loss as oloss
    anchors = gi.TRAIN_CASE["anchors"]
    sd = onet.synth_state_dict(5, 3, nc, gain=gi.NET_GAIN)
    x = onet.synth_input(S + B, B, S)
    tg = [torch.from_numpy(t) for t in gi.synth_targets(B, S, nc, anchors, 3)]
    sa = torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)
    par = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    full = dict(sd)
    full.update(par)
    pr = onet.forward(full, x, nc, "mish", training=True, new_stats={})
    sum(sum(oloss.yolo_loss(pr[i], tg[i].clone(), sa[i])) for i in range(3)).backward()
    m = yt.YOLOv3(num_classes=nc, activation="mish")
    m.load_state_dict(sd)
    m = m.cuda().train()
    lf = yt.FusedYOLOLoss()
    po = m(x.cuda())
    sum(sum(lf(po[i], tg[i].cuda(), sa[i].cuda())) for i in range(3)).backward()
    for k, p in m.named_parameters():
        g, r = p.grad.cpu().double().reshape(-1), par[k].grad.double().reshape(-1)
        if float(r.norm()) > 1e-12:
            assert float((g - r).norm() / r.norm()) < 2e-4, k


# ------------------------------------------------------------- letterbox (config.py:101-113) — parity UNPINNED
@pytest.mark.parametrize("h,w,size", [(480, 640, 416), (375, 500, 416), (1080, 1920, 608), (416, 416, 416), (200, 333, 416), (900, 37, 96)])
def test_letterbox_vs_restatement(yt, h, w, size):
    """Device letterbox against oracle/preprocess.py (a restatement of OpenCV's uint8 INTER_LINEAR and albumentations'
    size / padding rules; cv2 itself is not installed here, so parity with the reference transform is unpinned):
    bit-exact output, same geometry; up- and down-scaling, no-op size, extreme aspect ratio."""
    from oracle import preprocess as opre
    rng = np.random.Generator(np.random.PCG64(h * 7 + w))
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    want, meta_w = opre.letterbox(img, size)
    got, meta = yt.letterbox([img], size)
    assert tuple(got.shape) == (1, 3, size, size) and got.dtype == torch.float32
    assert tuple(meta[0]) == tuple(meta_w)
    np.testing.assert_array_equal(got[0].cpu().numpy(), want)
    boxes = [[0.5, 0.5, 0.2, 0.3, 0.9, 1.0], [0.1, 0.8, 0.05, 0.1, 0.7, 0.0]]
    assert yt.unletterbox_boxes(boxes, (h, w), (size, size)) == opre.unletterbox_boxes(boxes, (h, w), (size, size))


@pytest.mark.parametrize("ac", [None, torch.bfloat16])
def test_frozen_backbone_train_step(yt, ac):
    """`freeze=True` (model.py:306-309): parameters of the first 9 top-level modules do not require grad. Their .grad
    stays None, the trainable rest gets exactly the gradients of the unfrozen step (the backward simply stops at the
    first trainable block), in fp32 and under bf16 autocast."""
    nc, S, B = 2, 96, 2
    anchors = gi.TRAIN_CASE["anchors"]
    sd = onet.synth_state_dict(81, 3, nc, gain=gi.NET_GAIN)
    x = onet.synth_input(82, B, S).cuda()
    tg = [torch.from_numpy(t).cuda() for t in gi.synth_targets(B, S, nc, anchors, 83)]
    sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).cuda()
    lf = yt.FusedYOLOLoss()
    grads = []
    for frozen in (False, True):
        m = yt.YOLOv3(num_classes=nc, activation="mish")
        m.load_state_dict(sd)
        m = m.cuda().train()
        if frozen:
            for layer in list(m.layers)[:9]:
                for p in layer.parameters():
                    p.requires_grad_(False)
        with torch.autocast("cuda", dtype=ac or torch.bfloat16, enabled=ac is not None):
            po = m(x)
        sum(sum(lf(po[i], tg[i], sa[i])) for i in range(3)).backward()
        grads.append({k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()})
    full, part = grads
    n_frozen = 0
    for k, g in part.items():
        idx = int(k.split(".")[1])
        if idx < 9:
            assert g is None, k
            n_frozen += 1
        else:
            assert g is not None and torch.equal(g, full[k]), k
    assert n_frozen > 50


@pytest.mark.parametrize("loss_name", ["YOLOLoss", "FusedYOLOLoss"])
def test_reference_training_loop_runs_unchanged(yt, loss_name):
    """The body of train_one_epoch (train.py:41-82) verbatim on this package's drop-in classes: default CUDA autocast
    (fp16 kernels), loss inside the autocast block, GradScaler scale / step / update, LinearLR warm-up, and a change of
    input size in the middle (train.py:45-46). The loss must stay finite, the scaler must take real steps and the
    weights must move."""
    nc = 2
    anchors = gi.TRAIN_CASE["anchors"]
    sd = onet.synth_state_dict(91, 3, nc, gain=gi.NET_GAIN)
    model = yt.YOLOv3(num_classes=nc)
    model.load_state_dict(sd)
    model = model.cuda().train()
    optimizer = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    warmup_scheduler = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=0.1, total_iters=4)
    loss_fn = getattr(yt, loss_name)()
    grad_scaler = torch.amp.GradScaler()
    w_before = model.layers[0].conv.weight.detach().clone()
    losses = []
    for batch_idx, S in enumerate([96, 96, 128, 128]):
        grids = [S // 32, S // 16, S // 8]
        scaled_anchors = (torch.tensor(anchors) * torch.tensor(grids).view(3, 1, 1)).cuda()
        x = onet.synth_input(100 + batch_idx, 2, S)
        y = [torch.from_numpy(t) for t in gi.synth_targets(2, S, nc, anchors, 110 + batch_idx)]
        optimizer.zero_grad()
        x = x.to("cuda")
        y0, y1, y2 = (y[0].to("cuda"), y[1].to("cuda"), y[2].to("cuda"))
        with torch.amp.autocast(device_type="cuda"):
            out = model(x)
            box_loss_0, obj_loss_0, no_obj_loss_0, class_loss_0 = loss_fn(out[0], y0, scaled_anchors[0])
            box_loss_1, obj_loss_1, no_obj_loss_1, class_loss_1 = loss_fn(out[1], y1, scaled_anchors[1])
            box_loss_2, obj_loss_2, no_obj_loss_2, class_loss_2 = loss_fn(out[2], y2, scaled_anchors[2])
            box_loss = box_loss_0 + box_loss_1 + box_loss_2
            obj_loss = obj_loss_0 + obj_loss_1 + obj_loss_2
            no_obj_loss = no_obj_loss_0 + no_obj_loss_1 + no_obj_loss_2
            class_loss = class_loss_0 + class_loss_1 + class_loss_2
            loss = box_loss + obj_loss + no_obj_loss + class_loss
        grad_scaler.scale(loss).backward()
        grad_scaler.step(optimizer)
        grad_scaler.update()
        warmup_scheduler.step()
        losses.append(loss.item())
    assert all(np.isfinite(l) for l in losses), losses
    assert not torch.equal(model.layers[0].conv.weight.detach(), w_before)
    assert grad_scaler.get_scale() >= 65536.0 / 4          # at most a couple of skipped (overflow) steps
    assert all(torch.isfinite(p).all() for p in model.parameters())


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_two_rank_data_parallel_on_gpu(tmp_path, mode):
    """Data-parallel fine-tune step with TWO ranks (both on cuda:0, gradient exchange over gloo because RCCL does not
    accept two ranks on one device): the bucketed, overlapped all-reduce must leave every rank with the arithmetic mean
    of the two shards' gradients (SURVEY 8e parity definition), identical on both ranks."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for rank in range(2):
        env = dict(os.environ, WORLD_SIZE="2", RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29671",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "dp_worker.py"), str(tmp_path), mode], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=root))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    r0 = json.load(open(tmp_path / "rank0.json"))
    r1 = json.load(open(tmp_path / "rank1.json"))
    assert r0["norms"] == r1["norms"]                                   # same averaged gradients on both ranks
    assert r0["worst_rel_err_vs_mean_of_shards"] < (1e-5 if mode == "fp32" else 1e-5)
    # later steps of the same process group: p.grad tensors kept alive by zero_grad(set_to_none=False) (they alias the
    # buckets) must come out as 1x the mean, not 2x; a third backward without zero_grad accumulates on top; freezing /
    # unfreezing parameters rebuilds the buckets so that every trainable gradient is still exchanged
    assert r0["norms_again"] == r1["norms_again"]
    for k, v in r0["worst"].items():
        assert v < 1e-5, (k, v)
    assert r0["n_frozen_without_grad"] > 50


def test_checkpoint_round_trip_on_device(yt, tmp_path):
    """save_checkpoint after a real fine-tune step on the GPU, load_checkpoint into a model that has ALREADY run (so its
    packed-weight cache is warm and must be dropped): same forward, same momentum buffers, learning rate forced; a second
    step from the restored state equals the second step of the original."""
    c = gi.NET_CASES["nc2_s128_b1_leaky"]
    x = onet.synth_input(5, 2, 64).cuda()
    tgt = [torch.from_numpy(t).cuda() for t in gi.synth_targets(2, 64, c["nc"], gi.TRAIN_CASE["anchors"], 77)]
    anchors = torch.tensor(gi.TRAIN_CASE["anchors"], dtype=torch.float32).cuda()
    loss_fn = yt.FusedYOLOLoss()

    def step(m, opt):
        m.train()
        opt.zero_grad()
        preds = m(x)
        loss = sum(sum(loss_fn(p, t.clone(), anchors[i] * p.shape[2])) for i, (p, t) in enumerate(zip(preds, tgt)))
        loss.backward()
        opt.step()
        return float(loss.detach())

    m = _model(yt, c)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    step(m, opt)
    yt.save_checkpoint(m, opt, filename=str(tmp_path / "ck.pth"))
    other = dict(c, wseed=c["wseed"] + 1)
    m2 = _model(yt, other)
    with torch.no_grad():
        stale = m2(x)                                           # packs m2's OWN weights
    opt2 = torch.optim.SGD(m2.parameters(), lr=0.7, momentum=0.9, weight_decay=5e-4)
    yt.load_checkpoint(m2, opt2, lr=1e-3, filename="ck.pth", model_folder=str(tmp_path))
    assert all(g["lr"] == 1e-3 for g in opt2.param_groups)
    m.eval(); m2.eval()
    with torch.no_grad():
        a, b = m(x), m2(x)
    for pa, pb, ps in zip(a, b, stale):
        assert torch.equal(pa, pb)
        assert not torch.equal(pb, ps)
    for pa, pb in zip(m.parameters(), m2.parameters()):
        assert torch.equal(opt.state[pa]["momentum_buffer"], opt2.state[pb]["momentum_buffer"])
    l1, l2 = step(m, opt), step(m2, opt2)
    assert l1 == l2
    for pa, pb in zip(m.parameters(), m2.parameters()):
        assert torch.equal(pa, pb)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_batched_weight_pack_equals_per_layer_pack(yt, dtype):
    """yolo_pack_weights_batch (one launch per 48 layers, used after every optimizer step) writes byte-identical buffers to
    the per-layer yolo_pack_weights / yolo_pack_weights_dgrad(flip = 1), for forward and input-gradient layouts, incl.
    a head-like layer whose channel count is padded; more than 48 items exercise the chunking."""
    import ctypes as C
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    code = {"bf16": L.BF16, "fp16": L.F16}[dtype]
    shapes = [(64, 32, 3), (128, 64, 3), (32, 64, 1), (256, 128, 3), (24, 256, 1), (255, 512, 1), (512, 256, 3)] * 8     # 56 items
    gen = torch.Generator().manual_seed(5)
    ws = [torch.randn((co, ci, k, k), generator=gen).cuda() for co, ci, k in shapes]
    st = L.current_stream()
    for dgrad in (0, 1):
        single, batch, items = [], [], []
        for w, (co, ci, k) in zip(ws, shapes):
            n = lib.yolo_packed_dgrad_bytes(co, ci, k, 1, code) if dgrad else lib.yolo_packed_weight_bytes(co, ci, k, code)
            assert n > 0
            a = torch.zeros(n, dtype=torch.uint8, device="cuda")
            b = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            if dgrad:
                L.check(lib.yolo_pack_weights_dgrad(w.data_ptr(), a.data_ptr(), co, ci, k, 1, code, st), "single dgrad pack")
            else:
                L.check(lib.yolo_pack_weights(w.data_ptr(), a.data_ptr(), co, ci, k, code, st), "single pack")
            single.append(a); batch.append(b)
            items.append(L.PackItem(w.data_ptr(), b.data_ptr(), co, ci, k, 0))
        arr = (L.PackItem * len(items))(*items)
        L.check(lib.yolo_pack_weights_batch(C.cast(arr, C.c_void_p), len(items), dgrad, code, st), "batch pack")
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(single, batch)):
            assert torch.equal(a, b), (dgrad, i, shapes[i])


# ------------------------------------------------------------- the LDS-DMA 16-bit kernels at their edges (tile 8 forced)
DMA_CASES = [
    # (B, H, cin, cout, k, residual, act, upsample, x_ld, x_off, y_ld, y_off)
    (2, 13, 128, 128, 1, False, 1, False, 128, 0, 128, 0),     # 1x1, KT = 4: only the peeled last group runs
    (1, 19, 160, 136, 1, False, 2, False, 160, 0, 136, 0),     # KT = 5 (ring wraps once), cout not a multiple of 128, ragged pixel tile
    (3, 26, 384, 256, 1, False, 1, False, 512, 64, 768, 256),  # reads a slice of a concat buffer, writes into one
    (2, 13, 256, 128, 1, False, 1, True, 256, 0, 384, 128),    # the 1x1 in front of nn.Upsample: 2x store into the concat buffer
    (2, 20, 1024, 512, 1, True, 0, False, 1024, 0, 512, 0),    # 32 K steps, identity epilogue + residual = the 1x1 input gradient
    (2, 13, 128, 256, 3, True, 1, False, 128, 0, 256, 0),      # 3x3 residual block tail
    (1, 19, 96, 128, 3, False, 2, False, 96, 0, 128, 0),       # three 32-channel chunks (odd), odd grid width
    (2, 26, 64, 136, 3, False, 0, False, 64, 0, 136, 0),       # two chunks, cout not a multiple of 128
    (5, 7, 256, 128, 3, False, 1, True, 256, 0, 128, 0),       # tiles straddle images, 2x upsampling store
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", DMA_CASES)
def test_dma_conv_kernels_edge_shapes(yt, case, dtype):
    """conv3_dma_h16 / conv1_dma_h16 called through the C-ABI with `tile = 8` on the shapes their index math can get wrong
    (ring wrap-around, peeled last group, ragged tiles, image-straddling tiles, channel counts that are not tile multiples,
    ld / off views of concat buffers, the 2x-upsampling store, residual accumulate). Reference: fp64 convolution of the SAME
    rounded operands on the CPU, so the only error left is fp32 accumulation order + the final rounding."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, cin, cout, k, residual, act, upsample, x_ld, x_off, y_ld, y_off = case
    code, tdt, tol = {"bf16": (L.BF16, torch.bfloat16, 1e-2), "fp16": (L.F16, torch.float16, 2e-3)}[dtype]
    g = torch.Generator().manual_seed(1000 + 7 * cin + cout + k)
    lib, dev = L.lib(), torch.device("cuda:0")
    x = torch.randn((B, H, H, x_ld), generator=g).to(tdt)
    w = (torch.randn((cout, cin, k, k), generator=g) * (1.0 / (cin * k * k)) ** 0.5)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    Ho = 2 * H if upsample else H
    y0 = torch.randn((B, Ho, Ho, y_ld), generator=g).to(tdt)                    # what is NOT written must survive
    r = torch.randn((B, H, H, cout), generator=g).to(tdt) if residual else None
    xd, yd, sd, shd = x.to(dev), y0.clone().to(dev), scale.to(dev), shift.to(dev)
    rd = r.to(dev) if residual else None
    wd = w.to(dev)
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, k, code), dtype=torch.uint8, device=dev)
    st = L.current_stream()
    L.check(lib.yolo_pack_weights(wd.data_ptr(), wp.data_ptr(), cout, cin, k, code, st))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.ConvDesc(n=B, h=H, w=H, cin=cin, cout=cout, ksize=k, stride=1, x_ld=x_ld, x_off=x_off, y_ld=y_ld, y_off=y_off, r_ld=cout, r_off=0,
                   act=act, out_mode=L.OUT_UPSAMPLE2X if upsample else L.OUT_NHWC, dtype=code,
                   flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK, tile=8)
    L.check(lib.yolo_conv_fwd(d, xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                              yd.data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    xin = x[..., x_off:x_off + cin].double().permute(0, 3, 1, 2)
    ref = F.conv2d(xin, w.to(tdt).double(), stride=1, padding=k // 2)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1) if act == 1 else (F.mish(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + r.double()
    if upsample:
        ref = ref.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    got = yd.cpu()
    err = float((got[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max())
    assert err <= tol, err
    keep = torch.ones(y_ld, dtype=torch.bool)
    keep[y_off:y_off + cout] = False
    assert torch.equal(got[..., keep], y0[..., keep])                           # neighbouring channels of the buffer untouched

RS_CASES = [
    # (B, H, cin, cout, residual, act, upsample, x_ld, x_off, y_ld, y_off): conv1_rs_f32 (fp32 1x1, weights in registers)
    (2, 13, 256, 128, False, 1, False, 256, 0, 128, 0),        # 338 pixels: 11 tiles, the last one ragged; every workgroup gets <= 1 tile
    (1, 52, 256, 128, False, 2, False, 256, 0, 128, 0),        # 85 tiles over 85 workgroups... one tile each, Mish
    (8, 52, 256, 128, False, 1, False, 256, 0, 128, 0),        # 676 tiles on 256 workgroups: the ring wraps, 2-3 tiles per workgroup
    (16, 52, 256, 128, True, 1, False, 256, 0, 128, 0),        # 1352 tiles: the size from which the heuristic picks this kernel
    (3, 26, 384, 128, False, 1, False, 512, 64, 768, 256),     # K = 384: reads a slice of a concat buffer, writes into one
    (4, 26, 512, 256, True, 0, False, 512, 0, 256, 0),         # K = 512 (2-slot ring), two channel groups, identity epilogue + residual
    (2, 13, 256, 128, False, 1, True, 256, 0, 384, 128),       # the 1x1 in front of nn.Upsample: 2x store into the concat buffer
    (5, 26, 512, 384, False, 1, False, 512, 0, 384, 0),        # three channel groups: 85 workgroups per group
]


@pytest.mark.parametrize("case", RS_CASES)
def test_fp32_1x1_register_stationary_kernel(yt, case):
    """conv1_rs_f32 through the C-ABI with `tile = 12` (and the default tile, which must pick it): ragged last tile, several tiles
    per persistent workgroup, K = 256 / 384 / 512, channel groups, ld / off views of concat buffers, the 2x-upsampling store,
    residual accumulate, every activation. Reference: fp64 convolution of the same operands (tolerance = fp32 accumulation)."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, cin, cout, residual, act, upsample, x_ld, x_off, y_ld, y_off = case
    g = torch.Generator().manual_seed(500 + cin + cout + H + B)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = torch.randn((B, H, H, x_ld), generator=g)
    w = torch.randn((cout, cin, 1, 1), generator=g) * (1.0 / cin) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    Ho = 2 * H if upsample else H
    y0 = torch.randn((B, Ho, Ho, y_ld), generator=g)
    r = torch.randn((B, H, H, cout), generator=g) if residual else None
    xd, sd, shd, wd = x.to(dev), scale.to(dev), shift.to(dev), w.to(dev)
    rd = r.to(dev) if residual else None
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 1, L.F32), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(wd.data_ptr(), wp.data_ptr(), cout, cin, 1, L.F32, st))
    xin = x[..., x_off:x_off + cin].double().permute(0, 3, 1, 2)
    ref = F.conv2d(xin, w.double()) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1) if act == 1 else (F.mish(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + r.double()
    if upsample:
        ref = ref.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    outs = []
    for tile in (12, 0, 4):                                      # explicit, heuristic (must be the same kernel), round 2's kernel
        yd = y0.clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        d = L.ConvDesc(n=B, h=H, w=H, cin=cin, cout=cout, ksize=1, stride=1, x_ld=x_ld, x_off=x_off, y_ld=y_ld, y_off=y_off, r_ld=cout,
                       r_off=0, act=act, out_mode=L.OUT_UPSAMPLE2X if upsample else L.OUT_NHWC, dtype=L.F32,
                       flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK, tile=tile)
        L.check(lib.yolo_conv_fwd(d, xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                  yd.data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        got = yd.cpu()
        err = float((got[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max())
        assert err <= 2e-6, (tile, err)
        keep = torch.ones(y_ld, dtype=torch.bool)
        keep[y_off:y_off + cout] = False
        assert torch.equal(got[..., keep], y0[..., keep])           # neighbouring channels of the buffer untouched
        outs.append(got)
    # tile 0 = the heuristic: this kernel from ~4 tiles per persistent workgroup on, the register-staged one below that
    # the default tile's choice depends on the feature map and K only - never on the batch (an image's bits may not depend on its neighbours)
    assert torch.equal(outs[1], outs[0] if (H * H >= 2048 and cin <= 384 and not residual) else outs[2])
    # a NaN in the input reaches the flag
    xn = xd.clone()
    xn[0, 0, 0, x_off] = float("nan")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d.tile = 12
    L.check(lib.yolo_conv_fwd(d, xn.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                              yd.data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
    torch.cuda.synchronize()
    assert int(flag.item()) & 2


WINO_CASES = [
    # (B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off): conv_wino_f32 (fp32 3x3 stride 1, Winograd F(2x2, 3x3))
    (2, 10, 10, 128, 256, True, 1, 128, 0, 256, 0, 256, 0),        # 50 tiles: one ragged tile block, four channel blocks, 32 stages
    (2, 13, 13, 512, 1024, False, 1, 512, 0, 1024, 0, 0, 0),       # odd size: the last tile row / column writes one pixel; 128 stages
    (3, 9, 7, 256, 512, True, 2, 256, 0, 512, 0, 512, 0),          # H != W, both odd, Mish + residual; 60 tiles
    (1, 26, 26, 256, 128, False, 0, 384, 128, 384, 256, 0, 0),     # reads a slice of a concat buffer, writes into one; identity epilogue
    (2, 6, 8, 128, 84, True, 1, 128, 0, 84, 0, 96, 8),             # cout not a multiple of 64 (two channel blocks, the second ragged); residual view
    (1, 4, 4, 4, 64, False, 1, 4, 0, 64, 0, 0, 0),                 # one stage (cin = 4): prologue / tail branches of the ring
    (1, 5, 6, 32, 64, False, 1, 32, 0, 64, 0, 0, 0),               # eight stages
    (1, 8, 8, 64, 64, True, 1, 64, 0, 64, 0, 64, 0),               # sixteen stages
    (9, 26, 26, 128, 64, False, 1, 128, 0, 64, 0, 0, 0),           # 1,521 tiles: 24 tile blocks over the 8 XCD lanes of the block map (three rounds)
]


@pytest.mark.parametrize("case", WINO_CASES)
def test_fp32_winograd_kernel(yt, case):
    """conv_wino_f32 / conv_wino2_f32 through the C-ABI (`yolo_conv_fwd_ws`, tile = 13 / 14): ragged tile / channel blocks, odd and non-square maps,
    1-3 stage rings, ld / off views, residual, every activation; the rest of the output buffer untouched; NaN flag. Reference:
    fp64 convolution of the same operands (model.py:80-86, 115-121) - the bar is what Winograd's transforms cost in fp32
    (1e-5 of max|y|; the north-star bar is 1e-3). The direct kernel (tile 0 without a workspace) is checked beside it."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, residual, act, x_ld, x_off, y_ld, y_off, r_ld, r_off = case
    g = torch.Generator().manual_seed(900 + cin + cout + H + W + B)
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
    d = desc(13)
    need = lib.yolo_conv_workspace_bytes(d)
    tiles = B * ((H + 1) // 2) * ((W + 1) // 2)
    assert need == (tiles + 63) // 64 * 64 * cin * 64
    ws = torch.full((need + 64,), 0x7f, dtype=torch.uint8, device=dev)          # NaN-ish garbage: the transform pass must define all it reads
    errs = {}
    for tile, wsp, wsb in ((13, ws.data_ptr(), need), (14, ws.data_ptr(), need), (0, 0, 0)):    # Winograd in one / two passes; the direct kernel
        yd = y0.clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.yolo_conv_fwd_ws(desc(tile), xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                     yd.data_ptr(), wsp, wsb, flag.data_ptr(), st), "yolo_conv_fwd_ws")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        got = yd.cpu()
        errs[tile] = float((got[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max())
        keep = torch.ones(y_ld, dtype=torch.bool)
        keep[y_off:y_off + cout] = False
        assert torch.equal(got[..., keep], y0[..., keep])           # neighbouring channels of the buffer untouched
    assert errs[13] <= 1e-5 and errs[14] <= 1e-5 and errs[0] <= 5e-6, errs
    assert int(ws[need:].min()) == 0x7f                              # nothing written past the stated size
    # too small a workspace: tile 13 refuses, tile 0 silently takes the direct kernel
    yd = y0.clone().to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    assert lib.yolo_conv_fwd_ws(desc(13), xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                yd.data_ptr(), ws.data_ptr(), need - 16, flag.data_ptr(), st) == -4
    # a NaN in the input reaches the flag
    xn = xd.clone()
    xn[0, 0, 0, x_off] = float("nan")
    L.check(lib.yolo_conv_fwd_ws(d, xn.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                 yd.data_ptr(), ws.data_ptr(), need, flag.data_ptr(), st), "yolo_conv_fwd_ws")
    torch.cuda.synchronize()
    assert int(flag.item()) & 2


@pytest.mark.parametrize("case", [(2, 10, 10, 128, 256, False), (3, 13, 9, 256, 64, True), (1, 6, 6, 64, 96, True)])
def test_fp32_winograd_input_gradient(yt, case):
    """The stride-1 3x3 input gradient on the Winograd kernels: `yolo_pack_weights_dgrad(flip = 1)` appends G g' G^T with
    g'[ci][co][p][q] = w[co][ci][2-p][2-q], `yolo_conv_fwd_ws` (tile 13 and the default) on it is dx = conv_transpose(dz, w)
    [+ the gradient already accumulated in dx] - the backward of nn.Conv2d w.r.t. its input (train.py:67). Reference: fp64."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, accumulate = case
    g = torch.Generator().manual_seed(77 + cin + cout + H)
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
    dzd = dz.to(dev)
    for tile in (13, 0, 7 if coutp % 32 == 0 else 4):
        d = L.ConvDesc(n=B, h=H, w=W, cin=coutp, cout=cin, ksize=3, stride=1, x_ld=coutp, x_off=0, y_ld=cin, y_off=0, r_ld=cin, r_off=0,
                       act=L.ACT_NONE, out_mode=L.OUT_NHWC, dtype=L.F32, flags=L.FLAG_RESIDUAL if accumulate else 0, tile=tile)
        need = lib.yolo_conv_workspace_bytes(d)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        dx = dx0.clone().to(dev)
        L.check(lib.yolo_conv_fwd_ws(d, dzd.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), dx.data_ptr() if accumulate else 0,
                                     dx.data_ptr(), ws.data_ptr() if need else 0, need, 0, st), "yolo_conv_fwd_ws(dgrad)")
        torch.cuda.synchronize()
        err = float((dx.cpu().double() - ref).abs().max() / ref.abs().max())
        assert err <= 1e-5, (tile, err)


S2_CASES = [  # (B, H, cin, cout, residual, act, y_ld, y_off): 3x3 stride 2 on conv1_dma_h16 with gathered rows (tile 13)
    (2, 26, 64, 128, False, 1, 128, 0),          # KT = 18; 338 output pixels: three tiles, the last ragged
    (1, 52, 128, 256, False, 2, 256, 0),         # two n tiles
    (3, 10, 256, 136, False, 1, 136, 0),         # cout not a multiple of 128; 5x5 outputs: tiles straddle rows and images
    (2, 20, 96, 128, True, 0, 192, 64),          # three chunks (odd), residual accumulate into a slice of a wider buffer
    (1, 104, 128, 256, False, 1, 256, 0),        # 2,704 output pixels
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", S2_CASES)
def test_stride2_conv_as_gathered_gemm(yt, case, dtype):
    """The stride-2 3x3 blocks on conv1_dma_h16 with gathered activation rows (tile 13, and the default tile, which must pick
    it): image borders (top row / left column taps read the zero page), ragged and image-straddling pixel tiles, channel
    tiles with padding, residual + ld / off views. Reference: fp64 convolution of the same rounded operands."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, cin, cout, residual, act, y_ld, y_off = case
    code, tdt, tol = {"bf16": (L.BF16, torch.bfloat16, 1e-2), "fp16": (L.F16, torch.float16, 2e-3)}[dtype]
    g = torch.Generator().manual_seed(900 + cin + cout + H)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    Ho = H // 2
    x = torch.randn((B, H, H, cin), generator=g).to(tdt)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cin * 9)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    y0 = torch.randn((B, Ho, Ho, y_ld), generator=g).to(tdt)
    r = torch.randn((B, Ho, Ho, cout), generator=g).to(tdt) if residual else None
    xd, sd, shd, wd = x.to(dev), scale.to(dev), shift.to(dev), w.to(dev)
    rd = r.to(dev) if residual else None
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, code), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(wd.data_ptr(), wp.data_ptr(), cout, cin, 3, code, st))
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.to(tdt).double(), stride=2, padding=1)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1) if act == 1 else (F.mish(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + r.double()
    outs = []
    for tile in (13, 0, 6):                                     # explicit, heuristic (the same kernel), round 2's kernel
        yd = y0.clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        d = L.ConvDesc(n=B, h=H, w=H, cin=cin, cout=cout, ksize=3, stride=2, x_ld=cin, x_off=0, y_ld=y_ld, y_off=y_off, r_ld=cout, r_off=0,
                       act=act, out_mode=L.OUT_NHWC, dtype=code, flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK, tile=tile)
        L.check(lib.yolo_conv_fwd(d, xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                  yd.data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        got = yd.cpu()
        err = float((got[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max())
        assert err <= tol, (tile, err)
        keep = torch.ones(y_ld, dtype=torch.bool)
        keep[y_off:y_off + cout] = False
        assert torch.equal(got[..., keep], y0[..., keep])
        outs.append(got)
    assert torch.equal(outs[0], outs[1])


WS_CASES = [  # (B, H, W, cin, cout, stride, residual, act, y_ld, y_off): conv3_ws_h16 (3x3, <= 64 channels, weights in registers; tile 14)
    (2, 16, 32, 32, 64, 1, False, 1, 64, 0),         # exactly 2 x 2 tiles per image
    (1, 52, 52, 32, 64, 1, True, 1, 64, 0),          # ragged tiles in both directions (52 = 6.5 x 8 = 3.25 x 16), residual
    (3, 13, 19, 32, 40, 1, True, 2, 96, 32),         # cout not a multiple of 32; odd sizes; slice of a wider buffer; Mish
    (2, 26, 26, 64, 32, 1, True, 0, 32, 0),          # the input-gradient shape: 64 -> 32, identity epilogue + accumulate
    (1, 40, 24, 64, 24, 1, False, 1, 24, 0),         # 64 -> 24
    (2, 32, 64, 32, 64, 2, False, 1, 64, 0),         # stride 2: 16 x 32 outputs
    (1, 52, 44, 32, 48, 2, False, 2, 64, 16),        # stride 2, ragged, channel padding, view
    (1, 208, 208, 32, 64, 1, True, 1, 64, 0),        # 13 x 26 = 338 tiles on 338 workgroups: one tile each (the persistent loop, from 513
]                                                    # tiles on, and the second patch buffer: tests/test_gpu_conv_dma_h16.py)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", WS_CASES)
def test_small_channel_3x3_weights_in_registers(yt, case, dtype):
    """conv3_ws_h16 through the C-ABI (tile 14, and the default tile, which must pick it): image borders (zero page), ragged tiles,
    persistent workgroups (at most 338 tiles here: one tile each), residual / accumulate, ld / off views, channel padding, stride 2.
    Reference: fp64 convolution of the same rounded operands; round 2's kernel (tile 5) within the same tolerance."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, H, W, cin, cout, stride, residual, act, y_ld, y_off = case
    code, tdt, tol = {"bf16": (L.BF16, torch.bfloat16, 1e-2), "fp16": (L.F16, torch.float16, 2e-3)}[dtype]
    g = torch.Generator().manual_seed(1700 + cin + cout + H + W)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn((B, H, W, cin), generator=g).to(tdt)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cin * 9)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    y0 = torch.randn((B, Ho, Wo, y_ld), generator=g).to(tdt)
    r = torch.randn((B, Ho, Wo, cout), generator=g).to(tdt) if residual else None
    xd, sd, shd, wd = x.to(dev), scale.to(dev), shift.to(dev), w.to(dev)
    rd = r.to(dev) if residual else None
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, code), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(wd.data_ptr(), wp.data_ptr(), cout, cin, 3, code, st))
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.to(tdt).double(), stride=stride, padding=1)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = F.leaky_relu(ref, 0.1) if act == 1 else (F.mish(ref) if act == 2 else ref)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + r.double()
    outs = []
    for tile in (14, 0, 5):
        yd = y0.clone().to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        d = L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=3, stride=stride, x_ld=cin, x_off=0, y_ld=y_ld, y_off=y_off, r_ld=cout, r_off=0,
                       act=act, out_mode=L.OUT_NHWC, dtype=code, flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK, tile=tile)
        L.check(lib.yolo_conv_fwd(d, xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                                  yd.data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        got = yd.cpu()
        err = float((got[..., y_off:y_off + cout].double() - ref).abs().max() / ref.abs().max())
        assert err <= tol, (tile, err)
        keep = torch.ones(y_ld, dtype=torch.bool)
        keep[y_off:y_off + cout] = False
        assert torch.equal(got[..., keep], y0[..., keep])
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    xn = xd.clone()
    xn[0, H // 2, W // 2, 3] = float("nan")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d.tile = 14
    L.check(lib.yolo_conv_fwd(d, xn.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), rd.data_ptr() if residual else 0,
                              y0.clone().to(dev).data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
    torch.cuda.synchronize()
    assert int(flag.item()) == 2


@pytest.mark.parametrize("seed", range(6))
def test_small_channel_3x3_and_first_block_gradient_random_shapes(yt, seed):
    """Random sizes for the two per-tile streaming kernels of round 3: conv3_ws_h16 (default tile) against an fp64 convolution,
    and stem_wgrad_h16 against an fp64 weight gradient - odd heights, widths that are / are not multiples of the 16-pixel tile,
    batches that leave the last persistent round ragged."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    g = torch.Generator().manual_seed(seed)
    # --- conv3_ws_h16
    B, stride = int(rng.integers(1, 5)), int(rng.integers(1, 3))
    H, W = int(rng.integers(2, 40)) * stride, int(rng.integers(2, 70)) * stride
    cin, cout = (32, int(rng.integers(5, 9)) * 8) if (stride == 2 or rng.random() < 0.5) else (64, int(rng.integers(1, 5)) * 8)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn((B, H, W, cin), generator=g).bfloat16()
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cin * 9)) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.BF16), dtype=torch.uint8, device=dev)
    xd, wd, scd, shd = x.to(dev), w.to(dev), sc.to(dev), sh.to(dev)         # (named: a temporary's memory is recycled before the launch runs)
    L.check(lib.yolo_pack_weights(wd.data_ptr(), wp.data_ptr(), cout, cin, 3, L.BF16, st))
    y = torch.zeros((B, Ho, Wo, cout), dtype=torch.bfloat16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=3, stride=stride, x_ld=cin, x_off=0, y_ld=cout, y_off=0, r_ld=0, r_off=0, act=1,
                   out_mode=L.OUT_NHWC, dtype=L.BF16, flags=L.FLAG_NANCHECK, tile=0)
    L.check(lib.yolo_conv_fwd(d, xd.data_ptr(), wp.data_ptr(), scd.data_ptr(), shd.data_ptr(), 0, y.data_ptr(), flag.data_ptr(), st), "yolo_conv_fwd")
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.bfloat16().double(), stride=stride, padding=1)
    ref = F.leaky_relu(ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.1).permute(0, 2, 3, 1)
    err = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-2 and int(flag.item()) == 0, (B, H, W, cin, cout, stride, err)
    # --- stem_wgrad_h16
    N, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 50)), int(rng.integers(1, 9)) * 16
    cin, cout = int(rng.integers(1, 4)), int(rng.integers(1, 5)) * 8
    xs = torch.zeros((N, H, W, 8), dtype=torch.bfloat16)
    xs[..., :cin] = torch.randn((N, H, W, cin), generator=g).bfloat16()
    dz = torch.zeros((N, H, W, 32), dtype=torch.bfloat16)
    dz[..., :cout] = torch.randn((N, H, W, cout), generator=g).bfloat16()
    wz = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(xs[..., :cin].double().permute(0, 3, 1, 2), wz, padding=1).backward(dz[..., :cout].double().permute(0, 3, 1, 2))
    ws = torch.empty(lib.yolo_wgrad_workspace_bytes(N, H, W, cin, cout, 3, 1, L.BF16), dtype=torch.uint8, device=dev)
    dw = torch.full((cout, cin, 3, 3), float("nan"), dtype=torch.float32, device=dev)
    dzd, xsd = dz.to(dev), xs.to(dev)
    L.check(lib.yolo_conv_wgrad(dzd.data_ptr(), 32, 0, xsd.data_ptr(), 8, 0, dw.data_ptr(), N, H, W, cin, cout, 3, 1, L.BF16,
                                ws.data_ptr(), ws.numel(), st), "wgrad")
    err = float((dw.cpu().double() - wz.grad).abs().max() / wz.grad.abs().max())
    assert err < 2e-5, (N, H, W, cin, cout, err)


S2_DGRAD_CASES = [  # (B, Ho, cin, cout, residual, dz_ld, dx_ld, dx_off)
    (2, 13, 32, 64, False, 64, 32, 0),           # the stem's successor: four classes in ONE n tile; 338 dz pixels, ragged last tile
    (1, 26, 64, 128, True, 128, 64, 0),          # two n tiles, accumulate into the running gradient
    (3, 5, 64, 128, True, 160, 96, 32),          # tiles straddle rows and images; dz / dx are slices of wider buffers
    (2, 8, 32, 96, False, 96, 32, 0),            # three chunks
    (1, 12, 128, 256, True, 256, 128, 0),        # > 64 channels: the four per-class launches (unchanged path)
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", S2_DGRAD_CASES)
def test_stride2_input_gradient_kernels(yt, case, dtype):
    """yolo_conv_dgrad_s2: dx of a 3x3 stride-2 convolution (model.py:17's conv in the five down-sampling blocks). For
    <= 64 dx channels the four parity classes run as ONE gathered-row GEMM (conv1_dma_h16, gather mode 2); wider layers
    keep one launch per class. Reference: fp64 conv_transpose2d of the same rounded operands; the last row / column of
    dz (neighbours outside the image read the zero page), residual accumulate and ld / off views are covered."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    B, Ho, cin, cout, residual, dz_ld, dx_ld, dx_off = case
    code, tdt, tol = {"bf16": (L.BF16, torch.bfloat16, 1e-2), "fp16": (L.F16, torch.float16, 2e-3)}[dtype]
    g = torch.Generator().manual_seed(1300 + cin + cout + Ho)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    H = 2 * Ho
    dz = torch.randn((B, Ho, Ho, dz_ld), generator=g).to(tdt)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (cout * 2.25)) ** 0.5
    dx0 = torch.randn((B, H, H, dx_ld), generator=g).to(tdt)
    wd = w.to(dev)
    wp = torch.empty(lib.yolo_packed_dgrad_bytes(cout, cin, 3, 0, code), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights_dgrad(wd.data_ptr(), wp.data_ptr(), cout, cin, 3, 0, code, st))
    ref = F.conv_transpose2d(dz[..., :cout].double().permute(0, 3, 1, 2), w.to(tdt).double(), stride=2, padding=1, output_padding=1)
    ref = ref.permute(0, 2, 3, 1)
    if residual:
        ref = ref + dx0[..., dx_off:dx_off + cin].double()
    dzd, dxd = dz.to(dev), dx0.clone().to(dev)
    rptr = dxd.data_ptr() if residual else 0
    L.check(lib.yolo_conv_dgrad_s2(dzd.data_ptr(), dz_ld, 0, wp.data_ptr(), rptr, dx_ld, dx_off, dxd.data_ptr(), dx_ld, dx_off, B, Ho, Ho,
                                   cin, cout, code, st), "yolo_conv_dgrad_s2")
    torch.cuda.synchronize()
    got = dxd.cpu()
    err = float((got[..., dx_off:dx_off + cin].double() - ref).abs().max() / ref.abs().max())
    assert err <= tol, err
    keep = torch.ones(dx_ld, dtype=torch.bool)
    keep[dx_off:dx_off + cin] = False
    assert torch.equal(got[..., keep], dx0[..., keep])


FUSED_STATS_CASES = [  # B, H, cin, cout, k: 3x3 / 1x1 LDS-DMA kernels; ragged and image-straddling tiles, channel tiles with padding
    (2, 13, 64, 128, 3), (3, 7, 96, 72, 3), (1, 52, 128, 256, 3), (4, 26, 128, 136, 3), (2, 13, 256, 128, 1), (1, 19, 128, 200, 1),
    (3, 5, 384, 128, 1),
    # conv3_ws_h16 (<= 64 channels; one row per wave of the persistent workgroups): [, stride]
    (2, 20, 32, 64, 3), (1, 52, 64, 32, 3), (3, 9, 32, 40, 3), (2, 24, 32, 64, 3, 2), (1, 208, 32, 64, 3)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", FUSED_STATS_CASES)
def test_conv_epilogue_batchnorm_statistics(yt, case, dtype):
    """yolo_conv_fwd_stats + yolo_bn_stats_from_partials (train-mode forward: batch statistics from the convolution's epilogue)
    against (a) the same convolution through yolo_conv_fwd: z bit-identical, and (b) yolo_bn_stats on that z and an fp64 mean /
    variance of the stored values: mean, invstd, scale, shift and the running-statistic update."""
    from yolo_for_turbines_amd import _lib as L
    B, H, cin, cout, k = case[:5]
    stride = case[5] if len(case) > 5 else 1
    Ho = (H - 1) // stride + 1
    code, tdt = {"bf16": (L.BF16, torch.bfloat16), "fp16": (L.F16, torch.float16)}[dtype]
    g = torch.Generator().manual_seed(77 + cin + 3 * cout + H)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    x = (torch.randn((B, H, H, cin), generator=g) + 0.3).to(tdt).to(dev)
    w = (torch.randn((cout, cin, k, k), generator=g) * (1.0 / (cin * k * k)) ** 0.5).to(dev)
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, k, code), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights(w.data_ptr(), wp.data_ptr(), cout, cin, k, code, st))
    d = L.ConvDesc(n=B, h=H, w=H, cin=cin, cout=cout, ksize=k, stride=stride, x_ld=cin, x_off=0, y_ld=cout, y_off=0, r_ld=0, r_off=0, act=0,
                   out_mode=L.OUT_NHWC, dtype=code, flags=0, tile=0)
    import ctypes as C
    ld = C.c_int(0)
    rows = lib.yolo_conv_stats_rows(d, C.byref(ld))
    assert rows > 0 and ld.value >= cout
    ones, zeros = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    m = B * Ho * Ho
    z_ref = torch.full((m, cout), 7.0, dtype=tdt, device=dev)
    z = torch.full((m, cout), 7.0, dtype=tdt, device=dev)
    L.check(lib.yolo_conv_fwd(d, x.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), 0, z_ref.data_ptr(), 0, st), "conv")
    part = torch.full((rows * 2 * ld.value,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.yolo_conv_fwd_stats(d, x.data_ptr(), wp.data_ptr(), z.data_ptr(), part.data_ptr(), part.numel() * 4, st), "conv_fwd_stats")
    assert torch.equal(z, z_ref)
    gamma, beta = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)

    def stats(fused):
        rm, rv = torch.full((cout,), 0.25, device=dev), torch.full((cout,), 2.0, device=dev)
        out = [torch.empty(cout, device=dev) for _ in range(4)]
        if fused:
            L.check(lib.yolo_bn_stats_from_partials(part.data_ptr(), rows, ld.value, m, cout, gamma.data_ptr(), beta.data_ptr(), 0.1, 1e-5,
                                                    rm.data_ptr(), rv.data_ptr(), *[t.data_ptr() for t in out], st), "from_partials")
        else:
            ws = torch.empty(lib.yolo_bn_workspace_bytes(m, cout), dtype=torch.uint8, device=dev)
            L.check(lib.yolo_bn_stats(z.data_ptr(), m, cout, cout, 0, gamma.data_ptr(), beta.data_ptr(), 0.1, 1e-5, rm.data_ptr(), rv.data_ptr(),
                                      *[t.data_ptr() for t in out], code, ws.data_ptr(), ws.numel(), st), "bn_stats")
        return [t.cpu().double() for t in out + [rm, rv]]
    a, b = stats(True), stats(False)
    z64 = z.cpu().double()
    mu, var = z64.mean(0), z64.var(0, unbiased=False)
    np.testing.assert_allclose(a[0].numpy(), mu.numpy(), rtol=0, atol=2e-6 * float(z64.abs().max()))
    np.testing.assert_allclose(a[1].numpy(), (1.0 / torch.sqrt(var + 1e-5)).numpy(), rtol=5e-6)
    for u, v in zip(a, b):                      # and the separate statistics pass agrees (both sum the stored, rounded values)
        np.testing.assert_allclose(u.numpy(), v.numpy(), rtol=5e-6, atol=1e-6)
    assert not bool(torch.isnan(part.view(rows, 2, ld.value)[:, :, :cout]).any())


FUSED_BSTATS_CASES = [  # B, H, c (channels of dx = of the producing block), cg (channels of dz), k, accumulate, act of the block
    (2, 13, 128, 64, 3, False, 1), (3, 7, 72, 96, 3, True, 2), (1, 52, 256, 128, 3, False, 1), (2, 13, 128, 256, 1, True, 1),
    (1, 19, 200, 128, 1, True, 2), (4, 26, 256, 128, 1, True, 1)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", FUSED_BSTATS_CASES)
def test_dgrad_epilogue_batchnorm_backward_sums(yt, case, dtype):
    """yolo_conv_dgrad_bstats + yolo_bn_act_bwd_rows (the reduction pass of BatchNorm's backward taken in the epilogue of the
    convolution that writes dy) against the separate path: (a) dx bit-identical to the same input-gradient convolution through
    yolo_conv_fwd; (b) dgamma, dbeta, dz equal to yolo_bn_act_bwd on that dx (both sum the stored, rounded values; the orders
    differ) and to an fp64 evaluation of the formula. Ragged / image-straddling tiles, channel tiles with padding, accumulate."""
    import ctypes as C
    from yolo_for_turbines_amd import _lib as L
    B, H, c, cg, k, accum, act = case
    code, tdt = {"bf16": (L.BF16, torch.bfloat16), "fp16": (L.F16, torch.float16)}[dtype]
    g = torch.Generator().manual_seed(311 + c + 3 * cg + H)
    lib, dev, st = L.lib(), torch.device("cuda:0"), L.current_stream()
    m = B * H * H
    dzn = torch.randn((B, H, H, cg), generator=g).to(tdt).to(dev)                    # gradient of the NEXT block's conv output
    w = (torch.randn((cg, c, k, k), generator=g) * (1.0 / (cg * k * k)) ** 0.5).to(dev)  # the next block's weights (cout = cg, cin = c)
    wp = torch.empty(lib.yolo_packed_dgrad_bytes(cg, c, k, 1, code), dtype=torch.uint8, device=dev)
    L.check(lib.yolo_pack_weights_dgrad(w.data_ptr(), wp.data_ptr(), cg, c, k, 1, code, st))
    run = torch.randn((m, c), generator=g).to(tdt).to(dev) if accum else None       # the running gradient (skip connection)
    z = (torch.randn((m, c), generator=g) * 1.5 + 0.2).to(tdt).to(dev)              # the producing block's conv output
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev)
    z64 = z.cpu().double()
    mean = z64.mean(0).float().to(dev)
    invstd = (1.0 / torch.sqrt(z64.var(0, unbiased=False) + 1e-5)).float().to(dev)
    scale, shift = gamma * invstd, beta.clone()
    d = L.ConvDesc(n=B, h=H, w=H, cin=cg, cout=c, ksize=k, stride=1, x_ld=cg, x_off=0, y_ld=c, y_off=0, r_ld=c, r_off=0, act=0,
                   out_mode=L.OUT_NHWC, dtype=code, flags=L.FLAG_RESIDUAL if accum else 0, tile=0)
    ld = C.c_int(0)
    rows = lib.yolo_conv_bstats_rows(d, C.byref(ld))
    assert rows > 0 and ld.value >= c
    ones, zeros = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    dx_ref = torch.full((m, c), 7.0, dtype=tdt, device=dev)
    dx = torch.full((m, c), 7.0, dtype=tdt, device=dev)
    rp = run.data_ptr() if accum else 0
    L.check(lib.yolo_conv_fwd(d, dzn.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), rp, dx_ref.data_ptr(), 0, st), "dgrad")
    part = torch.full((rows * 2 * ld.value + 3 * c,), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.yolo_conv_dgrad_bstats(d, dzn.data_ptr(), wp.data_ptr(), rp, dx.data_ptr(), z.data_ptr(), c, 0, mean.data_ptr(),
                                       scale.data_ptr(), shift.data_ptr(), act, part.data_ptr(), part.numel() * 4, st), "dgrad_bstats")
    assert torch.equal(dx, dx_ref)
    assert not bool(torch.isnan(part[:rows * 2 * ld.value].view(rows, 2, ld.value)[:, :, :c]).any())

    def bwd(fused):
        dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
        out = torch.empty((m, c), dtype=tdt, device=dev)
        if fused:
            L.check(lib.yolo_bn_act_bwd_rows(dx.data_ptr(), c, 0, z.data_ptr(), c, 0, gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                             scale.data_ptr(), shift.data_ptr(), m, c, act, dg.data_ptr(), db.data_ptr(), out.data_ptr(), c, 0,
                                             code, part.data_ptr(), rows, ld.value, st), "bn_act_bwd_rows")
        else:
            ws = torch.empty(lib.yolo_bn_workspace_bytes(m, c), dtype=torch.uint8, device=dev)
            L.check(lib.yolo_bn_act_bwd(dx.data_ptr(), c, 0, z.data_ptr(), c, 0, gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        scale.data_ptr(), shift.data_ptr(), m, c, act, dg.data_ptr(), db.data_ptr(), out.data_ptr(), c, 0,
                                        code, ws.data_ptr(), ws.numel(), st), "bn_act_bwd")
        torch.cuda.synchronize()
        return dg.cpu().double(), db.cpu().double(), out.cpu().double()
    a, b = bwd(True), bwd(False)
    # fp64 evaluation of the formula on the stored values (the activation derivative decided in fp32 like the kernels)
    u32 = (z.float() - mean) * scale + shift
    if act == 1:
        gprime = torch.where(u32 > 0, 1.0, 0.1).cpu().double()
    else:
        u64 = u32.cpu().double().requires_grad_(True)
        torch.nn.functional.mish(u64).sum().backward()
        gprime = u64.grad
    du = dx.cpu().double() * gprime
    zhat = (z64 - mean.cpu().double()) * invstd.cpu().double()
    dbeta, dgamma = du.sum(0), (du * zhat).sum(0)
    sc_s, sc_q = float(du.abs().sum(0).max()), float((du * zhat).abs().sum(0).max())
    np.testing.assert_allclose(a[1].numpy(), dbeta.numpy(), rtol=0, atol=3e-6 * sc_s)
    np.testing.assert_allclose(a[0].numpy(), dgamma.numpy(), rtol=0, atol=3e-6 * sc_q)
    np.testing.assert_allclose(a[1].numpy(), b[1].numpy(), rtol=0, atol=3e-6 * sc_s)
    np.testing.assert_allclose(a[0].numpy(), b[0].numpy(), rtol=0, atol=3e-6 * sc_q)
    tol = {"bf16": 1.6e-2, "fp16": 2e-3}[dtype]                 # dz is rounded to the 16-bit type: at most one unit apart
    assert float((a[2] - b[2]).abs().max()) <= tol * float(b[2].abs().max())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 32, 32), (3, 37, 45), (2, 5, 3), (1, 1, 70), (2, 96, 96), (1, 416, 416)])
def test_stem_block_on_the_matrix_cores(yt, shape, dtype):
    """yolo_stem_fwd with a 16-bit output (stem3x3_mfma_h16): widths that are not multiples of the 32-pixel tile (tiles that wrap
    around rows and images), images narrower than a tile, a pixel count that is not a multiple of the wave's 8 tiles, every
    border, ld / off views, the activation, and the two NaN guards (input centre taps; an Inf input gives +-Inf / NaN like the
    reference, never a NaN from a masked or padded tap). Reference: fp64 convolution of the operands rounded to the 16-bit type
    (what the reference's autocast conv multiplies), so the only error left is fp32 accumulation order + the final rounding."""
    import torch.nn.functional as F
    from yolo_for_turbines_amd import _lib as L
    N, H, W = shape
    code, tdt, tol = {"bf16": (L.BF16, torch.bfloat16, 8e-3), "fp16": (L.F16, torch.float16, 1.5e-3)}[dtype]
    g = torch.Generator().manual_seed(31 * H + W + N)
    lib, dev = L.lib(), torch.device("cuda:0")
    x = torch.rand((N, 3, H, W), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) * 0.3
    scale, shift = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1
    y_ld, y_off = 48, 16
    y0 = torch.randn((N, H, W, y_ld), generator=g).to(tdt)
    xd, wd, sd, shd, yd = x.to(dev), w.to(dev), scale.to(dev), shift.to(dev), y0.clone().to(dev)
    wp = torch.empty(27 * 32, dtype=torch.float32, device=dev)
    st = L.current_stream()
    L.check(lib.yolo_stem_pack(wd.data_ptr(), wp.data_ptr(), 32, st))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(inp, out):
        L.check(lib.yolo_stem_fwd(inp.data_ptr(), wp.data_ptr(), sd.data_ptr(), shd.data_ptr(), out.data_ptr(), N, H, W, 32, y_ld, y_off,
                                  1, code, flag.data_ptr(), st), "yolo_stem_fwd")
        torch.cuda.synchronize()

    run(xd, yd)
    assert int(flag.item()) == 0
    ref = F.conv2d(x.to(tdt).double(), w.to(tdt).double(), stride=1, padding=1)
    ref = F.leaky_relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), 0.1).permute(0, 2, 3, 1)
    got = yd.cpu()
    err = float((got[..., y_off:y_off + 32].double() - ref).abs().max() / ref.abs().max())
    assert err <= tol, err
    keep = torch.ones(y_ld, dtype=torch.bool)
    keep[y_off:y_off + 32] = False
    assert torch.equal(got[..., keep], y0[..., keep])                           # the rest of the buffer untouched
    # an Inf in a corner: its 2x2 neighbourhood becomes +-Inf (or NaN where +Inf and -Inf meet), everything else stays finite
    xi = x.clone()
    xi[0, 1, 0, 0] = float("inf")
    yi = y0.clone().to(dev)
    flag.zero_()
    run(xi.to(dev), yi)
    outi = yi.cpu()[..., y_off:y_off + 32].float()
    far = torch.ones((N, H, W), dtype=torch.bool)
    far[0, :2, :2] = False
    assert torch.isfinite(outi[far]).all() and not torch.isfinite(outi[0, 0, 0]).all()
    # a NaN anywhere in the input raises bit 0 of the flag (model.py:175)
    xn = x.clone()
    xn[N - 1, 2, H - 1, W - 1] = float("nan")
    flag.zero_()
    run(xn.to(dev), yi)
    assert int(flag.item()) & 1


@pytest.mark.parametrize("cfg", [dict(lr=1e-4, momentum=0.9, weight_decay=5e-4), dict(lr=0.01), dict(lr=0.05, momentum=0.8, dampening=0.1),
                                 dict(lr=0.02, momentum=0.9, weight_decay=1e-3, nesterov=True), dict(lr=0.03, momentum=0.5, maximize=True),
                                 dict(lr=0.01, weight_decay=0.1)])
def test_sgd_step_same_bits_as_torch(yt, cfg):
    """yt.SGD (one HIP launch over all parameters) against torch.optim.SGD as train.py:171-172 constructs it: identical bits in
    every parameter and momentum buffer after each of four steps (the first one creates the buffers), tensor sizes that are not
    multiples of the 4,096-element chunk or of four, a parameter that never gets a gradient, one that gets it only from the
    third step on, a view that is not 16-byte aligned, and a state_dict round trip into the PyTorch optimizer."""
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 32, 3, 3), (32,), (1,), (255, 1024, 1, 1), (4097,), (3, 5, 7), (1030,)]
    base = torch.randn(1031, generator=g).cuda()
    def make():
        ps = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i)).cuda()) for i, s in enumerate(shapes)]
        ps.append(torch.nn.Parameter(base.clone()[1:]))                 # storage offset of 4 bytes: the scalar path
        return ps
    pa, pb = make(), make()
    oa, ob = yt.SGD(pa, **cfg), torch.optim.SGD(pb, **cfg)
    for step in range(4):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == 2 or (i == 4 and step < 2):
                a.grad = b.grad = None
                continue
            gr = torch.randn(a.shape, generator=torch.Generator().manual_seed(100 * step + i)).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert torch.equal(a, b), (step, i)
            ba, bb = oa.state[a].get("momentum_buffer"), ob.state[b].get("momentum_buffer")
            assert (ba is None) == (bb is None) and (ba is None or torch.equal(ba, bb)), (step, i)
    oc = torch.optim.SGD(make(), **cfg)
    oc.load_state_dict(oa.state_dict())                                  # utils.py:383-416 checkpoints load either way
    assert oc.state_dict()["param_groups"][0]["lr"] == cfg["lr"]
    cpu_p = torch.nn.Parameter(torch.zeros(4))
    cpu_p.grad = torch.ones(4)
    with pytest.raises(TypeError):                                       # no CPU fallback
        yt.SGD([cpu_p], lr=0.1).step()


def test_detect_images_one_sync_same_results_same_exceptions(yt):
    """detect_images(model, x, ...) = detect(model(x), ...) with the forward's NaN guards read after the post-processing is
    enqueued: identical boxes / kept indices / counts, the reference's exceptions for a NaN input (model.py:175) and for a
    NaN produced by a layer (model.py:183-184), and the engine back in its normal mode afterwards (also after a raise)."""
    c = gi.NET_CASES["nc80_s96_b2_leaky"]
    m = _model(yt, c)
    x = onet.synth_input(78, 3, 128).cuda()
    anchors = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
               [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]
    sa = [torch.tensor(a).cuda() * g for a, g in zip(anchors, (4, 8, 16))]
    with torch.no_grad():
        b0, k0, c0 = yt.detect(m(x), sa, 0.45, 0.5, "center")
    b1, k1, c1 = yt.detect_images(m, x, sa, 0.45, 0.5, "center")
    assert torch.equal(b0, b1) and torch.equal(c0, c1)
    for i in range(3):
        assert torch.equal(k0[i, :int(c0[i])], k1[i, :int(c1[i])])
    xn = x.clone()
    xn[1, 0, 5, 5] = float("nan")
    with pytest.raises(AssertionError):
        yt.detect_images(m, xn, sa, 0.45, 0.5, "center")
    assert m._engine._defer_nan is False and m._engine._pending_flag is None
    with pytest.raises(AssertionError):                                  # and the plain forward still guards by itself
        with torch.no_grad():
            m(xn)
    w = m.layers[3].conv.weight if hasattr(m.layers[3], "conv") else next(m.layers[3].parameters())
    with torch.no_grad():
        old = w.detach().clone()
        w.fill_(float("inf"))                                            # inf * 0-ish activations -> NaN inside the network
    with pytest.raises(ValueError, match="Nan in layer"):
        yt.detect_images(m, x, sa, 0.45, 0.5, "center")
    with torch.no_grad():
        w.copy_(old)
    b2, k2, c2 = yt.detect_images(m, x, sa, 0.45, 0.5, "center")
    assert torch.equal(b0, b2) and torch.equal(c0, c2)
