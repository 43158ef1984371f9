"""Training augmentation on the MI355X (csrc/augment.hip) against the numpy restatement tests/augment_ref.py: pixels bit
for bit, boxes bit for bit after the fp32 store; the no-sync train_batch path and one graphed training step fed by it."""
import numpy as np
import pytest
import torch

from tests import augment_ref as ar

pytestmark = pytest.mark.gpu

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
           [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as m
    return m


def _img(seed, h, w):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)      # smooth-ish content plus noise
    big = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w].astype(np.int32)
    return np.clip(big + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def _boxes(seed, n):
    rng = np.random.default_rng(seed + 1000)
    return [[float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.05, 0.4)),
             float(rng.uniform(0.05, 0.4)), float(rng.integers(0, 2))] for _ in range(n)]


def _params(B, **on):
    p = np.zeros((B, ar.NPARAM))
    p[:, ar.SCALE] = 1.0
    for k, v in on.items():
        p[:, getattr(ar, k.upper())] = v
    return p


def _check(yt, images, boxes, params, size, mosaic=None):
    H, W = (size, size) if np.isscalar(size) else size
    x, bt, ct = yt.augment_batch(images, boxes, image_size=size, params=torch.as_tensor(params), mosaic=mosaic)
    rx, rb, paths = ar.augment(images, boxes, params, H, W, mosaic)
    assert torch.equal(x.cpu(), torch.from_numpy(rx)), "pixels differ from augment_ref"
    ct = ct.cpu()
    for b in range(len(rb)):
        assert int(ct[b]) == len(rb[b])
        got = bt[b, :int(ct[b])].cpu().numpy()
        assert np.array_equal(got, np.asarray(rb[b], np.float32).reshape(-1, 5)), f"boxes of image {b} differ"
    return x, bt, ct, paths


SRC = [(375, 500), (480, 640), (1080, 1920), (416, 416)]


def test_all_off_equals_letterbox(yt):
    images = [_img(i, h, w) for i, (h, w) in enumerate(SRC)]
    boxes = [[[0.5, 0.5, 0.2, 0.3, 1.0], [0.3, 0.6, 0.1, 0.1, 0.0], [0.8, 0.25, 0.3, 0.4, 1.0]] for _ in SRC]   # nothing clipped
    p = _params(len(SRC))
    x, bt, ct, _ = _check(yt, images, boxes, p, 416)
    ref, meta = yt.letterbox(images, 416)
    assert torch.equal(x, ref)
    for b, m in enumerate(meta):                           # boxes follow the letterbox mapping
        h, w, nh, nw, top, left = m
        for r, bx in zip(bt[b, :int(ct[b])].cpu().tolist(), boxes[b]):
            assert abs(r[0] - (bx[0] * nw + left) / 416) < 1e-6 and abs(r[1] - (bx[1] * nh + top) / 416) < 1e-6
            assert abs(r[2] - bx[2] * nw / 416) < 1e-6 and abs(r[3] - bx[3] * nh / 416) < 1e-6
    landscape = [images[0], images[1], images[2]]
    ref_r, _ = yt.letterbox(landscape, 416, rect=True)
    xr, _, _, _ = _check(yt, landscape, [boxes[0], boxes[1], boxes[2]], _params(3), tuple(ref_r.shape[2:]))
    assert torch.equal(xr, ref_r)


@pytest.mark.parametrize("which", ["hsv", "ssr", "flip", "all"])
def test_transforms_match_restatement(yt, which):
    images = [_img(10 + i, h, w) for i, (h, w) in enumerate(SRC)]
    boxes = [_boxes(10 + i, 6) for i in range(len(SRC))]
    p = yt.augment_params(len(SRC), torch.Generator().manual_seed(5)).numpy()
    keep = {"hsv": [ar.DO_HSV], "ssr": [ar.DO_SSR], "flip": [ar.DO_FLIP], "all": [ar.DO_HSV, ar.DO_SSR, ar.DO_FLIP]}[which]
    for col in (ar.DO_HSV, ar.DO_SSR, ar.DO_FLIP):
        p[:, col] = 1.0 if col in keep else 0.0
    _check(yt, images, boxes, p, 416)
    _check(yt, images[:2], boxes[:2], p[:2], (320, 416))    # rectangular canvas


def test_visibility_cases(yt):
    img = _img(50, 64, 64)
    # 64 x 64 canvas, shift left by 16 px: columns [10, 20] -> [-6, 4] keeps 0.4 exactly; one px more drops; a box that
    # leaves the canvas entirely is clipped to zero area and dropped
    keep = [0.234375, 0.375, 0.15625, 0.25, 1.0]
    drop = [0.234375 - 1 / 64, 0.375, 0.15625, 0.25, 0.0]
    gone = [0.1, 0.6, 0.1, 0.1, 1.0]
    p = _params(1, do_ssr=1.0, dx=-0.25)
    _, bt, ct, _ = _check(yt, [img], [[keep, drop, gone]], p, 64)
    assert int(ct[0]) == 1 and float(bt[0, 0, 4]) == 1.0


def test_mosaic(yt):
    shapes = [(480, 640)] * 4 + [(375, 500)] * 4 + [(300, 400)] * 4
    images = [_img(70 + i, h, w) for i, (h, w) in enumerate(shapes)]
    boxes = [_boxes(70 + i, 2) for i in range(len(shapes))]
    boxes[5] = []
    boxes[6] = None
    mosaic = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [3, 2, 1, 0]]
    p = yt.augment_params(4, torch.Generator().manual_seed(9), mosaic=True).numpy()
    _, _, _, paths = _check(yt, images, boxes, p, 416, np.array(mosaic))
    assert all(a >= 0 for a in paths)
    # no box anywhere: the standard transform of the first image (the reference would crash); all ten draws missing: same
    empty = [[] for _ in images]
    _, _, ct, paths = _check(yt, images, empty, p, 416, np.array(mosaic))
    assert paths == [-1] * 4 and ct.sum() == 0
    tiny = [[[0.02, 0.02, 0.01, 0.01, 0.0]] if i % 4 == 0 else [] for i in range(len(images))]   # top-left corner only
    _, _, _, paths = _check(yt, images, tiny, p, 416, np.array(mosaic))
    assert paths[0] == -1
    with pytest.raises(ValueError):
        yt.augment_batch(images, boxes, image_size=(416, 320), params=torch.as_tensor(p), mosaic=np.array(mosaic))
    with pytest.raises(ValueError):
        yt.augment_batch(images, boxes, image_size=416, params=torch.as_tensor(p), mosaic=np.array([[0, 4, 8, 1]]))


def test_none_labels_and_empty_lists(yt):
    images = [_img(90, 480, 640), _img(91, 375, 500)]
    p = _params(2, do_hsv=1.0, hue=1.5, sat=30.0, val=-20.0, do_flip=1.0)
    x, _, ct, paths = _check(yt, images, [None, []], p, 416)
    assert paths == [-2, -1] and ct.tolist() == [0, 0]
    ref, _ = yt.letterbox(images, 416)
    assert torch.equal(x[0], ref[0]) and not torch.equal(x[1], ref[1])


def test_train_batch_no_sync(yt):
    images = [torch.from_numpy(_img(100 + i, 480, 640)) for i in range(4)]
    boxes = [_boxes(100 + i, 4) for i in range(4)]
    p = yt.augment_params(4, torch.Generator().manual_seed(2))
    x0, bt, ct = yt.augment_batch(images, boxes, 416, params=p)
    t0 = yt.build_targets(bt, ANCHORS, 416, counts=ct)
    torch.cuda.synchronize()
    anc = torch.tensor(ANCHORS).cuda()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x1, t1 = yt.train_batch(images, boxes, anc, 416, params=p)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(x0, x1)
    for a, b in zip(t0, t1):
        assert torch.equal(a, b)


def test_same_seed_same_bits(yt):
    images = [_img(120 + i, 480, 640) for i in range(4)]
    boxes = [_boxes(120 + i, 3) for i in range(4)]
    xa = yt.augment_batch(images, boxes, 416, generator=torch.Generator().manual_seed(7))[0]
    xb = yt.augment_batch(images, boxes, 416, generator=torch.Generator().manual_seed(7))[0]
    xc = yt.augment_batch(images, boxes, 416, generator=torch.Generator().manual_seed(8))[0]
    assert torch.equal(xa, xb) and not torch.equal(xa, xc)


def test_graphed_step_from_train_batch(yt):
    from oracle import net as onet
    B, S, nc = 8, 416, 2
    torch.manual_seed(0)
    m = yt.YOLOv3(num_classes=nc)
    m.load_state_dict(onet.synth_state_dict(11, 3, nc, gain=0.8))
    m = m.cuda().train()
    opt = yt.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
    sa = [torch.tensor(a).cuda() * g for a, g in zip(ANCHORS, (S // 32, S // 16, S // 8))]
    images = [_img(200 + i, 480, 640) for i in range(B)]
    boxes = [_boxes(200 + i, 3) for i in range(B)]
    x, targets = yt.train_batch(images, boxes, ANCHORS, S, generator=torch.Generator().manual_seed(3))
    step = yt.GraphedTrainStep(m, opt, sa, x, targets, autocast_dtype=torch.bfloat16)
    x2, t2 = yt.train_batch(images, boxes, ANCHORS, S, generator=torch.Generator().manual_seed(4))   # copied into the statics
    loss = step(x2, t2)
    assert bool(torch.isfinite(loss))
