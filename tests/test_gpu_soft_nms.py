"""yolo_soft_nms / soft_nms on the GPU, bit for bit against the numpy restatement of its contract (tests/soft_nms_ref.py) for all
three methods - w(t) is defined to the bit, so the Gaussian scores are compared by bits too: keep, count, scores and the rescored
column, with the output buffers pre-filled with 0xA5 and guard bytes behind them. The cases come from the reference's builders
(tests/test_soft_nms_host.py checks the same cases against the fp64 yardstick on the CPU). Then method 0 against yolo_nms, and the
``nms=`` keyword of detect, detect_tiled and the tracker."""
import functools

import numpy as np
import pytest
import torch

from tests import golden_inputs as gi
from tests import soft_nms_ref as R

pytestmark = pytest.mark.gpu
SPARE = 4096            # guard bytes behind every output buffer
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    import yolo_for_turbines_amd  # noqa: F401
    from yolo_for_turbines_amd import _lib
    _lib.lib()                       # must load: no fallback
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd
    return yolo_for_turbines_amd


@pytest.fixture(scope="module")
def model(yt):
    from oracle import net as onet
    m = yt.YOLOv3(num_classes=80)
    m.load_state_dict(onet.synth_state_dict(11, 3, 80, gain=gi.NET_GAIN))
    return m.cuda().eval()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def filled(nbytes, value=0xA5):
    return torch.full((nbytes + SPARE,), value, dtype=torch.uint8, device="cuda")


def run_c(L, boxes, rescore="separate", iou_threshold=0.45, obj_threshold=0.25, score_threshold=None, box_format="center",
          method="gaussian", sigma=0.5, class_agnostic=False, max_det=None):
    """yolo_soft_nms through the C ABI into 0xA5-filled buffers; checks the guard bytes; returns numpy arrays (keep, count, scores,
    rescored). ``rescore``: "none" (NULL; rescored is None), "separate" (a copy of boxes) or "boxes" (boxes itself)."""
    boxes = np.ascontiguousarray(boxes, F32)
    B, N, _ = boxes.shape
    lib = L.lib()
    sizes = [B * N * 4, B * 4, B * N * 4, B * N * 24]
    bufs = [filled(s) for s in sizes]
    d_boxes = bufs[3][:sizes[3]].view(torch.float32)
    d_boxes.copy_(torch.from_numpy(boxes).reshape(-1))
    d_res = {"none": None, "separate": d_boxes.clone(), "boxes": d_boxes}[rescore]
    nbytes = lib.yolo_soft_nms_workspace_bytes(B, N)
    assert nbytes > 0
    ws = filled(nbytes, 0x5A)
    rc = lib.yolo_soft_nms(d_boxes.data_ptr(), B, N, float(iou_threshold), float(obj_threshold),
                           float(obj_threshold if score_threshold is None else score_threshold), int(box_format == "center"),
                           R.METHODS[method], float(sigma), int(class_agnostic), int(max_det or 0), bufs[0].data_ptr(), bufs[1].data_ptr(),
                           bufs[2].data_ptr(), None if d_res is None else d_res.data_ptr(), ws.data_ptr(), nbytes,
                           torch.cuda.current_stream().cuda_stream)
    L.check(rc, "yolo_soft_nms")
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs + [ws]]
    for h, s in zip(host, sizes + [nbytes]):
        guard = h[s:]
        assert (guard == guard[0]).all() and guard[0] in (0xA5, 0x5A), "wrote behind a buffer"
    keep = host[0][:sizes[0]].view(np.int32).reshape(B, N)
    count = host[1][:sizes[1]].view(np.int32)
    scores = host[2][:sizes[2]].view(F32).reshape(B, N)
    after = host[3][:sizes[3]].view(F32).reshape(B, N, 6)
    if rescore != "boxes":
        np.testing.assert_array_equal(bits(after), bits(boxes))              # boxes is never written unless it is rescore_rows
    rescored = None if d_res is None else (after if rescore == "boxes" else d_res.cpu().numpy().reshape(B, N, 6))
    return keep, count, scores, rescored


def as_batch(rows):
    rows = np.asarray(rows, F32)
    return rows if rows.ndim == 3 else rows[None]


def check(L, rows, kw, rescore="separate", want=None):
    rows = as_batch(rows)
    got = run_c(L, rows, rescore=rescore, **kw)
    want = want or R.soft_nms_ref_batch(rows, **kw)
    np.testing.assert_array_equal(got[1], want[1])                           # count
    np.testing.assert_array_equal(got[0], want[0])                           # keep, -1 behind count
    np.testing.assert_array_equal(bits(got[2]), bits(want[2]))               # scores, 0 behind count, by bits
    if got[3] is not None:
        np.testing.assert_array_equal(bits(got[3]), bits(want[3]))           # column 4 of the emitted rows, every other byte as it was
    return want


@functools.lru_cache(maxsize=None)
def hand_case(name, C):
    rows, kw = R.build_case(name, C)
    return rows, kw, R.soft_nms_ref_batch(as_batch(rows), **kw)


# ------------------------------------------------------------------------------------------ the contract, bit for bit
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_hand_cases(L, name):
    C = L.lib().yolo_soft_nms_onchip_rows()
    rows, kw, want = hand_case(name, C)
    check(L, rows, kw, want=want)
    count = want[1]
    if name.startswith("len_"):
        n = {"0": 0, "1": 1, "63": 63, "64": 64, "65": 65, "C-1": C - 1, "C": C, "C+1": C + 1}[name.split("_")[1]]
        assert int((as_batch(rows)[0, :, 4] > 0.25).sum()) == n              # the segment has exactly that many candidates
        assert (count[0] > 0) == (n > 0) and (n < 1000 or 20 <= count[0] <= 200)      # the long walks end early, but not at once
    if name.startswith("spill"):
        r = as_batch(rows)[0]
        pos = np.empty(len(r), np.int64)                                     # position in the segment: score descending, ties by row
        pos[np.lexsort((np.arange(len(r)), -r[:, 4].astype(np.float64)))] = np.arange(len(r))
        emitted, spilled = want[0][0, :count[0]], pos[want[0][0, :count[0]]] >= C
        rescored = bits(want[2][0, :count[0]]) != bits(r[emitted, 4])
        assert len(r) - C > 4 * 512 and spilled.sum() >= 50                  # more than one batch of spilled rows; the winners come from the spill
        assert name == "spill_hard" or (spilled & rescored).sum() >= 10      # ... with scores that were decayed there
    if name.startswith("ragged"):
        assert count[0] > 0 and count[1] == 0 and count[2] == 0
    if name.startswith("zeros"):
        zero = as_batch(rows)[0, :, 4] == 0                                  # -0.0 and +0.0 pass obj_threshold -1 and are emitted ...
        assert zero.sum() >= 26 and (name == "zeros_hard" or count[0] == 40)
        emitted = want[0][0, :count[0]]
        assert zero[emitted].any() and not np.signbit(want[2][0, :count[0]]).any()   # ... with the score +0.0
    if name == "maxdet_tie_cut":
        assert want[0][0, :5].tolist() == [1, 5, 0, 2, 4]                    # the run of 0.5 spans both classes: cut in input order
    if name in ("edge_hard", "edge_linear"):
        assert count[0] == (1 if name == "edge_hard" else 2) and (name == "edge_hard" or want[2][0, 1] == F32(0.25))
    if name == "edge_below_linear":
        assert want[2][0, 1] == F32(0.25) * (F32(1) - R.PAIR_IOU)


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_random_cases(L, seed):
    """Seeded clustered boxes under drawn options. The kernel has to give the fp32 reference's bits in every case; the fp64 yardstick
    must agree with those unless a recorded fp32 margin shows a decision on a rounding edge (tests/test_soft_nms_host.py holds the
    share of such cases under 2 % for these seeds)."""
    rows, kw = R.random_case(seed)
    r32, status = R.compare_with_fp64(rows, kw)
    assert status != "differ"
    check(L, rows, kw, want=tuple(np.asarray(a)[None] for a in r32))


# ------------------------------------------------------------------------------------------ method 0 is yolo_nms
def nms_keep(yt, rows, iou_thr, obj_thr, fmt):
    keep, count = yt.nms_indices(torch.from_numpy(np.ascontiguousarray(rows, F32)).cuda(), iou_thr, obj_thr, fmt)
    return keep.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("name", list(gi.NMS_CASES) + ["random_nc2", "random_nc80"])
def test_hard_method_is_yolo_nms(L, yt, name):
    if name in gi.NMS_CASES:
        rows, iou_thr, obj_thr, fmt = gi.nms_boxes(name)
    else:
        rows = R.clustered(np.random.default_rng(31), n=3000, copies=5, classes=2 if name.endswith("nc2") else 80)
        iou_thr, obj_thr, fmt = 0.45, 0.25, "center"
    if len(rows) == 0:
        k, c, s = yt.soft_nms(torch.zeros((1, 0, 6), device="cuda"), iou_thr, obj_thr, fmt, method="hard")
        assert c.tolist() == [0] and tuple(k.shape) == (1, 1)
        return
    keep, count, scores, _ = run_c(L, rows[None], rescore="none", iou_threshold=iou_thr, obj_threshold=obj_thr, box_format=fmt, method="hard")
    wk, wc = nms_keep(yt, rows[None], iou_thr, obj_thr, fmt)
    k = int(wc[0])
    assert count[0] == k and (name in ("empty", "one") or k > 1)
    np.testing.assert_array_equal(keep[0, :k], wk[0, :k])
    assert (keep[0, k:] == -1).all()
    np.testing.assert_array_equal(bits(scores[0, :k]), bits(rows[keep[0, :k], 4] + F32(0)))


# ------------------------------------------------------------------------------------------ rescore_rows, streams, graphs
@pytest.mark.parametrize("rescore", ["none", "separate", "boxes"])
def test_rescore_rows_variants(L, rescore):
    """NULL, a separate buffer, boxes itself: the same keep / count / scores; with boxes itself only column 4 of the emitted rows
    changes (run_c compares every other byte through the reference's rescored copy)."""
    rows, kw, want = hand_case("ties_gaussian", 4096)
    check(L, rows, kw, rescore=rescore, want=want)
    changed = bits(want[3]) != bits(as_batch(rows))
    assert changed.any() and not changed[..., [0, 1, 2, 3, 5]].any()


def test_wrapper_twice_in_one_stream_and_single_image(yt):
    """Two calls back to back share the workspace in stream order; (N, 6) input gives unbatched results; boxes is not written."""
    rows_a, kw_a, want_a = hand_case("ties_linear", 4096)
    rows_b, kw_b, want_b = hand_case("agnostic_gaussian", 4096)
    ta, tb = torch.from_numpy(rows_a).cuda(), torch.from_numpy(rows_b).cuda()
    opts = lambda kw: {k: v for k, v in kw.items() if k in yt.NMSOptions._fields}
    a = yt.soft_nms(ta, kw_a["iou_threshold"], kw_a["obj_threshold"], kw_a["box_format"], **opts(kw_a))
    b = yt.soft_nms(tb[None], kw_b["iou_threshold"], kw_b["obj_threshold"], kw_b["box_format"], **opts(kw_b))
    assert tuple(a[0].shape) == (len(rows_a),) and a[1].dim() == 0 and tuple(b[0].shape) == (1, len(rows_b))
    for got, want, sl in ((a, want_a, 0), (b, want_b, slice(None))):
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0][sl])
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1][sl])
        np.testing.assert_array_equal(bits(got[2].cpu().numpy()), bits(want[2][sl]))
    assert torch.equal(ta.cpu(), torch.from_numpy(rows_a))
    assert yt.soft_nms(ta, 0.45, 0.25, "center")[1] == yt.soft_nms(ta, 0.45, 0.25, "center", **yt.NMSOptions()._asdict())[1]


def test_one_captured_replay_equals_the_eager_call(yt):
    rows, kw, want = hand_case("ties_gaussian", 4096)
    static = torch.from_numpy(rows).cuda()[None].contiguous()
    eager = yt.soft_nms(static, 0.45, 0.25, "center")                        # also sizes the kernel's LDS outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = yt.soft_nms(static, 0.45, 0.25, "center")
    for t in out:
        t.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager)) and int(eager[1][0]) == want[1][0]


# ------------------------------------------------------------------------------------------ the nms= keyword
def test_detect_without_nms_is_unchanged_and_with_nms_rescored(yt, model):
    from oracle import net as onet
    anchors = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, 96, 96)]
    with torch.no_grad():
        preds = [p.float().contiguous() for p in model(onet.synth_input(1, 2, 96).cuda())]
    flat = torch.cat([yt.decode_boxes(p, a, mutate=False) for p, a in zip(preds, anchors)], 1)
    thr = float(torch.quantile(flat[..., 4].double().flatten(), 0.9))
    wk, wc = yt.nms_indices(flat, 0.45, thr, "center")
    for out in (yt.detect(preds, anchors, 0.45, thr), yt.detect(preds, anchors, 0.45, thr, nms=None)):
        assert torch.equal(out[0].view(torch.int32), flat.view(torch.int32)) and torch.equal(out[2], wc) and int(wc.min()) > 1
        assert all(torch.equal(out[1][b, :int(wc[b])], wk[b, :int(wc[b])]) for b in range(2))
    boxes, keep, count = yt.detect(preds, anchors, 0.45, thr, nms={"method": "gaussian"})
    sk, sc, ss = yt.soft_nms(flat, 0.45, thr, "center", method="gaussian")
    assert tuple(boxes.shape) == tuple(flat.shape) and keep.dtype == torch.int32 and tuple(keep.shape) == tuple(wk.shape)
    assert torch.equal(keep, sk) and torch.equal(count, sc) and int(count.min()) > 1
    lowered = 0
    for b in range(2):
        k = int(count[b])
        idx = keep[b, :k].long()
        assert torch.equal(boxes[b, idx, 4], ss[b, :k])                      # column 4 of the kept rows is the rescored objectness
        lowered += int((boxes[b, idx, 4] < flat[b, idx, 4]).sum())
        untouched = torch.ones(flat.shape[1], dtype=torch.bool, device="cuda")
        untouched[idx] = False
        assert torch.equal(boxes[b, untouched].view(torch.int32), flat[b, untouched].view(torch.int32))
        assert torch.equal(boxes[b, :, [0, 1, 2, 3, 5]].view(torch.int32), flat[b, :, [0, 1, 2, 3, 5]].view(torch.int32))
    assert lowered > 0
    hard = yt.detect(preds, anchors, 0.45, thr, nms=yt.NMSOptions(method="hard"))
    assert torch.equal(hard[2], wc) and all(torch.equal(hard[1][b, :int(wc[b])], wk[b, :int(wc[b])]) for b in range(2))
    via_images = yt.detect_images(model, onet.synth_input(1, 2, 96).cuda(), anchors, 0.45, thr, nms={"method": "gaussian"})
    assert torch.equal(via_images[2], count)


def test_tracker_split_follows_the_rescored_objectness(yt):
    """Two boxes of one class, 0.9 and 0.7, IoU 0.8 / 1.2 = 2/3: the Gaussian decay takes the second to 0.7 exp(-(4/9) / 0.5) = 0.29, from
    HIGH (> 0.5, and above new_threshold 0.6: it founds a track) to LOW (it can only continue one). First frame of a tracker: the
    plain boxes found two tracks, the rescored ones found one."""
    from yolo_for_turbines_amd import boxes as B
    rows = torch.tensor([[[0.5, 0.5, 0.2, 0.2, 0.9, 0.0], [0.54, 0.5, 0.2, 0.2, 0.7, 0.0]]], device="cuda")
    kw = dict(max_tracks=8, high_threshold=0.5, low_threshold=0.1, new_threshold=0.6)
    keep, count, scores = yt.soft_nms(rows, 0.45, 0.1, "center")
    assert count.tolist() == [2] and keep[0].tolist() == [0, 1] and 0.25 < float(scores[0, 1]) < 0.33
    plain = yt.Tracker(1, **kw).update(rows, keep, count)
    assert plain.count.tolist() == [2]
    rescored = rows.clone()
    k2, c2, s2 = B._soft_nms(rescored, 0.45, 0.1, "center", B._nms_options(yt.NMSOptions(), 0.1), rescored)
    assert torch.equal(k2, keep) and torch.equal(rescored[0, :, 4], scores[0]) and torch.equal(rescored[..., :4], rows[..., :4])
    res = yt.Tracker(1, **kw).update(rescored, k2, c2)
    assert res.count.tolist() == [1] and float(res.boxes[0, 0, 4]) == pytest.approx(0.9)


def test_track_images_and_detect_tiled_take_nms(yt, model):
    from oracle import net as onet
    anchors = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, 96, 96)]
    x = onet.synth_input(1, 2, 96).cuda()
    scores = yt.detect_images(model, x, anchors, 0.45, 0.0)[0][..., 4].double().flatten()
    high = float(torch.quantile(scores, 0.9))
    tracker = yt.Tracker(2, max_tracks=128, high_threshold=high, low_threshold=high / 2, new_threshold=high)
    res, boxes, keep, count = yt.track_images(model, x, anchors, tracker, iou_threshold=0.45, nms=yt.NMSOptions("gaussian", 0.5))
    want = yt.detect_images(model, x, anchors, 0.45, high / 2, nms={"method": "gaussian"})
    assert torch.equal(count, want[2]) and torch.equal(keep, want[1]) and int(count.min()) > 0 and int(res.count.sum()) > 0
    # one small frame, 2 x 2 tiles of 64
    sa = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, 64)]
    img = np.random.default_rng(5).integers(0, 256, (100, 100, 3), dtype=np.uint8)
    assert len(yt.tile_grid(100, 100, 64, 0.25)) == 4
    plain = yt.detect_tiled(model, img, sa, tile=64, overlap=0.25, obj_threshold=0.0, batch=4, max_candidates=2048)
    thr = float(torch.quantile(plain[0][0, :int(plain[3][0]), 4].double(), 0.9))
    hard = yt.detect_tiled(model, img, sa, tile=64, overlap=0.25, obj_threshold=thr, batch=4, max_candidates=2048)
    soft = yt.detect_tiled(model, img, sa, tile=64, overlap=0.25, obj_threshold=thr, batch=4, max_candidates=2048, nms={"method": "gaussian"})
    as_hard = yt.detect_tiled(model, img, sa, tile=64, overlap=0.25, obj_threshold=thr, batch=4, max_candidates=2048, nms={"method": "hard"})
    k = int(hard[2][0])
    assert k > 0 and int(as_hard[2][0]) == k and torch.equal(as_hard[1][0, :k], hard[1][0, :k]) and torch.equal(soft[3], hard[3])
    ks = int(soft[2][0])
    sk, sc, ss = yt.soft_nms(hard[0], 0.45, thr, "center")
    assert ks > 0 and ks == int(sc[0]) and torch.equal(soft[1], sk)
    assert torch.equal(soft[0][0, soft[1][0, :ks].long(), 4], ss[0, :ks])
