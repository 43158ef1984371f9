"""yolo_fuse_boxes / fuse_boxes on the GPU, bit for bit against the numpy restatement of its contract (tests/fuse_ref.py): fused
rows, members, count, assign and the zero rows behind count, with the output buffers pre-filled with 0xA5 and guard bytes behind
them."""
import numpy as np
import pytest
import torch

from tests import fuse_ref as R

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


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def filled(nbytes, value=0xA5):
    return torch.full((nbytes + SPARE,), value, dtype=torch.uint8, device="cuda")


def run_c(L, boxes, iou_threshold=0.55, obj_threshold=0.0, box_format="center", n_views=0, conf_type="avg", class_agnostic=False,
          want_assign=True):
    """yolo_fuse_boxes through the C ABI into 0xA5-filled buffers; checks the guard bytes; returns numpy arrays."""
    boxes = np.ascontiguousarray(boxes, F32)
    B, N, _ = boxes.shape
    lib = L.lib()
    d_boxes = torch.from_numpy(boxes).cuda()
    sizes = [B * N * 24, B * N * 4, B * 4, B * N * 4]
    bufs = [filled(s) for s in sizes]
    nbytes = lib.yolo_fuse_workspace_bytes(B, N)
    assert nbytes > 0
    ws = filled(nbytes, 0x5A)
    rc = lib.yolo_fuse_boxes(d_boxes.data_ptr(), B, N, float(iou_threshold), float(obj_threshold), int(box_format == "center"),
                             int(class_agnostic), int(n_views), {"avg": 0, "max": 1}[conf_type], bufs[0].data_ptr(), bufs[1].data_ptr(),
                             bufs[2].data_ptr(), bufs[3].data_ptr() if want_assign else None, ws.data_ptr(), nbytes,
                             torch.cuda.current_stream().cuda_stream)
    L.check(rc, "yolo_fuse_boxes")
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs + [ws]]
    for h, s in zip(host, sizes + [nbytes]):
        guard = h[s:]
        assert (guard == guard[0]).all() and guard[0] in (0xA5, 0x5A), "wrote behind a buffer"
    if not want_assign:
        assert (host[3] == 0xA5).all()
    fused = host[0][:sizes[0]].view(F32).reshape(B, N, 6)
    members = host[1][:sizes[1]].view(np.int32).reshape(B, N)
    count = host[2][:sizes[2]].view(np.int32)
    assign = host[3][:sizes[3]].view(np.int32).reshape(B, N)
    return fused, members, count, assign


def check(L, boxes, **kw):
    boxes = np.asarray(boxes, F32)
    if boxes.ndim == 2:
        boxes = boxes[None]
    got = run_c(L, boxes, **kw)
    want = R.fuse_ref_batch(boxes, **kw)
    np.testing.assert_array_equal(got[2], want[2])                       # count
    np.testing.assert_array_equal(got[1], want[1])                       # members, zeros behind count
    np.testing.assert_array_equal(got[3], want[3])                       # assign
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))           # fused rows and the zero rows behind them, by bits
    return want


# ------------------------------------------------------------------------------------------ generators
def disjoint(k, rng, cls=0.0, copies=1, jitter=0.0):
    """k objects on a grid of 0.02 x 0.02 boxes with 0.03 pitch (no two objects touch), `copies` reports each, shuffled."""
    side = int(np.ceil(np.sqrt(k)))
    idx = np.arange(k)
    rows = np.zeros((k, copies, 6))
    rows[..., 0] = (0.03 * (idx % side) + 0.015)[:, None] + rng.uniform(-jitter, jitter, (k, copies))
    rows[..., 1] = (0.03 * (idx // side) + 0.015)[:, None] + rng.uniform(-jitter, jitter, (k, copies))
    rows[..., 2] = rows[..., 3] = 0.02
    rows[..., 4] = rng.uniform(0.1, 1.0, (k, copies))
    rows[..., 5] = cls
    rows = rows.reshape(-1, 6)
    return rows[rng.permutation(len(rows))].astype(F32)


def one_cluster(members, rng):
    rows = np.zeros((members, 6))
    rows[:, 0] = 0.5 + rng.uniform(-0.002, 0.002, members)
    rows[:, 1] = 0.4 + rng.uniform(-0.002, 0.002, members)
    rows[:, 2], rows[:, 3] = 0.2, 0.3
    rows[:, 4] = rng.uniform(0.1, 1.0, members)
    rows[:, 5] = 1.0
    return rows.astype(F32)


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
@pytest.mark.parametrize("fmt", ["corners", "center"])
def test_hand_cases(L, case, fmt):
    _, rows, kw, want_rows, want_members, _ = case
    rows = np.array(rows, F32) if fmt == "corners" else R.to_center(rows)
    want = check(L, rows, box_format=fmt, **kw)
    exp = np.array(want_rows, F32) if fmt == "corners" else R.to_center(want_rows)
    assert want[2][0] == len(exp) and np.array_equal(want[0][0, :len(exp)], exp)      # the reference gives the literals here too


def test_threshold_edge(L):
    a, b = R.HAND_CASES[0][1]
    one = F32(1)
    iou = (F32(0.625) * one) / (((one + F32(0.625)) - F32(0.625)) + F32(1e-6))
    rows = np.array([a, b], F32)
    assert check(L, rows, iou_threshold=float(iou), box_format="corners")[2][0] == 2
    assert check(L, rows, iou_threshold=float(np.nextafter(iou, F32(0))), box_format="corners")[2][0] == 1


def test_empty_and_trivial(L):
    got = run_c(L, np.zeros((2, 0, 6), F32))
    assert got[2].tolist() == [0, 0]
    assert check(L, [[0.5, 0.5, 0.2, 0.2, 0.7, 3.0]])[2][0] == 1                          # one candidate
    rows = R.clustered(np.random.default_rng(2), 50)
    assert check(L, rows, obj_threshold=1.0)[2][0] == 0                                   # all rows filtered
    with_assign, without = run_c(L, rows[None]), run_c(L, rows[None], want_assign=False)      # assign = NULL is allowed
    assert all(np.array_equal(a, b) for a, b in zip(with_assign[:3], without[:3]))


@pytest.mark.parametrize("k", [63, 64, 65, 127, 128, 129, "cap-1", "cap", "cap+1"])
@pytest.mark.parametrize("agnostic", [False, True])
def test_clusters_per_segment(L, k, agnostic):
    """Disjoint boxes of one class: every candidate founds a cluster, so the segment has k clusters and k candidates - around the
    lanes of a wave, the prefetch chunk and the on-chip capacity (the cluster behind it lives in the workspace)."""
    cap, chunk = L.lib().yolo_fuse_onchip_clusters(), L.lib().yolo_fuse_chunk_candidates()
    assert chunk == 64, "the sizes above straddle a 64-candidate chunk"
    if isinstance(k, str):
        k = cap + {"cap-1": -1, "cap": 0, "cap+1": 1}[k]
    rows = disjoint(k, np.random.default_rng(k))
    assert check(L, rows, class_agnostic=agnostic)[2][0] == k


@pytest.mark.parametrize("agnostic", [False, True])
def test_spilled_clusters_take_members(L, agnostic):
    """More clusters than the on-chip capacity, three jittered reports each: clusters in the workspace are matched and updated."""
    cap = L.lib().yolo_fuse_onchip_clusters()
    rows = disjoint(cap + 40, np.random.default_rng(9), copies=3, jitter=0.001)
    want = check(L, rows, class_agnostic=agnostic, n_views=4)
    assert want[2][0] == cap + 40 and (want[1][0, :cap + 40] == 3).all()


@pytest.mark.parametrize("members", [1, 64, 65, 300])
def test_one_cluster(L, members):
    want = check(L, one_cluster(members, np.random.default_rng(members)))
    assert want[2][0] == 1 and want[1][0, 0] == members


def test_ragged_batch_with_an_empty_image(L):
    rng = np.random.default_rng(4)
    boxes = np.stack([R.clustered(rng, 200) for _ in range(3)])
    boxes[0, 150:] = 0                       # zero rows behind a caller's boxes
    boxes[1, :, 4] *= 0.2                    # nothing above the threshold
    want = check(L, boxes, obj_threshold=0.3)
    assert want[2][1] == 0 and want[2][0] > 0 and want[2][2] > 0 and want[2][0] != want[2][2]


@pytest.mark.parametrize("classes", [2, 80])
@pytest.mark.parametrize("n", [480, 4096])
def test_clustered(L, n, classes):
    want = check(L, R.clustered(np.random.default_rng(5), n, classes=classes), obj_threshold=0.3)
    assert n // 24 < want[2][0] < n // 2


@pytest.mark.parametrize("n_views", [0, 1, 4])
@pytest.mark.parametrize("conf_type", ["avg", "max"])
@pytest.mark.parametrize("agnostic", [False, True])
def test_options(L, n_views, conf_type, agnostic):
    rows = R.clustered(np.random.default_rng(6), 480, classes=3)
    check(L, rows[None].repeat(2, 0), obj_threshold=0.2, n_views=n_views, conf_type=conf_type, class_agnostic=agnostic, box_format="center")


def test_corner_format_on_clustered(L):
    rows = R.clustered(np.random.default_rng(8), 480)
    rows[:, 0] -= rows[:, 2] / 2
    rows[:, 1] -= rows[:, 3] / 2
    check(L, rows, obj_threshold=0.3, box_format="corners")


def test_lumped_classes_share_the_bucket_but_no_cluster(L):
    """Classes that are no integers in [0, 4094) are ordered together (bucket 4094) and still merge by float equality only."""
    rng = np.random.default_rng(12)
    cls = [4094.0, 5000.0, 2.5, 2.5, 4094.0, -1.0, 5000.0, 2.5, 7.0, 4093.0, 4093.0]
    rows = one_cluster(len(cls), rng)
    rows[:, 5] = cls
    want = check(L, rows)
    assert want[2][0] == 6 and sorted(want[1][0, :6].tolist()) == [1, 1, 2, 2, 2, 3]
    assert check(L, rows, class_agnostic=True)[2][0] == 1


def test_wrapper_twice_in_one_stream(L, yt):
    """fuse_boxes twice without a synchronisation between them: different inputs, the same cached workspace."""
    a = np.stack([R.clustered(np.random.default_rng(20), 700, classes=4), R.clustered(np.random.default_rng(21), 700, classes=4)])
    b = R.clustered(np.random.default_rng(22), 300)
    ra = yt.fuse_boxes(torch.from_numpy(a).cuda(), 0.55, 0.3, n_views=2, return_assign=True)
    rb = yt.fuse_boxes(torch.from_numpy(b).cuda(), 0.5, 0.1, conf_type="max", class_agnostic=True, return_assign=True)
    wa = R.fuse_ref_batch(a, iou_threshold=0.55, obj_threshold=0.3, n_views=2)
    wb = R.fuse_ref(b, 0.5, 0.1, conf_type="max", class_agnostic=True)
    fused, count, members, assign = (t.cpu().numpy() for t in ra)
    assert fused.shape == (2, 700, 6) and count.dtype == np.int32 and members.dtype == np.int32
    np.testing.assert_array_equal(bits(fused), bits(wa[0]))
    np.testing.assert_array_equal(members, wa[1])
    np.testing.assert_array_equal(count, wa[2])
    np.testing.assert_array_equal(assign, wa[3])
    fused, count, members, assign = (t.cpu().numpy() for t in rb)         # (N, 6) in: no batch axis out
    assert fused.shape == (300, 6) and count.shape == () and members.shape == (300,)
    np.testing.assert_array_equal(bits(fused), bits(wb[0]))
    np.testing.assert_array_equal(members, wb[1])
    assert int(count) == wb[2]
    np.testing.assert_array_equal(assign, wb[3])
    assert len(yt.fuse_boxes(torch.from_numpy(b).cuda())) == 3
    # a fused result is input for another fusion and for the NMS: zero rows never pass a threshold >= 0
    again = yt.fuse_boxes(ra[0], 0.55, 0.0)
    assert int(again[1][0]) <= int(ra[1][0]) and int(again[1][0]) > 0
    keep, kc = yt.nms_indices(ra[0], 0.45, 0.0, "center")
    assert 0 < int(kc[0]) <= int(ra[1][0])


def test_limits(L):
    lib = L.lib()
    one = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = lib.yolo_fuse_boxes(one.data_ptr(), 1, 163457, 0.5, 0.0, 1, 0, 0, 0, one.data_ptr(), one.data_ptr(), one.data_ptr(), None,
                             one.data_ptr(), 1 << 40, None)
    assert rc != 0 and b"too large" in lib.yolo_last_error()
    rc = lib.yolo_fuse_boxes(one.data_ptr(), 1, 100, 0.5, 0.0, 1, 0, 0, 0, one.data_ptr(), one.data_ptr(), one.data_ptr(), None,
                             one.data_ptr(), 16, None)
    assert rc != 0 and b"workspace" in lib.yolo_last_error()
    rc = lib.yolo_fuse_boxes(one.data_ptr(), 1, 100, 0.5, 0.0, 1, 0, 0, 2, one.data_ptr(), one.data_ptr(), one.data_ptr(), None,
                             one.data_ptr(), 1 << 40, None)
    assert rc != 0
    torch.cuda.synchronize()


def test_fuses_the_candidates_of_detect_tiled(L, yt):
    """The two small frames of the pyramid test's end-to-end case: detect_tiled's candidates, fused class-aware and class-agnostic,
    equal the reference on the same candidates. The threshold lies between two scores (the rule of that test's _pick_threshold)."""
    from tests import test_gpu_tiles_pyramid as P
    m = P._model(yt)
    cand, _, _, ncand = yt.detect_tiled(m, P._images(), P._anchors(yt), tile=(P.TH, P.TW), overlap=P.OVERLAP, obj_threshold=0.0,
                                        batch=P.BATCH, max_candidates=8192, scales=(1.0, 0.5))
    host = cand.cpu().numpy()
    assert all(0 < n < 8192 for n in ncand.tolist())
    per_image = [host[f, :n, 4].astype(np.float64) for f, n in enumerate(ncand.tolist())]
    q = min(np.quantile(s, 0.9, method="lower") for s in per_image)
    scores = np.unique(np.concatenate(per_image))
    thr = float((q + scores[scores > q][0]) / 2)
    assert q < thr < scores[scores > q][0] and not (scores == thr).any()
    for agnostic in (False, True):
        fused, count, members, assign = yt.fuse_boxes(cand, 0.55, thr, class_agnostic=agnostic, return_assign=True)
        want = R.fuse_ref_batch(host, iou_threshold=0.55, obj_threshold=thr, class_agnostic=agnostic)
        print("threshold", thr, "candidates", [(a >= 0).sum() for a in want[3]], "fused", want[2].tolist())
        assert (want[2] > 0).all()
        np.testing.assert_array_equal(bits(fused.cpu().numpy()), bits(want[0]))
        np.testing.assert_array_equal(members.cpu().numpy(), want[1])
        np.testing.assert_array_equal(count.cpu().numpy(), want[2])
        np.testing.assert_array_equal(assign.cpu().numpy(), want[3])
