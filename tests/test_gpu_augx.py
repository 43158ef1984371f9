"""The augmentation extras on the MI355X (rotation, vertical flip, MixUp, Cutout: csrc/augment.h through augment.hip and crops.hip)
against the numpy restatement tests/augx_ref.py: pixels with torch.equal, boxes bit for bit after the fp32 store, counts, and zero
rows past them. Every shared case of tests/augx_cases.py runs through both ``augment_batch`` and ``CropPool.batch``
(tests/test_augx_host.py shows on the CPU that none of them compares empty box tables); then the neutral table against the calls
without ``extra``, truncation at a small ``max_out`` through the C entry points, graph capture with device tables, and the
train_batch paths."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import augx_cases as xc
from tests import augx_ref as xr

pytestmark = pytest.mark.gpu

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
           [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]
B = xc.B
CASE = {c["name"]: c for c in xc.CASES}


@pytest.fixture(scope="module")
def yt():
    import yolo_for_turbines_amd as m
    return m


@pytest.fixture(scope="module")
def pools(yt):
    return {canvas: yt.CropPool(images, boxes) for canvas, (images, boxes) in xc.POOLS.items()}


def _run(yt, pools, case, user, extra="case", **kw):
    """The call of ``user`` on a case: (x, boxes, counts). extra: "case" (the case's host table), None, or a table."""
    images, boxes = xc.POOLS[case["canvas"]]
    if isinstance(extra, str):
        extra = torch.as_tensor(case["extra"])
    if user == "augment":
        return yt.augment_batch(images, boxes, case["canvas"], params=torch.as_tensor(case["params"]), mosaic=case["mosaic"],
                                extra=extra, **kw)
    return pools[case["canvas"]].batch(B, case["canvas"], index=torch.tensor(case["index"], dtype=torch.int32),
                                       crop_params=torch.as_tensor(case["cp"]), params=torch.as_tensor(case["params"]), extra=extra,
                                       **kw)[:3]


def _equal_ref(got, ref, what):
    x, bt, ct = got[:3]
    rx, rb = ref
    assert torch.equal(x.cpu(), torch.from_numpy(rx)), f"{what}: pixels differ from augx_ref"
    ct, bt = ct.cpu(), bt.cpu()
    for b in range(len(rb)):
        assert int(ct[b]) == len(rb[b]), f"{what}: count of row {b}: {int(ct[b])}, augx_ref has {len(rb[b])}"
        assert np.array_equal(bt[b, :len(rb[b])].numpy(), np.asarray(rb[b], np.float32).reshape(-1, 5)), f"{what}: boxes of row {b}"
        assert not bt[b, len(rb[b]):].any(), f"{what}: rows past the count of row {b} are not zero"


@pytest.mark.parametrize("user", ["augment", "crop"])
@pytest.mark.parametrize("name", list(CASE))
def test_cases_equal_restatement(yt, pools, name, user):
    case = CASE[name]
    got = _run(yt, pools, case, user)
    _equal_ref(got, xc.reference(case, user), f"{name} / {user}")
    if case["kind"] == "neutral":                             # today's outputs bit for bit; only the box table is wider
        x0, b0, c0 = _run(yt, pools, case, user, extra=None)
        M = b0.shape[1]
        assert torch.equal(got[0], x0) and torch.equal(got[2], c0) and torch.equal(got[1][:, :M], b0) and not got[1][:, M:].any()
        assert int(c0.sum()) > 0


def test_box_table_sizes(yt, pools):
    case = CASE["mix_mutual"]
    images, boxes = xc.POOLS[case["canvas"]]
    own = [sum(len(boxes[k]) for k in r if k >= 0 and boxes[k]) for r in case["mosaic"].tolist()]
    pt = [xr.partner(case["extra"][b], b, B) for b in range(B)]
    exact = max(own[b] + (own[pt[b]] if pt[b] >= 0 else 0) for b in range(B))
    assert _run(yt, pools, case, "augment")[1].shape == (B, exact, 5)                       # a host table: the exact sum
    dev = _run(yt, pools, case, "augment", extra=torch.as_tensor(case["extra"]).cuda())
    assert dev[1].shape == (B, 2 * max(own), 5)
    _equal_ref(dev, xc.reference(case, "augment"), "device extras / augment")
    pool = pools[case["canvas"]]
    assert _run(yt, pools, case, "crop")[1].shape == (B, 2 * pool.max_boxes, 5)
    assert _run(yt, pools, case, "crop", extra=None)[1].shape == (B, pool.max_boxes, 5)     # shapes change only with extra


def test_truncation_at_max_out_crop_entry(yt, pools):
    from yolo_for_turbines_amd import _lib as L
    case = CASE["mix_mutual"]
    H, W = case["canvas"]
    images, boxes = xc.POOLS[case["canvas"]]
    pool = pools[case["canvas"]]
    full = xc.reference(case, "crop")[1]
    idx = torch.tensor(case["index"], dtype=torch.int32).cuda()
    cp, p, e = (torch.as_tensor(case[k]).cuda() for k in ("cp", "params", "extra"))
    for max_out in (1, 3):
        assert max(len(r) for r in full) > max_out
        ob = torch.full((B, max_out, 5), -1.0, device="cuda")
        ct = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        win = torch.empty((B, 6), dtype=torch.int32, device="cuda")
        L.check(L.lib().yolo_crop_boxes_ex(pool.boxes.data_ptr(), pool.nbox.data_ptr(), pool.max_boxes, pool.hw.data_ptr(), len(pool),
                                           idx.data_ptr(), cp.data_ptr(), None, p.data_ptr(), e.data_ptr(), B, H, W, 0.4, ob.data_ptr(),
                                           ct.data_ptr(), max_out, win.data_ptr(), L.current_stream()), "yolo_crop_boxes_ex")
        want = xr.crop(images, boxes, case["index"], case["cp"], case["params"], case["extra"], H, W, max_out=max_out)[1]
        assert [len(r) for r in want] == [min(len(r), max_out) for r in full]
        _equal_ref((torch.from_numpy(xc.reference(case, "crop")[0]), ob, ct), (xc.reference(case, "crop")[0], want), f"max_out {max_out}")


def test_truncation_at_max_out_augment_entry(yt):
    from yolo_for_turbines_amd import _lib as L
    case = CASE["mix_chain"]                                  # standard rows only: src[b] = {image, -1, -1, -1}
    H, W = case["canvas"]
    images, boxes = xc.POOLS[case["canvas"]]
    n, max_in = len(images), max(len(b or []) for b in boxes)
    tab = np.zeros((n, max_in, 5))
    for i, bl in enumerate(boxes):
        if bl:
            tab[i, :len(bl)] = bl
    nbox = [-1 if b is None else len(b) for b in boxes]
    hw = [v for im in images for v in im.shape[:2]]
    src = [int(v) for r in case["mosaic"] for v in r]
    d_tab, d_p, d_e = (torch.as_tensor(t).cuda() for t in (tab, case["params"], case["extra"]))
    d_nbox, d_hw, d_src = (torch.tensor(t, dtype=torch.int32).cuda() for t in (nbox, hw, src))
    full = xc.reference(case, "augment")[1]
    for max_out in (2, 6):
        assert max(len(r) for r in full) > max_out
        ob = torch.full((B, max_out, 5), -1.0, device="cuda")
        ct = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        sel = torch.empty((B,), dtype=torch.int32, device="cuda")
        L.check(L.lib().yolo_augment_boxes_ex(d_tab.data_ptr(), d_nbox.data_ptr(), max_in, d_hw.data_ptr(), d_src.data_ptr(),
                                              (C.c_int32 * len(hw))(*hw), n, (C.c_int32 * len(src))(*src), d_p.data_ptr(), d_e.data_ptr(),
                                              B, H, W, ob.data_ptr(), ct.data_ptr(), max_out, sel.data_ptr(), L.current_stream()),
                "yolo_augment_boxes_ex")
        want = xr.augment(images, boxes, case["params"], case["extra"], H, W, case["mosaic"], max_out=max_out)[1]
        assert [len(r) for r in want] == [min(len(r), max_out) for r in full]
        rx = xc.reference(case, "augment")[0]
        _equal_ref((torch.from_numpy(rx), ob, ct), (rx, want), f"max_out {max_out}")
        assert sel.tolist() == [-1, -1, -1, -2]               # the paths of the rows' own images


def _captured(first, again, tables, second):
    """Warm up on a side stream, capture ``again`` (the call with out=), replay; copy ``second`` into the device tables, replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = first()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        again(out)
    results = []
    for step in range(2):
        if step:
            for t, v in zip(tables, second):
                t.copy_(torch.as_tensor(v))
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        results.append([t.clone() for t in out])
    return results


def test_capture_crop_with_device_extras(yt, pools):
    a, b = CASE["all_32"], CASE["cut_32"]                     # same canvas and pool; every table differs
    pool = pools[a["canvas"]]
    d_idx = torch.tensor(a["index"], dtype=torch.int32).cuda()
    d_cp, d_p, d_e = (torch.as_tensor(a[k]).cuda() for k in ("cp", "params", "extra"))
    kw = dict(index=d_idx, crop_params=d_cp, params=d_p, extra=d_e)
    r0, r1 = _captured(lambda: pool.batch(B, a["canvas"], **kw), lambda out: pool.batch(B, a["canvas"], out=out, **kw),
                       (d_idx, d_cp, d_p, d_e), (torch.tensor(b["index"], dtype=torch.int32), b["cp"], b["params"], b["extra"]))
    for res, case in ((r0, a), (r1, b)):
        eager = _run(yt, pools, case, "crop")
        assert all(torch.equal(u, v) for u, v in zip(res[:3], eager)), case["name"]
        _equal_ref(res, xc.reference(case, "crop"), f"replay of {case['name']}")


def test_capture_augment_with_device_extras(yt, pools):
    from yolo_for_turbines_amd.data import _augment_prepare
    a, b = CASE["all_32"], CASE["cut_32"]
    assert a["canvas"] == b["canvas"]
    images, boxes = xc.POOLS[a["canvas"]]
    d_p, d_e = torch.as_tensor(a["params"]).cuda(), torch.as_tensor(a["extra"]).cuda()
    x, ob, ct, launch = _augment_prepare(images, boxes, a["canvas"], d_p, None, a["mosaic"], None, d_e)
    r0, r1 = _captured(lambda: (launch(), (x, ob, ct))[1], lambda out: launch(), (d_p, d_e), (a["params"], b["extra"]))
    _equal_ref(r0, xc.reference(a, "augment"), "replay of all_32")
    mixed = dict(a, extra=b["extra"])                         # the rows and params of all_32 under the extras of cut_32
    want = xr.augment(images, boxes, mixed["params"], mixed["extra"], *a["canvas"], mixed["mosaic"])
    _equal_ref(r1, want, "replay after the extras were rewritten")
    assert any(want[1]) and not torch.equal(r0[0], r1[0])
    eager = yt.augment_batch(images, boxes, a["canvas"], params=d_p, mosaic=a["mosaic"], extra=d_e)
    assert all(torch.equal(u, v) for u, v in zip(r1, eager))


def test_train_batch_targets(yt, pools):
    case = CASE["all_32"]
    S = case["canvas"][0]
    images, boxes = xc.POOLS[case["canvas"]]
    anc = torch.tensor(ANCHORS).cuda()
    for user in ("augment", "crop"):
        rx, rb = xc.reference(case, user)
        M = max(len(r) for r in rb)
        assert M > 0
        tab = np.zeros((B, M, 5), np.float32)
        for b, rows in enumerate(rb):
            tab[b, :len(rows)] = np.asarray(rows, np.float32).reshape(-1, 5)
        want = yt.build_targets(torch.from_numpy(tab).cuda(), anc, S, counts=torch.tensor([len(r) for r in rb], dtype=torch.int32).cuda())
        if user == "augment":
            x, t = yt.train_batch(images, boxes, anc, S, params=torch.as_tensor(case["params"]), mosaic=case["mosaic"],
                                  extra=torch.as_tensor(case["extra"]))
        else:
            x, t = pools[case["canvas"]].train_batch(B, anc, S, index=torch.tensor(case["index"], dtype=torch.int32),
                                                     crop_params=torch.as_tensor(case["cp"]), params=torch.as_tensor(case["params"]),
                                                     extra=torch.as_tensor(case["extra"]))
        assert torch.equal(x.cpu(), torch.from_numpy(rx)), user
        assert all(torch.equal(u, v) for u, v in zip(t, want)) and any(bool(v.any()) for v in want), user


def test_argument_errors(yt, pools):
    case = CASE["neutral_32"]
    pool = pools[case["canvas"]]
    with pytest.raises(ValueError, match="extra .* was given with augment=False"):
        pool.batch(B, 32, extra=xr.neutral(B), augment=False)
    with pytest.raises(ValueError, match=r"extra must have shape \(4, 24\)"):
        _run(yt, pools, case, "crop", extra=xr.neutral(B + 1))
    with pytest.raises(ValueError, match=r"extra must have shape \(4, 24\)"):
        _run(yt, pools, case, "augment", extra=xr.neutral(B)[:, :23])
    bad = xr.neutral(B)
    bad[2, xr.CUT_N] = 5.0
    for user in ("augment", "crop"):
        with pytest.raises(ValueError, match="CUT_N must be an integer"):
            _run(yt, pools, case, user, extra=bad)
    with pytest.raises(ValueError, match="device table must be a contiguous torch.float64"):
        _run(yt, pools, case, "crop", extra=torch.as_tensor(xr.neutral(B)).float().cuda())
