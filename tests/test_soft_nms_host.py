"""Soft-NMS on the host: the numpy reference (tests/soft_nms_ref.py) against the NMS oracle and against its own per-class walk, w(t)
against fp64 exp, the random cases of the GPU test against the fp64 yardstick, the C entry's host-only queries and argument errors,
and the Python options. No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import postprocess as opp
from tests import golden_inputs as gi
from tests import soft_nms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ERR_ARG, ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib.lib()



# ---- the reference
@pytest.mark.parametrize("name", list(gi.NMS_CASES))
def test_hard_method_is_the_nms_oracle(name):
    """Method 0 with nothing else set keeps what non_max_suppression keeps, in its order, on every golden NMS case."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "nms.npz"))
    boxes, iou_thr, obj_thr, fmt = gi.nms_boxes(name)
    keep, count, scores, rescored = R.soft_nms_ref(boxes, iou_thr, obj_thr, box_format=fmt, method="hard")
    want = g[f"{name}/keep"]
    assert count == len(want)
    np.testing.assert_array_equal(keep[:count], want)
    # tests/golden/nms.npz is that oracle's recorded output (tests/gen_golden.py; tests/test_oracle_golden.py holds oracle.postprocess
    # .nms_indices and its C twin to it on every case); the live numpy oracle is called again here where it is quick
    if len(want) <= 3000:
        np.testing.assert_array_equal(keep[:count], opp.nms_indices(boxes.tolist(), iou_thr, obj_thr, fmt))
    assert (keep[count:] == -1).all() and not scores[count:].any()
    np.testing.assert_array_equal(scores[:count], boxes[want, 4] + F32(0))
    np.testing.assert_array_equal(rescored, boxes)                # hard removal rescored nothing


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("max_det", [None, 7])
def test_emission_order_and_segment_walks(method, agnostic, max_det):
    """Scores only fall and the walk takes the maximum: the emitted scores never rise, equal ones come in input order, and the
    per-class walks merged by (score, row) ARE the global loop - with ties and duplicates, the case that would tell them apart."""
    for seed in (11, 12, 13):
        rows = R.tied_boxes(seed)
        kw = dict(iou_threshold=0.4, obj_threshold=0.2, box_format="center", method=method, sigma=0.5, class_agnostic=agnostic, max_det=max_det)
        keep, count, scores, rescored = R.soft_nms_ref(rows, **kw)
        assert count > 3 and (max_det is None or count == max_det)
        s = scores[:count]
        assert (np.diff(s) <= 0).all()
        same = np.diff(s) == 0
        assert same.any() and (np.diff(keep[:count])[same] > 0).all()
        assert len(set(keep[:count].tolist())) == count
        k2, c2, s2, r2 = R.soft_nms_ref_segments(rows, **kw)
        assert c2 == count
        np.testing.assert_array_equal(k2, keep)
        np.testing.assert_array_equal(s2.view(np.int32), scores.view(np.int32))
        np.testing.assert_array_equal(r2.view(np.int32), rescored.view(np.int32))
        np.testing.assert_array_equal(rescored[keep[:count], 4], s)


def test_hand_worked_pair():
    """The unit square (0.5) and its right 5/8 (0.25), corner format: inter = 0.625, iou = 0.625 / (1 + 1e-6) in fp32."""
    rows = np.array([[0, 0, 1, 1, 0.5, 0], [0.375, 0, 0.625, 1, 0.25, 0]], F32)
    one = F32(1)
    iou = F32(0.625) / (((one + F32(0.625)) - F32(0.625)) + F32(1e-6))
    assert iou.dtype == F32
    k, c, s, _ = R.soft_nms_ref(rows, 0.5, 0.1, method="hard")
    assert (c, k.tolist()) == (1, [0, -1])
    k, c, s, _ = R.soft_nms_ref(rows, 0.5, 0.1, method="linear", score_threshold=0.05)
    assert c == 2 and s[1] == F32(0.25) * (one - iou)
    k, c, s, _ = R.soft_nms_ref(rows, 0.5, 0.1, method="linear")                   # 0.09375 fails the final threshold 0.1
    assert c == 1
    k, c, s, r = R.soft_nms_ref(rows, 0.5, 0.1, method="gaussian", sigma=0.5)
    want = F32(0.25) * R.w_ref((iou * iou) / F32(0.5))
    assert c == 2 and s[1] == want and r[1, 4] == want and abs(float(want) - 0.25 * math.exp(-0.625 ** 2 / 0.5)) < 1e-6
    # the threshold edge: thr == the fp32 IoU itself - hard removes (!(iou < thr)), linear leaves (iou > thr is false)
    assert R.soft_nms_ref(rows, float(iou), 0.1, method="hard")[1] == 1
    k, c, s, _ = R.soft_nms_ref(rows, float(iou), 0.1, method="linear")
    assert c == 2 and s[1] == F32(0.25)
    # another class does not interact unless class_agnostic
    rows[1, 5] = 1
    assert R.soft_nms_ref(rows, 0.5, 0.1, method="hard")[1] == 2
    assert R.soft_nms_ref(rows, 0.5, 0.1, method="hard", class_agnostic=True)[1] == 1


# ---- w(t)
def test_w_against_fp64_exp():
    """Step 4 of the contract: on 200,001 grid points of [0, 100] and on 100,000 random points of [0, 4] (every t = iou^2 / sigma the
    GPU tests produce is checked there, from the same function), 0 <= w <= 1, w(0) == 1, w == 0 beyond the underflow point, NaN
    stays NaN, and wherever w is at least the smallest normal it is within 1e-6 of exp(-t), relatively."""
    t = np.concatenate([np.linspace(0, 100, 200001), np.random.default_rng(0).uniform(0, 4, 100000)]).astype(F32)
    err = check_w(t)
    print("w(t) against exp(-t): max relative error %.3e" % err)
    assert R.w_ref(F32(0)) == F32(1) and R.w_ref(F32(88)) == 0 and R.w_ref(F32(np.inf)) == 0
    assert np.isnan(R.w_ref(F32(np.nan)))
    assert np.array_equal(R.w_ref(np.array([0.0, 1.0], F32)), np.array([R.w_ref(F32(0)), R.w_ref(F32(1))]))


def test_w_on_every_argument_the_gpu_tests_produce(lib):
    """Every t = fl(fl(iou iou) / sigma) of the Gaussian cases of tests/test_gpu_soft_nms.py (hand cases and random cases, from the
    same builders) meets the conditions of step 4."""
    C = lib.yolo_soft_nms_onchip_rows()
    ts = []
    cases = [R.build_case(n, C) for n in R.CASE_NAMES] + [R.random_case(s) for s in R.RANDOM_SEEDS]
    for rows, kw in cases:
        if kw["method"] != "gaussian":
            continue
        for img in (rows if rows.ndim == 3 else rows[None]):
            mg = R.new_margins()
            R.soft_nms_ref(img, margins=mg, **kw)
            ts += mg["t"]
    assert len(ts) > 10000
    print("%d arguments, max relative error %.3e" % (len(ts), check_w(np.array(ts, F32))))


def check_w(t):
    """The conditions of step 4 on the fp32 points ``t``; returns the largest relative error."""
    t = np.asarray(t, F32)
    w = R.w_ref(t)
    assert w.dtype == F32 and (w >= 0).all() and (w <= 1).all()
    normal = w >= np.finfo(F32).tiny
    assert not w[~normal].any()                                   # below the smallest normal there is only 0
    e = np.exp(-t[normal].astype(np.float64))
    err = float(np.max(np.abs(w[normal].astype(np.float64) - e) / e)) if normal.any() else 0.0
    assert err <= 1e-6
    return err


def test_random_cases_stay_clear_of_rounding_edges():
    """The seeded random cases of tests/test_gpu_soft_nms.py, fp32 walk against fp64 walk: none may differ with clear margins, and
    at most 2 % may be set aside because a recorded margin shows a decision on a rounding edge."""
    status = [R.compare_with_fp64(*R.random_case(seed))[1] for seed in R.RANDOM_SEEDS]
    assert "differ" not in status
    assert len(R.RANDOM_SEEDS) >= 50 and status.count("edge") <= 0.02 * len(status)
    methods = {R.random_case(seed)[1]["method"] for seed in R.RANDOM_SEEDS}
    assert methods == {"hard", "linear", "gaussian"}


# ---- the C entry without a device
def test_header_declares_the_exports_and_host_queries_work(lib):
    from yolo_for_turbines_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    for name in ("yolo_soft_nms_onchip_rows", "yolo_soft_nms_workspace_bytes", "yolo_soft_nms"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    rows = lib.yolo_soft_nms_onchip_rows()
    assert rows >= 64 and rows % 64 == 0 and rows * 28 <= 160 * 1024      # 28 bytes of LDS a row, inside the 160 KiB of a CU
    small, big = lib.yolo_soft_nms_workspace_bytes(1, 100), lib.yolo_soft_nms_workspace_bytes(16, 10000)
    assert 0 < small < big and big > 16 * 10000 * (8 + 8 + 32 + 12)
    assert lib.yolo_soft_nms_workspace_bytes(1, 163456) > 0 and lib.yolo_soft_nms_workspace_bytes(1, 163457) == 0
    assert lib.yolo_soft_nms_workspace_bytes(2047, 1) > 0 and lib.yolo_soft_nms_workspace_bytes(2048, 1) == 0
    assert lib.yolo_soft_nms_workspace_bytes(0, 10) == 0 and lib.yolo_soft_nms_workspace_bytes(1, -1) == 0
    assert lib.yolo_soft_nms_workspace_bytes(1, 0) > 0
    # the header's constants are the reference's: w(t) is restated from the same text
    for c in ("0x1.715476p+0f", "0x1.63p-1f", "-0x1.bd0106p-13f", "-0x1.a01a02p-13f", "0x1.6c16c2p-10f", "-0x1.111112p-7f",
              "0x1.555556p-5f", "-0x1.555556p-3f"):
        assert c in hdr, c


BOXES, KEEP, COUNT, SCORES, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000     # never dereferenced: refused before any launch
GOOD = dict(boxes=BOXES, b=1, n=10, iou=0.45, obj=0.25, score=0.25, center=1, method=2, sigma=0.5, agnostic=0, max_det=0, keep=KEEP,
            count=COUNT, scores=SCORES, rescore=None, ws=WS, ws_bytes=1 << 30, stream=None)
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("change,code,word", [
    (dict(boxes=None), ERR_ARG, "null"), (dict(keep=None), ERR_ARG, "null"), (dict(count=None), ERR_ARG, "null"),
    (dict(scores=None), ERR_ARG, "null"),
    (dict(b=-1), ERR_ARG, "negative"), (dict(n=-1), ERR_ARG, "negative"),
    (dict(method=-1), ERR_ARG, "method"), (dict(method=3), ERR_ARG, "method"), (dict(max_det=-1), ERR_ARG, "max_det"),
    (dict(iou=NAN), ERR_ARG, "iou_threshold"), (dict(iou=INF), ERR_ARG, "iou_threshold"), (dict(iou=-0.1), ERR_ARG, "iou_threshold"),
    (dict(obj=NAN, score=NAN), ERR_ARG, "obj_threshold"), (dict(obj=-INF), ERR_ARG, "obj_threshold"), (dict(score=INF), ERR_ARG, "score_threshold"),
    (dict(score=NAN), ERR_ARG, "score_threshold"), (dict(score=0.2), ERR_ARG, "below obj_threshold"),
    (dict(sigma=0.0), ERR_ARG, "sigma"), (dict(sigma=-1.0), ERR_ARG, "sigma"), (dict(sigma=NAN), ERR_ARG, "sigma"),
    (dict(sigma=INF), ERR_ARG, "sigma"), (dict(sigma=1e-60), ERR_ARG, "sigma"),
    (dict(ws=None), ERR_ARG, "workspace"), (dict(ws=WS + 4), ERR_ARG, "aligned"), (dict(ws_bytes=1024), ERR_ARG, "workspace"),
    (dict(rescore=BOXES + 24), ERR_ARG, "overlaps"), (dict(rescore=BOXES - 24), ERR_ARG, "overlaps"),
    (dict(rescore=BOXES + 4), ERR_ARG, "overlaps"),
    (dict(n=163457), ERR_UNSUPPORTED, "too large"), (dict(b=2048), ERR_UNSUPPORTED, "too large"),
])
def test_argument_errors_need_no_device(lib, change, code, word):
    a = dict(GOOD, **change)
    rc = lib.yolo_soft_nms(a["boxes"], a["b"], a["n"], a["iou"], a["obj"], a["score"], a["center"], a["method"], a["sigma"], a["agnostic"],
                           a["max_det"], a["keep"], a["count"], a["scores"], a["rescore"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), a["stream"])
    msg = lib.yolo_last_error().decode()
    assert rc == code, msg
    assert msg.startswith("soft_nms:") and word in msg, msg


def test_sigma_is_only_judged_for_the_gaussian_method(lib):
    """sigma = 0 with the linear method is no error; what stops this call is the short workspace that comes later in the checks."""
    a = dict(GOOD, method=1, sigma=0.0, ws_bytes=8)
    rc = lib.yolo_soft_nms(a["boxes"], a["b"], a["n"], a["iou"], a["obj"], a["score"], a["center"], a["method"], a["sigma"], a["agnostic"],
                           a["max_det"], a["keep"], a["count"], a["scores"], a["rescore"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), a["stream"])
    assert rc == ERR_ARG and "workspace 8 <" in lib.yolo_last_error().decode()


# ---- the Python surface
def test_names_are_attributes_outside_all():
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import boxes, utils
    assert yt.soft_nms is boxes.soft_nms and yt.NMSOptions is boxes.NMSOptions
    for name in ("soft_nms", "NMSOptions"):
        assert name not in yt.__all__ and name not in utils.__all__
    assert yt.NMSOptions() == ("gaussian", 0.5, None, False, None)
    assert yt.NMSOptions._fields == ("method", "sigma", "score_threshold", "class_agnostic", "max_det")


@pytest.mark.parametrize("options,message", [
    (dict(method="soft"), "method must be 'hard', 'linear' or 'gaussian', got 'soft'"),
    (dict(method=2), "method must be 'hard', 'linear' or 'gaussian', got 2"),
    (dict(sigma=0), "sigma must be a finite number > 0, got 0"),
    (dict(sigma=float("nan")), "sigma must be a finite number > 0, got nan"),
    (dict(sigma="wide"), "sigma must be a finite number > 0, got 'wide'"),
    (dict(sigma=True), "sigma must be a finite number > 0, got True"),
    (dict(score_threshold=0.1), "score_threshold must be None or a finite number >= obj_threshold (0.25), got 0.1"),
    (dict(score_threshold=float("inf")), "score_threshold must be None or a finite number >= obj_threshold (0.25), got inf"),
    (dict(class_agnostic="yes"), "class_agnostic must be a bool, got 'yes'"),
    (dict(class_agnostic=2), "class_agnostic must be a bool, got 2"),
    (dict(max_det=0), "max_det must be None or an integer >= 1, got 0"),
    (dict(max_det=2.5), "max_det must be None or an integer >= 1, got 2.5"),
    (dict(max_det=True), "max_det must be None or an integer >= 1, got True"),
    (dict(top_k=5), "unknown NMS option 'top_k'"),
])
def test_option_validation_messages(options, message):
    from yolo_for_turbines_amd import boxes
    with pytest.raises(ValueError, match=re.escape(message)):
        boxes._nms_options(options, 0.25)
    if "top_k" not in options:
        with pytest.raises(ValueError, match=re.escape(message)):
            boxes._nms_options(boxes.NMSOptions(**options), 0.25)


def test_options_resolve_and_python_argument_errors():
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import boxes
    assert boxes._nms_options(yt.NMSOptions(), 0.25) == (2, 0.5, 0.25, 0, 0)
    assert boxes._nms_options(dict(method="hard", score_threshold=0.5, class_agnostic=True, max_det=300), 0.25) == (0, 0.5, 0.5, 1, 300)
    assert boxes._nms_options({"method": "linear", "sigma": 2}, 0.0) == (1, 2.0, 0.0, 0, 0)
    with pytest.raises(ValueError, match="nms must be None, an NMSOptions or a dict"):
        boxes._nms_options("gaussian", 0.25)
    cpu = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.soft_nms(cpu, 0.45, 0.25)
    with pytest.raises(ValueError, match="unknown NMS option 'topk'"):
        yt.soft_nms(_FakeCuda(), 0.45, 0.25, topk=3)
    for fn in (yt.detect, yt.detect_images, yt.detect_tiled, yt.track_images):
        assert "nms" in fn.__code__.co_varnames[:fn.__code__.co_argcount + fn.__code__.co_kwonlyargcount], fn.__name__
    with pytest.raises(ValueError, match="method must be"):       # a bad option is refused before the forward runs
        yt.track_images(None, None, None, yt.Tracker(1), nms={"method": "matrix"})
    with pytest.raises(ValueError, match="method must be"):
        yt.detect([torch.zeros(1, 3, 2, 2, 7)] * 3, torch.rand(3, 3, 2), nms={"method": "matrix"})


class _FakeCuda:
    """Just enough of a tensor for soft_nms to reach its option check without a device."""
    is_cuda = True
