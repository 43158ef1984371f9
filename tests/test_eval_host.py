"""Evaluation at several IoU thresholds, on the host (nothing is launched): the sequential restatement the GPU tests compare with
(tests/eval_ref.py) against ``oracle.metrics.calc_map`` and the reference's own values in tests/golden/kat.npz, the hand-over case,
and the return codes / workspace sizes of yolo_eval_detections for arguments that are refused before any launch."""
import ctypes as C
import functools
import math

import pytest

from oracle import metrics as om
from tests import eval_ref as er
from tests import golden_inputs as gi

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_WORKSPACE = 0, -1, -2, -3, -4
FAKE = 1 << 20          # a non-null, aligned "device pointer" for calls that must return before they launch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _ref(case):
    pb, tb = gi.map_boxes(case)
    return er.evaluate(pb, tb, gi.MAP_CASES[case]["nc"])


@pytest.mark.parametrize("case", list(gi.MAP_CASES))
def test_restatement_equals_the_oracle_at_ten_thresholds(case):
    pb, tb = gi.map_boxes(case)
    nc = gi.MAP_CASES[case]["nc"]
    ref = _ref(case)
    for t, thr in enumerate(er.DEFAULT_THRESHOLDS):
        want = float(om.calc_map(pb, tb, thr, "center", nc))
        assert float(ref["map"][t]) == want, f"{case} @{thr}: {float(ref['map'][t])} vs {want}"
    to_thr, lead = er.check_precondition(ref)
    print(f"{case}: margins {to_thr:.1e} (threshold) {lead:.1e} (second best)")
    # the flags of a threshold are consistent with its counts
    assert ref["flags"].shape == (10, len(ref["order"]))
    assert (ref["tp_at_conf"] <= ref["n_det_at_conf"][None, :]).all() and (ref["tp_at_conf"] <= ref["n_gt"][None, :]).all()


@pytest.mark.parametrize("case", list(gi.MAP_CASES))
def test_restatement_vs_reference_values(golden, case):
    g = golden("kat")
    ref = _ref(case)
    for t, key in ((0, f"map_{case}"), (5, f"map_{case}_iou75")):
        assert abs(float(ref["map"][t]) - float(g[key])) <= 2e-6, f"{case} {key}: {float(ref['map'][t])} vs {float(g[key])}"


def test_the_cases_exercise_the_threshold_dependent_part():
    """Some ground truth changes owner between thresholds in at least one case: a design in which the first claimer keeps it at
    every threshold would differ from the walk there."""
    changed = 0
    for case in gi.MAP_CASES:
        ref = _ref(case)
        owner = []
        for t in range(10):
            o = {}
            for k in range(len(ref["order"])):
                if ref["flags"][t, k]:
                    o[int(ref["best_gt"][k])] = k
            owner.append(o)
        changed += sum(1 for g_ in owner[0] if any(g_ in o and o[g_] != owner[0][g_] for o in owner[1:]))
    assert changed > 0


def test_hand_over_case():
    h = er.HANDOVER
    thr = sorted(h["flags"])
    ref = er.evaluate(h["preds"], h["trues"], 1, thr)
    for t, v in enumerate(thr):
        assert ref["flags"][t].astype(int).tolist() == h["flags"][v], v
        assert abs(float(ref["map"][t]) - float(om.calc_map(h["preds"], h["trues"], v, "center", 1))) == 0
    for v, a in h["ap"].items():
        assert abs(float(ref["ap"][thr.index(v), 0]) - a) <= 1e-6
    assert abs(float(ref["best_iou"][0]) - 0.66666) < 1e-5 and abs(float(ref["best_iou"][1]) - 0.92499) < 1e-5
    assert abs(float(ref["map"].astype("float64").mean()) - 0.525) <= 1e-6
    assert h["map_50_95"] == 0.525


def test_restatement_corner_cases():
    p = [[0, .5, .5, .2, .2, .9, 0], [0, .5, .5, .2, .2, .5, 1], [0, .5, .5, .2, .2, .5, 3], [0, .5, .5, .2, .2, .5, -1], [0, .5, .5, .2, .2, .5, .5]]
    t = [[0, .5, .5, .2, .2, 1., 0], [0, .1, .1, .1, .1, 1., 2]]
    ref = er.evaluate(p, t, 3, [0.5], conf_threshold=0.5)
    assert ref["order"].tolist() == [0, 1]                                   # classes 3, -1 and 0.5 are dropped
    assert ref["n_det"].tolist() == [1, 1, 0] and ref["n_gt"].tolist() == [1, 0, 1]
    assert ref["n_det_at_conf"].tolist() == [1, 0, 0]                        # 0.5 > 0.5 is false
    assert ref["ap"][0, 0] == 1.0 and math.isnan(ref["ap"][0, 1]) and ref["ap"][0, 2] == 0.0
    assert float(ref["map"][0]) == 0.5
    with pytest.raises(ZeroDivisionError):
        er.evaluate(p, [], 3, [0.5])


# ---------------------------------------------------------------------------------------------------- the C entry points
def _eval(L, n_det=100, n_gt=40, nc=3, thr=(0.5, 0.75), n_thr=None, conf=0.5, center=1, dets=FAKE, d_off=FAKE, gts=FAKE, g_off=FAKE,
          best_iou=FAKE, best_gt=FAKE, tp=FAKE, ap=FAKE, tpc=FAKE, ndc=FAKE, ws=FAKE, ws_bytes=None, no_thr=False):
    lib = L.lib()
    n_thr = len(thr) if n_thr is None else n_thr
    arr = None if no_thr else (C.c_float * max(len(thr), 1))(*thr)           # the thresholds are read on the host
    if ws_bytes is None:
        ws_bytes = lib.yolo_eval_workspace_bytes(n_det, n_gt, n_thr)
    return lib.yolo_eval_detections(dets or None, d_off or None, n_det, gts or None, g_off or None, n_gt, nc, arr, n_thr, conf, center,
                                    best_iou or None, best_gt or None, tp or None, ap or None, tpc or None, ndc or None, ws or None, ws_bytes,
                                    None)


def test_eval_argument_errors(built):
    L = built
    sixteen = tuple(0.05 * i for i in range(16))
    for kw in (dict(n_det=-1), dict(n_gt=-1), dict(nc=0), dict(nc=-2), dict(thr=()), dict(thr=sixteen + (0.9,)), dict(n_thr=0), dict(n_thr=17),
               dict(thr=(1.0,)), dict(thr=(0.5, -0.01)), dict(thr=(0.5, math.nan)), dict(thr=(math.inf,)), dict(conf=math.nan),
               dict(center=2), dict(center=-1), dict(no_thr=True), dict(dets=0), dict(d_off=0), dict(gts=0), dict(g_off=0), dict(best_iou=0),
               dict(best_gt=0), dict(tp=0), dict(ap=0), dict(tpc=0), dict(ndc=0)):
        assert _eval(L, ws_bytes=1 << 30, **kw) == ERR_ARG, kw
        assert L.lib().yolo_last_error().startswith(b"eval_detections")
    # an argument error comes before the workspace is looked at
    assert _eval(L, nc=0, ws=0, ws_bytes=0) == ERR_ARG
    assert _eval(L, thr=(1.5,), ws=0, ws_bytes=0) == ERR_ARG


def test_eval_workspace_errors(built):
    L = built
    lib = L.lib()
    for n_det, n_gt, thr in ((100, 40, (0.5, 0.75)), (0, 40, (0.5,)), (100, 0, (0.5,)), (0, 0, (0.5,)), (262144, 262144, tuple(0.05 * i for i in range(16)))):
        need = lib.yolo_eval_workspace_bytes(n_det, n_gt, len(thr))
        assert need >= max(16, 4 * n_gt * len(thr))
        assert _eval(L, n_det=n_det, n_gt=n_gt, thr=thr, ws=0, ws_bytes=0) == ERR_WORKSPACE
        assert _eval(L, n_det=n_det, n_gt=n_gt, thr=thr, ws=0, ws_bytes=need) == ERR_WORKSPACE
        assert _eval(L, n_det=n_det, n_gt=n_gt, thr=thr, ws_bytes=need - 1) == ERR_WORKSPACE
        assert b"workspace" in lib.yolo_last_error()
    assert _eval(L, ws=FAKE + 2) == ERR_WORKSPACE                             # not 4-byte aligned


def test_eval_workspace_query(built):
    """Nonzero inside the limits, never smaller for more ground truths or thresholds, 64-bit, 0 outside the limits."""
    lib = built.lib()
    ns = (0, 1, 2, 255, 256, 257, 5000, 262144, 2 ** 31 - 1)
    for n_thr in (1, 10, 16):
        sizes = [lib.yolo_eval_workspace_bytes(1000, n, n_thr) for n in ns]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    by_thr = [lib.yolo_eval_workspace_bytes(1000, 5000, k) for k in range(1, 17)]
    assert by_thr == sorted(by_thr) and by_thr[-1] > by_thr[0]
    assert lib.yolo_eval_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 16) > 2 ** 32
    for n_det, n_gt, n_thr in ((-1, 10, 1), (10, -1, 1), (10, 10, 0), (10, 10, 17), (10, 10, -1)):
        assert lib.yolo_eval_workspace_bytes(n_det, n_gt, n_thr) == 0


def test_wrapper_refuses_bad_thresholds(built):
    import yolo_for_turbines_amd as yt
    assert "evaluate_detections" in yt.__all__ and "evaluate_model" in yt.__all__
    rows = [[0, .5, .5, .2, .2, .9, 0]]
    for bad in ([], [1.0], [-0.1], [0.5] * 17, [math.nan]):
        with pytest.raises(ValueError, match="iou_thresholds"):
            yt.evaluate_detections(rows, rows, 1, iou_thresholds=bad)
    with pytest.raises(ValueError, match="conf_threshold"):
        yt.evaluate_detections(rows, rows, 1, conf_threshold=math.nan)
