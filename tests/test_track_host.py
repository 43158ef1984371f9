"""Multi-object tracking on the host: the numpy reference (tests/track_ref.py) against itself (three statements of the matching, the
decoupled fp32 filter against the fp64 matrix filter), its behaviour on scenes with known answers, and the C interface as far as
it works without a GPU. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the matching
def test_three_statements_of_the_matching_agree_on_tie_heavy_matrices():
    """300 random matrices whose IoUs come from five values (so most comparisons are ties) with a random eligibility mask: the
    reference's lexsort walk, a brute-force sort of tuples and the kernel's mutual-best rounds give the same pairs; the rounds
    never exceed min(slots, detections)."""
    rng = np.random.default_rng(7)
    values = np.array([0.25, 0.5, 0.5, 0.75, 1.0], F32)
    most_rounds = 0
    for _ in range(300):
        S, D = rng.integers(1, 13, 2)
        iou = values[rng.integers(0, len(values), (S, D))]
        elig = rng.uniform(size=(S, D)) < rng.choice([0.2, 0.6, 1.0])
        a = R.greedy_match(iou, elig)
        assert a == R.brute_force_match(iou, elig)
        b, rounds = R.mutual_best_match(iou, elig)
        assert sorted(a) == sorted(b)
        assert rounds <= min(S, D)
        most_rounds = max(most_rounds, rounds)
        assert len({s for s, _ in a}) == len(a) == len({d for _, d in a})
    assert most_rounds >= 3                                   # the cases do need several rounds


def test_matching_order_is_iou_then_slot_then_detection():
    iou = np.array([[0.5, 0.5], [0.5, 0.9]], F32)
    assert R.greedy_match(iou, iou > 0) == [(1, 1), (0, 0)]
    iou = np.full((2, 2), 0.5, F32)
    assert R.greedy_match(iou, iou > 0) == [(0, 0), (1, 1)]
    assert R.greedy_match(iou, iou > F32(0.5)) == []          # the threshold is strict


# ---- the filter
def test_decoupled_fp32_filter_against_the_fp64_matrix_filter():
    """Six linearly moving objects (position noise 0.002, size noise 2 %) over 60 frames, seeds 0 .. 7: the four 2-state fp32
    filters against the 8-state fp64 filter with F, H, Q, R as matrices. Largest deviation measured over these seeds: 4.7e-8 on
    the mean (coordinates in the unit square) and 4.8e-7 of the slot's largest covariance entry on the covariance; the bars are
    four times that (profiles/track/README.md)."""
    worst_mean = worst_cov = 0.0
    for seed in range(8):
        zs = np.stack(R.linear_scene(np.random.default_rng(seed), frames=60))[:, :, :4]
        refs = [R.kalman8_fp64(zs[:, o].astype(np.float64)) for o in range(zs.shape[1])]
        mean, cov = R.kf_found(zs[0])
        for t in range(1, 60):
            mean, cov = R.kf_update(*R.kf_predict(mean, cov), zs[t])
            assert mean.dtype == F32 and cov.dtype == F32
            for o, (m64, c64) in enumerate(refs):
                blocks = np.array([[c64[t][c, c], c64[t][c, 4 + c], c64[t][4 + c, 4 + c]] for c in range(4)]).reshape(-1)
                off_block = c64[t].copy()
                for c in range(4):
                    off_block[np.ix_([c, 4 + c], [c, 4 + c])] = 0
                assert not off_block.any()                    # the 8-state filter really is four independent 2-state filters
                worst_mean = max(worst_mean, np.abs(mean[o] - m64[t]).max())
                worst_cov = max(worst_cov, np.abs(cov[o] - blocks).max() / np.abs(blocks).max())
    print("fp32 against fp64: mean %.2e, covariance %.2e (relative)" % (worst_mean, worst_cov))
    assert worst_mean <= 1.9e-7 and worst_cov <= 1.9e-6


def test_found_and_lost_rules():
    mean, cov = R.kf_found(np.array([0.5, 0.4, 0.2, 0.1], F32))
    assert mean.tolist() == [F32(0.5), F32(0.4), F32(0.2), F32(0.1), 0, 0, 0, 0]
    t, u = (F32(2) * R.WP) * F32(0.2), (F32(10) * R.WV) * F32(0.1)
    assert cov[0] == t * t and cov[1] == 0 and cov[5] == u * u and cov[3] == ((F32(2) * R.WP) * F32(0.1)) ** 2
    mean[4:] = [0.01, 0.02, 0.03, 0.04]
    moved, _ = R.kf_predict(mean, cov, lost=np.array(True))
    assert moved[6] == 0 and moved[7] == 0 and moved[2] == mean[2] and moved[0] == mean[0] + F32(0.01)


# ---- behaviour on scenes
def run_scene(frames, **kw):
    """frames: list of (k, 6) arrays. Returns the tracker and per frame (out_ids[:count], det_ids)."""
    tr = R.TrackerRef(1, **kw)
    log = []
    for rows in frames:
        _, ids, count, det = tr.update(np.asarray(rows, F32)[None])
        log.append((ids[0, :count[0]].tolist(), det[0].tolist()))
    return tr, log


@pytest.fixture(scope="module")
def scene():
    return R.linear_scene(np.random.default_rng(3), objects=6, frames=120, classes=2)


def test_ids_are_constant_over_120_frames(scene):
    tr, log = run_scene(scene)
    for ids, det in log:
        assert ids == [1, 2, 3, 4, 5, 6] and det == [1, 2, 3, 4, 5, 6]
    assert tr.next_id[0] == 7 and tr.overflow[0] == 0 and tr.frame[0] == 120


def test_missing_for_20_frames_returns_under_its_id_and_for_40_under_a_new_one(scene):
    gone20 = [f[1:] if 40 <= t < 60 else f for t, f in enumerate(scene)]
    tr, log = run_scene(gone20)
    assert log[45][0] == [2, 3, 4, 5, 6] and tr.next_id[0] == 7
    assert log[60][1] == [1, 2, 3, 4, 5, 6] and log[60][0] == [1, 2, 3, 4, 5, 6]
    gone40 = [f[1:] if 40 <= t < 80 else f for t, f in enumerate(scene)]
    tr, log = run_scene(gone40)
    assert log[80][1] == [-7, 2, 3, 4, 5, 6] and log[80][0] == [2, 3, 4, 5, 6]       # tentative in its first frame
    assert log[81][1] == [7, 2, 3, 4, 5, 6] and log[81][0] == [2, 3, 4, 5, 6, 7]
    assert tr.next_id[0] == 8


def test_a_low_score_keeps_an_id_but_founds_nothing(scene):
    frames = []
    for t, f in enumerate(scene):
        f = f.copy()
        if 40 <= t < 60:
            f[2, 4] = 0.3
        frames.append(f)
    tr, log = run_scene(frames)
    for ids, det in log:
        assert ids == [1, 2, 3, 4, 5, 6] and det == [1, 2, 3, 4, 5, 6]
    # a seventh object that is only ever reported at 0.3
    extra = np.array([0.9, 0.9, 0.05, 0.05, 0.3, 0.0], F32)
    tr, log = run_scene([np.vstack([f, extra]) for f in scene[:40]])
    for ids, det in log:
        assert ids == [1, 2, 3, 4, 5, 6] and det == [1, 2, 3, 4, 5, 6, 0]
    assert tr.next_id[0] == 7


def test_a_detection_seen_once_is_never_listed(scene):
    ghost = np.array([0.9, 0.1, 0.05, 0.05, 0.9, 1.0], F32)
    frames = [np.vstack([f, ghost]) if t == 10 else f for t, f in enumerate(scene[:30])]
    tr, log = run_scene(frames)
    assert log[10][1] == [1, 2, 3, 4, 5, 6, -7]
    assert all(7 not in ids for ids, _ in log)
    assert (tr.state[0] == R.TRACKED).sum() == 6 and (tr.state[0] == R.FREE).sum() == tr.M - 6
    assert tr.next_id[0] == 8                                 # the id is spent


def test_overflow_counts_the_dropped_detections(scene):
    tr, log = run_scene(scene[:10], max_tracks=4)
    assert log[0][1] == [1, 2, 3, 4, 0, 0] and log[9][0] == [1, 2, 3, 4]
    assert tr.overflow[0] == 2 * 10 and tr.next_id[0] == 5


# ---- the C interface
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    return _lib


def test_header_declares_the_exports_and_the_size_functions_follow_it(lib):
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    for name in ("yolo_track_state_bytes", "yolo_track_workspace_bytes", "yolo_track_reset", "yolo_track_update"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in lib.EXPORTS
    assert "multi-object tracking (csrc/track.hip; nothing of the reference)" in hdr
    l = lib.lib()
    assert l.yolo_version() >= 103
    for b, m in ((1, 1), (3, 128), (2047, 512)):
        assert l.yolo_track_state_bytes(b, m) == b * (R.HDR_WORDS + R.SLOT_WORDS * m) * 4
    for b, m in ((0, 8), (2048, 8), (1, 0), (1, 513), (-1, -1)):
        assert l.yolo_track_state_bytes(b, m) == 0 and l.yolo_track_workspace_bytes(b, 10, m) == 0
    for b, n, m in ((1, 1, 1), (33, 1025, 512), (2047, 163456, 512)):
        assert l.yolo_track_workspace_bytes(b, n, m) == 8 * b * n
    assert l.yolo_track_workspace_bytes(4, 0, 8) == 0 and l.yolo_track_workspace_bytes(1, 163457, 8) == 0
    assert l.yolo_track_workspace_bytes(1, -1, 8) == 0


def test_params_struct_layout_matches_the_header(lib):
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} yolo_track_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in names.split(",")]
    want = [(n, {C.c_double: "double", C.c_double * 3: "double", C.c_int32: "int32_t"}[t]) for n, t in lib.TrackParams._fields_]
    assert [(n if t != C.c_double * 3 else n + "[3]") for n, t in lib.TrackParams._fields_] == [n for _, n in fields]
    assert [t for _, t in want] == [t for t, _ in fields]
    assert C.sizeof(lib.TrackParams) == 64 and lib.TrackParams.match_iou.offset == 24 and lib.TrackParams.max_age.offset == 48
    assert lib.TrackParams.class_agnostic.offset == 56


def test_c_argument_errors_without_a_gpu(lib):
    """Everything yolo_track_update and yolo_track_reset refuse, they refuse before the launch: no GPU is touched."""
    l = lib.lib()
    p = lib.TrackParams(0.5, 0.1, 0.6, (C.c_double * 3)(0.2, 0.5, 0.3), 30, 1, 0, 0)
    buf = (C.c_int32 * 4096)()
    a = C.addressof(buf)

    def update(b=1, m=4, n=8, boxes=a, keep=None, count=None, params=p, out=a, ws=a, ws_bytes=1 << 20, state=a):
        return l.yolo_track_update(state, b, m, boxes, n, keep, count, C.byref(params) if params is not None else None, out, out, out, out,
                                   ws, ws_bytes, None)

    for kw in (dict(b=0), dict(b=2048), dict(m=0), dict(m=513), dict(n=-1), dict(n=163457)):
        assert update(**kw) == -2, kw                         # YOLO_ERR_UNSUPPORTED
        assert b"outside the limits" in l.yolo_last_error()
    for kw in (dict(state=None), dict(boxes=None), dict(params=None), dict(out=None), dict(keep=a), dict(state=a + 2)):
        assert update(**kw) == -1, kw                         # YOLO_ERR_ARG
    for field, value in (("high_threshold", float("nan")), ("max_age", -1)):
        bad = lib.TrackParams.from_buffer_copy(p)
        setattr(bad, field, value)
        assert update(params=bad) == -1, field
    for i, v in ((0, -0.1), (1, 1.5), (2, float("nan"))):
        bad = lib.TrackParams.from_buffer_copy(p)
        bad.match_iou[i] = v
        assert update(params=bad) == -1 and b"match_iou" in l.yolo_last_error()
    for kw in (dict(ws=None), dict(ws_bytes=8 * 8 - 1), dict(ws=a + 1)):
        assert update(**kw) == -4, kw                         # YOLO_ERR_WORKSPACE
    assert l.yolo_track_reset(None, 1, 4, None, None) == -1
    assert l.yolo_track_reset(a, 0, 4, None, None) == -2 and l.yolo_track_reset(a, 1, 513, None, None) == -2


def test_python_argument_errors():
    import yolo_for_turbines_amd as yt
    for kw in (dict(streams=0), dict(streams=2048), dict(streams=1.5), dict(streams=True), dict(max_tracks=0), dict(max_tracks=513),
               dict(high_threshold=0.05), dict(new_threshold=0.4), dict(low_threshold=-0.1), dict(high_threshold=float("nan")),
               dict(new_threshold=float("inf")), dict(match_iou=(0.2, 0.5)), dict(match_iou=(0.2, 0.5, 1.5)), dict(match_iou=0.3),
               dict(match_iou=(0.2, float("nan"), 0.3)), dict(max_age=-1), dict(max_age=1.5), dict(box_format="xyxy")):
        with pytest.raises(ValueError):
            yt.Tracker(**{"streams": 2, **kw})
    t = yt.Tracker(2, max_tracks=8)
    assert (t.high_threshold, t.low_threshold, t.new_threshold, t.match_iou, t.max_age) == (0.5, 0.1, 0.6, (0.2, 0.5, 0.3), 30)
    for bad in (torch.zeros(2, 4, 5), torch.zeros(4, 6), torch.zeros(3, 4, 6), torch.zeros(2, 4, 6, dtype=torch.int32), [[0.0] * 6]):
        with pytest.raises(ValueError):
            t.update(bad)
    with pytest.raises(ValueError):
        t.update(torch.zeros(2, 4, 6), keep=torch.zeros(2, 4, dtype=torch.int32))                    # keep without count
    with pytest.raises(ValueError):
        t.update(torch.zeros(2, 4, 6), count=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        t.update(torch.zeros(2, 4, 6), keep=torch.zeros(2, 4), count=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="MI355X only"):
        t.update(torch.zeros(2, 4, 6))
    with pytest.raises(ValueError):
        t.reset([2])
    m = yt.YOLOv3(num_classes=2).eval()
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.track_images(m, torch.zeros(2, 3, 64, 64), torch.rand(3, 3, 2), t)
    with pytest.raises(ValueError):
        yt.track_images(m, torch.zeros(2, 3, 64, 64), torch.rand(3, 3, 2), yt.Tracker(2, box_format="corners"))
    with pytest.raises(ValueError):
        yt.track_images(m, torch.zeros(2, 3, 64, 64), torch.rand(3, 3, 2), None)
