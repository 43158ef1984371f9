"""Weighted box fusion and the test-time-augmentation helpers on the host: the numpy reference (tests/fuse_ref.py) on hand-worked
cases with literal results, its fp32 walk against its fp64 walk on clustered data, tta_views, the view reference against torch's
bilinear interpolation, and the C header. No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fuse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_cases(case, dtype):
    _, rows, kw, want_rows, want_members, want_assign = case
    fused, members, count, assign = R.fuse_ref(np.array(rows, np.float32), box_format="corners", dtype=dtype, **kw)
    assert count == len(want_rows)
    assert np.array_equal(fused[:count], np.array(want_rows, dtype))          # exact: every number is representable
    assert members[:count].tolist() == want_members and assign.tolist() == want_assign
    assert not fused[count:].any() and not members[count:].any()
    # the same boxes in centre format fuse to the same boxes in centre format
    fc, mc, cc, ac = R.fuse_ref(R.to_center(rows), box_format="center", dtype=dtype, **kw)
    assert cc == count and np.array_equal(fc[:cc], R.to_center(want_rows).astype(dtype)) and np.array_equal(mc, members)
    assert np.array_equal(ac, assign)


def test_threshold_edge_is_strict():
    """With the threshold at the reference's own fp32 IoU of a pair the pair stays apart; one ulp below, it merges."""
    a, b = R.HAND_CASES[0][1]
    one = np.float32(1)
    inter = np.float32(0.625) * one
    iou = inter / (((one + np.float32(0.625)) - inter) + np.float32(1e-6))     # the contract's expression for the unit square and _B
    assert iou.dtype == np.float32 and 0.62 < iou < 0.625
    rows = np.array([a, b], np.float32)
    assert R.fuse_ref(rows, iou_threshold=float(iou), box_format="corners")[2] == 2
    assert R.fuse_ref(rows, iou_threshold=float(np.nextafter(iou, np.float32(0))), box_format="corners")[2] == 1


def test_fp32_walk_matches_fp64_on_clustered_boxes():
    """40 objects x 12 jittered reports (centre sigma 0.012, relative size sigma 0.036, scores U(0.05, 1), 2 classes), threshold
    0.55, objectness 0.3; three draws of default_rng(5). No IoU the fp64 walk compares lies within 1e-5 of the threshold (smallest
    margin measured: 2.3e-5, 2.2e-4, 1.1e-3), so the fp32 walk must take the same decisions; corners and scores then differ by
    rounding only. Bound 2e-6: at most 16 sequential fp32 additions and one division on values <= 1 (measured: 1.8e-7)."""
    rng = np.random.default_rng(5)
    for _ in range(3):
        boxes = R.clustered(rng)
        margins = []
        f64, m64, c64, a64 = R.fuse_ref(boxes, 0.55, 0.3, dtype=np.float64, margins=margins)
        assert min(margins) > 1e-5
        f32, m32, c32, a32 = R.fuse_ref(boxes, 0.55, 0.3)
        assert c32 == c64 and 40 <= c64 < 480 and np.array_equal(m32, m64) and np.array_equal(a32, a64)
        assert m64.max() <= 16
        err = np.abs(f32[:c64, :5].astype(np.float64) - f64[:c64, :5]).max()
        print("fp32 against fp64: max abs difference %.2e" % err)
        assert err <= 2e-6
        assert np.array_equal(f32[:, 5], f64[:, 5])


def test_ref_order_and_zero_rows():
    boxes = R.clustered(np.random.default_rng(1), 100)
    boxes[::7, 4] = 0.0                                                        # filtered by obj_threshold = 0 (strict)
    fused, members, count, assign = R.fuse_ref(boxes, 0.55, 0.0, n_views=4)
    assert 0 < count < 100 and (np.diff(fused[:count, 4]) <= 0).all()
    assert members[:count].sum() == (assign >= 0).sum() == 100 - len(boxes[::7])
    assert (assign[::7] == -1).all() and np.array_equal(np.bincount(assign[assign >= 0], minlength=count), members[:count])


# ---- tta_views
def test_tta_views_rounding_and_order():
    import yolo_for_turbines_amd as yt
    assert yt.tta_views(416, 416) == [(416, 416, 0, 0), (416, 416, 1, 0)]
    # 416 * 0.75 / 32 = 9.75 -> 10 -> 320; 416 * 0.5 / 32 = 6.5 -> 6 (half to even) -> 192; 416 * 1.25 / 32 = 16.25 -> 16 -> 512
    assert yt.tta_views(416, 416, ("none",), (0.75, 0.5, 1.25)) == [(320, 320, 0, 0), (192, 192, 0, 0), (512, 512, 0, 0)]
    # 7.5 -> 8 (half to even, upwards) and 2.5 -> 2; 0.4 -> 0 -> the minimum of one cell
    assert yt.tta_views(480, 160, ("none",), (0.5,)) == [(256, 64, 0, 0)]
    assert yt.tta_views(32, 64, ("none",), (0.4,)) == [(32, 32, 0, 0)]
    # scale-major, then flip, both in the order given; rectangular inputs per axis
    assert yt.tta_views(96, 128, ("lrud", "none", "ud", "lr"), (0.75, 1.0)) == [
        (64, 96, 1, 1), (64, 96, 0, 0), (64, 96, 0, 1), (64, 96, 1, 0), (96, 128, 1, 1), (96, 128, 0, 0), (96, 128, 0, 1), (96, 128, 1, 0)]
    assert yt.tta_views(96, 128, ("none",), (1.0, 0.75), max_sizes=2) == [(96, 128, 0, 0), (64, 96, 0, 0)]


@pytest.mark.parametrize("kw", [
    dict(flips=()), dict(flips=("none", "diag")), dict(flips="lr"), dict(flips=("none", "none")), dict(flips=(0,)),
    dict(scales=()), dict(scales=(0.0,)), dict(scales=(-1.0,)), dict(scales=(4.5,)), dict(scales=(float("nan"),)),
    dict(scales=(float("inf"),)), dict(scales=("1.0",)), dict(scales=(True,)), dict(scales=1.0),
    dict(scales=(1.0, 1.01)),                        # both round to 416: the same view twice
    dict(scales=(1.0, 0.75, 0.5), max_sizes=2),      # three sizes, two plans
])
def test_tta_views_rejects(kw):
    import yolo_for_turbines_amd as yt
    with pytest.raises(ValueError):
        yt.tta_views(416, 416, **kw)


def test_tta_views_rejects_bad_size():
    import yolo_for_turbines_amd as yt
    with pytest.raises(ValueError):
        yt.tta_views(0, 416)


# ---- the view reference
@pytest.mark.parametrize("shape,out", [((2, 3, 5, 7), (8, 3)), ((2, 3, 4, 4), (9, 13)), ((2, 3, 32, 64), (64, 32))])
def test_view_ref_against_torch_bilinear(shape, out):
    """torch forms the source coordinate in fp32 and blends in another association, so equality is not expected. Measured on
    these shapes with U(-1, 1) data: 6.0e-7, 3.0e-7, 1.2e-7; the bound is four times the largest, 2.4e-6."""
    x = np.random.default_rng(11).uniform(-1, 1, shape).astype(np.float32)
    ref = R.tta_view_ref(x, *out)
    t = torch.nn.functional.interpolate(torch.from_numpy(x), size=out, mode="bilinear", align_corners=False).numpy()
    err = np.abs(ref.astype(np.float64) - t).max()
    print("view reference against torch: %.2e" % err)
    assert ref.shape == shape[:2] + out and err <= 2.4e-6


def test_view_ref_mirror_is_exact_and_edges_clamp():
    x = np.random.default_rng(3).standard_normal((2, 3, 5, 7)).astype(np.float32)
    for lr in (False, True):
        for ud in (False, True):
            want = torch.flip(torch.from_numpy(x), [d for d, on in ((2, ud), (3, lr)) if on]).numpy() if (lr or ud) else x
            assert np.array_equal(R.tta_view_ref(x, 5, 7, lr, ud), want)
    up = R.tta_view_ref(x, 10, 14)                   # the first and last output pixels sit outside the source centres: copies
    assert np.array_equal(up[:, :, 0, 0], x[:, :, 0, 0]) and np.array_equal(up[:, :, -1, -1], x[:, :, -1, -1])
    b = np.random.default_rng(4).uniform(0, 1, (2, 9, 6)).astype(np.float32)
    u = R.unflip_ref(b, 2, 4, True, False)
    assert np.array_equal(u[:, 2:6, 0], np.float32(1) - b[:, 2:6, 0]) and np.array_equal(u[:, :, 1:], b[:, :, 1:])
    assert np.array_equal(u[:, :2], b[:, :2]) and np.array_equal(u[:, 6:], b[:, 6:])


# ---- interface
def test_header_declares_the_exports_and_host_queries_work():
    import __graft_entry__ as g
    g.build()
    from yolo_for_turbines_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolo_mi355x.h")).read()
    for name in ("yolo_fuse_workspace_bytes", "yolo_fuse_boxes", "yolo_fuse_onchip_clusters", "yolo_fuse_chunk_candidates",
                 "yolo_tta_view", "yolo_boxes_unflip"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    lib = _lib.lib()
    assert lib.yolo_fuse_onchip_clusters() >= 64 and lib.yolo_fuse_onchip_clusters() % 64 == 0
    assert lib.yolo_fuse_chunk_candidates() >= 1
    small, big = lib.yolo_fuse_workspace_bytes(1, 100), lib.yolo_fuse_workspace_bytes(16, 10000)
    assert 0 < small < big and big > 16 * 10000 * (8 + 8 + 52 + 32)
    assert lib.yolo_fuse_workspace_bytes(1, 163456) > 0 and lib.yolo_fuse_workspace_bytes(1, 163457) == 0
    assert lib.yolo_fuse_workspace_bytes(0, 10) == 0 and lib.yolo_fuse_workspace_bytes(1, 0) > 0


def test_python_argument_errors():
    import yolo_for_turbines_amd as yt
    cpu = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.fuse_boxes(cpu)
    for kw in (dict(obj_threshold=-0.1), dict(obj_threshold=float("nan")), dict(iou_threshold=1.5), dict(iou_threshold=float("nan")),
               dict(conf_type="mean"), dict(n_views=-1), dict(n_views=1.5), dict(box_format="xyxy")):
        with pytest.raises(ValueError):
            yt.fuse_boxes(cpu, **kw)
    with pytest.raises(ValueError):
        yt.fuse_boxes(torch.zeros(4, 5))
    with pytest.raises(ValueError):
        yt.fuse_boxes(torch.zeros(4, 6, dtype=torch.int32))
    m = yt.YOLOv3(num_classes=2).eval()
    anchors = torch.rand(3, 3, 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.tta_boxes(m, torch.zeros(1, 3, 64, 64), anchors)
    with pytest.raises(RuntimeError, match="MI355X only"):
        yt.detect_tta(m, torch.zeros(1, 3, 64, 64), anchors)
    with pytest.raises(ValueError):
        yt.tta_boxes(m, torch.zeros(3, 64, 64), anchors)
    with pytest.raises(ValueError, match="eval plans"):           # five sizes, four plans: refused before anything runs
        yt.tta_boxes(m, torch.zeros(1, 3, 416, 416), anchors, ("none",), (1.0, 0.75, 0.5, 1.25, 1.5))
    assert m._engine.max_eval_plans == 4
    assert "fuse_boxes(" in yt.detect_tiled.__doc__
