"""Times yolo_soft_nms against yolo_nms on the same input in the same process (the inputs of tools/nms_bench.py: 16 images of 10,000
boxes with 2 and 80 classes, uniform and clustered; plus the 22,743 rows of one 608 x 608 forward): each of the three methods with
and without max_det=300, windows alternating with yolo_nms round by round, every window as many calls as fill 50 ms (at least 5)
and ended by a device synchronise; the median of the rounds is reported with their spread. A plain torch-ops Soft-NMS loop (Gaussian) is timed on the first image of every input.
Prints one JSON line per measurement.   python tools/soft_nms_bench.py [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import yolo_for_turbines_amd as yt
from oracle import net as onet
from tests import golden_inputs as gi

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WINDOW_MS = 50.0               # a timed window holds as many calls as fill this (at least 5): yolo_nms takes 0.1 to 0.6 ms a call
IOU, SIGMA = 0.45, 0.5


def window(fn, calls=5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def calls_for(fn):
    return max(5, min(1000, int(WINDOW_MS / window(fn)) + 1))


def torch_soft_nms_gaussian(rows, obj_thr):
    """The straightforward loop in torch ops on one image (centre format), per-class: argmax, IoU against the rest, decay, filter."""
    rows = rows[rows[:, 4] > obj_thr]
    x1, y1 = rows[:, 0] - rows[:, 2] / 2, rows[:, 1] - rows[:, 3] / 2
    x2, y2, area, cls = x1 + rows[:, 2], y1 + rows[:, 3], rows[:, 2] * rows[:, 3], rows[:, 5]
    s = rows[:, 4].clone()
    live = torch.ones_like(s, dtype=torch.bool)
    kept = 0
    while True:
        cur = torch.where(live, s, torch.full_like(s, -1.0))
        top, g = cur.max(0)
        if not bool(top > obj_thr):                      # one host read per pick, as such loops have
            return kept
        kept += 1
        live[g] = False
        inter = (torch.minimum(x2[g], x2) - torch.maximum(x1[g], x1)).clamp(min=0) * (torch.minimum(y2[g], y2) - torch.maximum(y1[g], y1)).clamp(min=0)
        iou = inter / (area[g] + area - inter + 1e-6)
        s = torch.where(live & (cls == cls[g]), s * torch.exp(-(iou * iou) / SIGMA), s)
        live &= s > obj_thr


def inputs():
    for nc in (2, 80):
        for kind in ("uniform", "clustered"):
            gen = gi.boxes_uniform if kind == "uniform" else (lambda n, nc, s: gi.boxes_clustered(n, nc, s, jitter=0.15))
            yield f"{kind}_nc{nc}_16x10000", torch.from_numpy(np.stack([gen(10000, nc, 1000 + b) for b in range(16)])).cuda(), 0.5
    m = yt.YOLOv3(num_classes=2)
    m.load_state_dict(onet.synth_state_dict(11, 3, 2, gain=gi.NET_GAIN))
    m = m.cuda().eval()
    anchors = [a.cuda() for a in yt.scaled_anchors(gi.COCO_ANCHORS, 608, 608)]
    boxes = yt.detect_images(m, onet.synth_input(1, 1, 608).cuda(), anchors, IOU, 0.1)[0]
    assert boxes.shape[1] == 22743
    yield "forward608_nc2_1x22743", boxes, 0.1           # the tracker's low threshold: thousands of rows per class


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "window_ms": WINDOW_MS, "iou": IOU, "sigma": SIGMA}))
    for name, t, thr in inputs():
        variants = {"yolo_nms": lambda: yt.nms_indices(t, IOU, thr, "center")}
        for method in ("hard", "linear", "gaussian"):
            for max_det in (None, 300):
                variants[f"soft_{method}" + ("_maxdet300" if max_det else "")] = (
                    lambda method=method, max_det=max_det: yt.soft_nms(t, IOU, thr, "center", method=method, sigma=SIGMA, max_det=max_det))
        kept = {}
        for k, fn in variants.items():                    # warm-up: code objects, the workspace, the LDS attribute
            for _ in range(2):
                out = fn()
            kept[k] = float(out[1].float().mean())
        calls = {k: calls_for(fn) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):                           # alternating: every round times every variant once
            for k, fn in variants.items():
                times[k].append(window(fn, calls[k]))
        base = statistics.median(times["yolo_nms"])
        cand = float((t[..., 4] > thr).sum(1).float().mean())
        for k, v in times.items():
            med = statistics.median(v)
            print(json.dumps({"input": name, "obj_threshold": thr, "candidates_per_image": cand, "variant": k, "ms_per_call_median": round(med, 4),
                              "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "spread_pct": round(100 * (max(v) - min(v)) / med, 1),
                              "calls_per_window": calls[k], "kept_per_image": kept[k],
                              "ratio_to_yolo_nms": round(med / base, 3)}), flush=True)
        one = t[:1].contiguous()
        soft_one = lambda: yt.soft_nms(one, IOU, thr, "center", method="gaussian", sigma=SIGMA)
        soft_one()
        n_one = calls_for(soft_one)
        ms_kernel = statistics.median(window(soft_one, n_one) for _ in range(ROUNDS))
        torch.cuda.synchronize()                          # no warm-up run: thousands of picks, the first launches vanish in them
        t0 = time.perf_counter()
        n_kept = torch_soft_nms_gaussian(one[0], thr)
        torch.cuda.synchronize()
        ms_torch = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"input": name + " (first image)", "variant": "torch_ops_loop_gaussian", "ms_per_call": round(ms_torch, 2), "kept": n_kept,
                          "soft_gaussian_ms_per_call_median": round(ms_kernel, 4), "kernel_kept": int(soft_one()[1][0]),
                          "torch_over_kernel": round(ms_torch / ms_kernel, 1)}), flush=True)


if __name__ == "__main__":
    main()
