"""Kernel time of the training augmentation (augment_batch: yolo_augment_boxes + yolo_augment_images) for B images at
S x S, HIP events around 20 back-to-back launches of the kernels only (tables and images already on the device), after
warm-up, and around the whole augment_batch call; the pinned H2D staging
of the sources on its own line; the numpy restatement's CPU time per image for scale. One JSON line per case.

    python tools/augment_bench.py [--batch 32] [--size 416] [--iters 50] [--out profiles/augment/bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yolo_for_turbines_amd as yt  # noqa: E402
from tests import augment_ref as ar  # noqa: E402


REP = 20


def _events(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment", "bench.jsonl"))
    a = ap.parse_args()
    B, S = a.batch, a.size
    rng = np.random.default_rng(0)
    lines = []
    for (h, w) in ((480, 640), (1080, 1920)):
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]
        boxes = [[[float(v) for v in rng.uniform(0.2, 0.8, 2)] + [0.1, 0.15, 1.0] for _ in range(4)] for _ in range(B)]
        dev_imgs = [torch.from_numpy(i).cuda() for i in imgs]
        for mosaic in (False, True):
            mo = np.array([[(b + k) % B for k in range(4)] for b in range(B)]) if mosaic else None
            p = yt.augment_params(B, torch.Generator().manual_seed(1), mosaic=mosaic)
            p[:, 0] = p[:, 4] = p[:, 8] = 1.0                               # every transform on: the most work
            pd = p.cuda()
            name = f"{'mosaic' if mosaic else 'standard'} {w}x{h} -> {S}x{S}"
            # kernels only: tables and images on the device, REP launches back to back between two events
            _, _, _, launch = yt.data._augment_prepare(dev_imgs, boxes, S, pd, None, mo, None)
            med, best = _events(lambda: [launch() for _ in range(REP)], a.iters)
            med, best = med / REP, best / REP
            lines.append({"case": name + " (kernels)", "batch": B, "ms_median": round(med, 4), "ms_min": round(best, 4),
                          "images_per_s": round(B / med * 1e3, 1)})
            # the whole call: host tables, one pinned copy, allocation, launches (what a training loop pays per batch)
            med, best = _events(lambda: yt.augment_batch(dev_imgs, boxes, S, params=pd, mosaic=mo), a.iters)
            lines.append({"case": name + " (augment_batch call)", "batch": B, "ms_median": round(med, 4), "ms_min": round(best, 4)})
        pinned = [torch.from_numpy(i).pin_memory() for i in imgs]
        pool = torch.empty(B * h * w * 3, dtype=torch.uint8, device="cuda")

        def h2d():
            o = 0
            for t in pinned:
                n = t.numel()
                pool[o:o + n].copy_(t.reshape(-1), non_blocking=True)
                o += n
        med, best = _events(h2d, a.iters)
        lines.append({"case": f"H2D staging of {B} {w}x{h} sources (pinned)", "batch": B, "ms_median": round(med, 4),
                      "ms_min": round(best, 4), "GB_per_s": round(B * h * w * 3 / med / 1e6, 1)})
        p = yt.augment_params(4, torch.Generator().manual_seed(1)).numpy()
        p[:, 0] = p[:, 4] = p[:, 8] = 1.0
        t0 = time.perf_counter()
        ar.augment(imgs[:4], boxes[:4], p, S, S)
        lines.append({"case": f"augment_ref (numpy, CPU) {w}x{h} -> {S}x{S}", "ms_per_image": round((time.perf_counter() - t0) / 4 * 1e3, 1)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
