"""Times the augmentation extras (rotation, vertical flip, MixUp, Cutout; ``extra=`` of augment_batch and CropPool.batch) on the
shapes of profiles/crops/bench.txt and profiles/augment/bench.jsonl: 32 crops of 416 x 416 from 16 device-resident 3000 x 4000
images at scale 1 (``crop``), and 32 device-resident 640 x 480 images to 416 x 416, standard and mosaic rows (``augment``,
``augment_mosaic``). Everything is device-resident and only the launches are timed: ``pool.batch`` with device tables and ``out=``,
and the ``launch()`` of ``_augment_prepare``. Variants per shape:
  base           the call without ``extra`` (today's path; the only variant of ``--base``, which also runs on a tree without the
                 extras, so that the parent commit and this one can be timed in turn on one machine);
  neutral        the neutral table: the extras' kernels doing today's work (for crops: plus staging every crop);
  rotation       angles ~ U(-30, 30) on the rows whose ShiftScaleRotate is on (every second row);
  rotation_all   the same with ShiftScaleRotate on in every row, against ``neutral_all`` (the neutral table on those params);
  vflip, mixup, cutout   each alone, on every row (MixUp: partner b + 1, lambda 0.5; Cutout: 4 rectangles of side 0.15);
  all            everything at once;
  copy_of_output out.copy_(x), the floor of writing the output.
Windows alternate round by round between the variants, every window as many calls as fill 100 ms (at least 5) and ended by a device
synchronise; "device" is the time between two events around the window's calls, per call. The median of the rounds is reported with
min .. max. One JSON line per measurement.
    python tools/augx_bench.py [rounds] [--base] [--out=profiles/augx/bench.txt]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import yolo_for_turbines_amd as yt
from yolo_for_turbines_amd import data as D

BASE = "--base" in sys.argv
OUT = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(ARGS[0]) if ARGS else 7
WINDOW_MS = 100.0
B, S = 32, 416


def window(fn, calls=5):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3, start.elapsed_time(end) / calls


def extras_tables(ap):
    """name -> ((B, 29) params, (B, 24) extras): each extra alone and all together, on the drawn augmentation table ``ap``."""
    from yolo_for_turbines_amd import extras as X
    g = torch.Generator().manual_seed(7)
    neutral = X.extra_params(B, g)
    rot = X.extra_params(B, g, degrees=30.0)
    ap_all = ap.clone()
    ap_all[:, 4] = 1.0                                        # ShiftScaleRotate on in every row
    vflip = neutral.clone()
    vflip[:, X.DO_VFLIP] = 1.0
    mix = neutral.clone()
    mix[:, X.MIX_PARTNER] = (torch.arange(B, dtype=torch.float64) + 1) % B
    mix[:, X.MIX_LAMBDA] = 0.5
    cut = neutral.clone()
    cut[:, X.CUT_N] = 4.0
    for k in range(4):
        cx, cy = 0.2 + 0.2 * k, 0.8 - 0.2 * k
        cut[:, X.CUT_RECT + 4 * k:X.CUT_RECT + 4 * k + 4] = torch.tensor([cx - 0.075, cy - 0.075, cx + 0.075, cy + 0.075], dtype=torch.float64)
    every = rot.clone()
    every[:, X.DO_VFLIP:X.CUT_RECT + 16] = cut[:, X.DO_VFLIP:X.CUT_RECT + 16]
    every[:, X.DO_VFLIP] = 1.0
    every[:, X.MIX_PARTNER], every[:, X.MIX_LAMBDA] = mix[:, X.MIX_PARTNER], 0.5
    return {"neutral": (ap, neutral), "rotation": (ap, rot), "neutral_all": (ap_all, neutral), "rotation_all": (ap_all, rot),
            "vflip": (ap, vflip), "mixup": (ap, mix), "cutout": (ap, cut), "all": (ap, every)}


def shapes():
    """name -> (make(params, extra or None) -> (launch, x)): the launch-only callables of the three shapes."""
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    big = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda") for _ in range(16)]
    boxes = [[[float(v) for v in 0.1 + 0.8 * torch.rand(2, generator=g)] + [0.02, 0.03, 0.0] for _ in range(8)] for _ in range(16)]
    pool = yt.CropPool(big, boxes)
    index = torch.randint(0, 16, (B,), generator=g).to(torch.int32).cuda()
    cp = yt.crop_params(B, g).cuda()

    def crop(ap, ex):
        kw = dict(index=index, crop_params=cp, params=ap.cuda())
        if ex is not None:
            kw["extra"] = ex.cuda()
        out = pool.batch(B, S, **kw)
        return (lambda: pool.batch(B, S, out=out, **kw)), out[0]
    small = [torch.randint(0, 256, (480, 640, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    sboxes = [[[float(v) for v in 0.1 + 0.8 * torch.rand(2, generator=g)] + [0.1, 0.15, 0.0] for _ in range(8)] for _ in range(B)]
    mosaic = [[b, (b + 1) % B, (b + 2) % B, (b + 3) % B] for b in range(B)]

    def augment(rows):
        def make(ap, ex):
            pre = D._augment_prepare(small, sboxes, S, ap.cuda(), None, rows, None, *(() if ex is None else (ex.cuda(),)))
            return pre[3], pre[0]
        return make
    return {"crop": crop, "augment": augment(None), "augment_mosaic": augment(mosaic)}


def main():
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    emit({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "window_ms": WINDOW_MS, "base_only": BASE, "batch": B, "size": S})
    for seed, (name, make) in enumerate(shapes().items()):
        ap = yt.augment_params(B, torch.Generator().manual_seed(20 + seed), mosaic=name == "augment_mosaic")
        ap[:, 4] = (torch.arange(B) % 2 == 0).to(torch.float64)         # ShiftScaleRotate in every second row, as the draws average
        launch, x = make(ap, None)
        launch()
        want = x.clone()
        floor_dst = torch.empty_like(x)
        variants = {"copy_of_output": lambda: floor_dst.copy_(want), "base": launch}
        if not BASE:
            for k, (p, e) in extras_tables(ap).items():
                variants[k], xk = make(p, e)
                variants[k]()
                if k == "neutral":                           # today's bits, before any timing
                    assert torch.equal(xk, want), name
                else:
                    assert bool(torch.isfinite(xk).all()) and (k in ("neutral_all",) or not torch.equal(xk, want)), (name, k)
        for fn in variants.values():
            for _ in range(3):
                fn()
        calls = {k: max(5, min(2000, int(WINDOW_MS / window(fn)[0]) + 1)) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                times[k].append(window(fn, calls[k]))
        med = {k: statistics.median(t[1] for t in v) for k, v in times.items()}
        for k, v in times.items():
            dev = [t[1] for t in v]
            row = {"shape": name, "variant": k, "device_ms_median": round(med[k], 4), "device_ms_min": round(min(dev), 4),
                   "device_ms_max": round(max(dev), 4), "wall_ms_median": round(statistics.median(t[0] for t in v), 4),
                   "calls_per_window": calls[k], "ratio_to_floor": round(med[k] / med["copy_of_output"], 2),
                   "ratio_to_base": round(med[k] / med["base"], 3)}
            if "neutral" in med:
                row["ratio_to_neutral"] = round(med[k] / med["neutral_all" if k == "rotation_all" else "neutral"], 3)
            emit(row)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT[0])), exist_ok=True)
        with open(OUT[0], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
