"""Times training crops (CropPool.batch) against the parent's chain on the same canvas, against the torch ops a user writes today,
and against the floor of writing the output, in the same process: 32 crops of 416 x 416 from 16 device-resident 3000 x 4000 images
at scale 1 and at scale 0.5, and 16 crops of 608 x 608 at scale 1. Per case:
  pool_batch_device   pool.batch with index / crop / augmentation tables on the device and out= (three launches, no allocation);
  pool_batch_host     pool.batch with host tables (one pinned upload and the allocation of the outputs on top);
  augment_batch_precut   the parent: augment_batch over the same number of device-resident, pre-cut tile-sized images with as many
                      box rows each (its letterbox is the identity on them, so it writes the same pixels through the same chain);
                      the whole call, which builds its pool and tables anew every time, and augment_launch_precut, its three
                      launches alone;
  pool_noaug_device   pool.batch(augment=False), device tables and out= (two launches);
  torch_loop_noaug    what a user writes today without augmentation: slice, permute, float() / 255, stack (origins known on the host);
  copy_of_output      out.copy_(x), the floor of writing the output.
Windows alternate round by round between the variants, every window as many calls as fill 200 ms (at least 5) and ended by a device
synchronise: "wall" is the window's time per call, "device" the time between two events recorded around the window's calls, per
call. The median of the rounds is reported with min .. max. Every variant's output is checked before it is timed: the two pool.batch
forms against each other, at scale 1 against augment_batch of the tiles pre-cut at the same windows (bit for bit), and the
unaugmented crops against the image's own bytes. Prints one JSON line per measurement.
    python tools/crops_bench.py [rounds] [--case=N]
    python tools/crops_bench.py --trace [--case=N]     (a dozen calls of each variant in turn and no timing, for rocprofv3)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import yolo_for_turbines_amd as yt
from yolo_for_turbines_amd import data as D

TRACE = "--trace" in sys.argv
ONLY = [int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--case=")]
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
ROUNDS = int(ARGS[0]) if ARGS else 7
WINDOW_MS = 200.0
POOL_N, POOL_H, POOL_W = 16, 3000, 4000
CASES = (("416_x32_scale_1.0", 32, 416, 1.0), ("416_x32_scale_0.5", 32, 416, 0.5), ("608_x16_scale_1.0", 16, 608, 1.0))


def window(fn, calls=5):
    """(wall ms per call, device ms per call) of `calls` calls ended by a synchronise."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3, start.elapsed_time(end) / calls


def calls_for(fn):
    return max(5, min(2000, int(WINDOW_MS / window(fn)[0]) + 1))


def main():
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "window_ms": WINDOW_MS,
                      "pool": [POOL_N, POOL_H, POOL_W], "trace": TRACE}))
    torch.manual_seed(0)
    images = [torch.randint(0, 256, (POOL_H, POOL_W, 3), dtype=torch.uint8, device="cuda") for _ in range(POOL_N)]
    g = torch.Generator().manual_seed(1)
    boxes = [[[float(v) for v in 0.1 + 0.8 * torch.rand(2, generator=g)] + [0.02, 0.03, 0.0] for _ in range(8)] for _ in range(POOL_N)]
    pool = yt.CropPool(images, boxes)
    for seed, (name, B, S, scale) in enumerate(CASES):
        if ONLY and seed not in ONLY:
            continue
        g = torch.Generator().manual_seed(10 + seed)
        index = torch.randint(0, POOL_N, (B,), generator=g).to(torch.int32)
        cp = yt.crop_params(B, g, scale=(scale, scale))
        ap = yt.augment_params(B, g)
        d_index, d_cp, d_ap = index.cuda(), cp.cuda(), ap.cuda()
        out = pool.batch(B, S, index=d_index, crop_params=d_cp, params=d_ap)
        out_na = pool.batch(B, S, index=d_index, crop_params=d_cp, augment=False)
        win = out[3].cpu().tolist()
        assert all(0 <= w[1] <= w[3] - S and 0 <= w[2] <= w[4] - S for w in win)                   # every window inside its level
        # the parent's input: tiles of the canvas size, cut once (at scale 1 at the crops' own windows, so the pixels must agree)
        tiles = [images[k][(y0 if scale == 1.0 else 0):(y0 if scale == 1.0 else 0) + S,
                           (x0 if scale == 1.0 else 0):(x0 if scale == 1.0 else 0) + S].contiguous() for k, y0, x0, _, _, _ in win]
        tile_boxes = [boxes[k] for k, *_ in win]             # as many rows per tile as the crop's image has: the box kernels do equal work
        pre = D._augment_prepare(tiles, tile_boxes, S, ap, None, None, None)
        floor_dst = torch.empty_like(out[0])
        origins = [(w[0], w[1], w[2]) for w in win]

        def torch_loop():
            return torch.stack([images[k][y0:y0 + S, x0:x0 + S].permute(2, 0, 1).float() / 255 for k, y0, x0 in origins])
        variants = {
            "copy_of_output": lambda: floor_dst.copy_(out[0]),
            "pool_batch_device": lambda: pool.batch(B, S, index=d_index, crop_params=d_cp, params=d_ap, out=out),
            "pool_batch_host": lambda: pool.batch(B, S, index=index, crop_params=cp, params=ap),
            "augment_batch_precut": lambda: yt.augment_batch(tiles, tile_boxes, S, params=ap),
            "augment_launch_precut": pre[3],
            "pool_noaug_device": lambda: pool.batch(B, S, index=d_index, crop_params=d_cp, augment=False, out=out_na),
        }
        if scale == 1.0:
            variants["torch_loop_noaug"] = torch_loop
        # every variant's output, before any timing
        want = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(variants["pool_batch_device"](), want))
        assert all(torch.equal(a, b) for a, b in zip(variants["pool_batch_host"](), want))
        pre[3]()
        if scale == 1.0:
            assert torch.equal(variants["augment_batch_precut"]()[0], want[0]) and torch.equal(pre[0], want[0])
            u8 = torch.stack([images[k][y0:y0 + S, x0:x0 + S].permute(2, 0, 1) for k, y0, x0 in origins])
            assert torch.equal((variants["pool_noaug_device"]()[0] * 255).round().to(torch.uint8), u8)
            assert torch.equal((torch_loop() * 255).round().to(torch.uint8), u8)
        else:
            assert tuple(variants["augment_batch_precut"]()[0].shape) == tuple(want[0].shape)
            x_na = variants["pool_noaug_device"]()[0]
            assert bool((x_na >= 0).all()) and bool((x_na <= 1).all()) and float(x_na.mean()) > 0.4
        if TRACE:
            for _ in range(12):                            # in turn: every launch finds what the other variants left in the caches
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            continue
        for fn in variants.values():
            for _ in range(3):
                fn()
        calls = {k: calls_for(fn) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):                            # alternating: every round times every variant once
            for k, fn in variants.items():
                times[k].append(window(fn, calls[k]))
        med = {k: (statistics.median(t[0] for t in v), statistics.median(t[1] for t in v)) for k, v in times.items()}
        for k, v in times.items():
            wall, dev = [t[0] for t in v], [t[1] for t in v]
            print(json.dumps({"case": name, "crops": B, "tile": S, "scale": scale, "variant": k,
                              "wall_ms_median": round(med[k][0], 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                              "device_ms_median": round(med[k][1], 4), "device_ms_min": round(min(dev), 4), "device_ms_max": round(max(dev), 4),
                              "spread_pct": round(100 * (max(wall) - min(wall)) / med[k][0], 1), "calls_per_window": calls[k],
                              "device_ratio_to_floor": round(med[k][1] / med["copy_of_output"][1], 2),
                              "wall_ratio_to_parent_call": round(med[k][0] / med["augment_batch_precut"][0], 4),
                              "device_ratio_to_parent_launch": round(med[k][1] / med["augment_launch_precut"][1], 4)}), flush=True)
        verdict = {"case": name}
        # not slower than the parent's chain: rounds whose min .. max ranges overlap count as equal
        for parent in ("augment_launch_precut", "augment_batch_precut"):
            verdict["pool_batch_device_not_slower_than_" + parent] = \
                min(t[0] for t in times["pool_batch_device"]) <= max(t[0] for t in times[parent])
        if scale == 1.0:                                   # faster than the torch loop by more than the spread
            verdict["pool_noaug_beats_torch_loop_beyond_spread"] = \
                max(t[0] for t in times["pool_noaug_device"]) < min(t[0] for t in times["torch_loop_noaug"])
        print(json.dumps(verdict), flush=True)


if __name__ == "__main__":
    main()
