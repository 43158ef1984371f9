"""Times the frame front end against the loop of letterbox calls it replaces and against the floor of writing its output, in the same
process: 32 frames of 1920 x 1080 to 416 (square and rect) and 8 frames of 3840 x 2160 to 608. Per case, on device-resident frames:
FrameStager.stage of one batch tensor (one launch, no allocation) for RGB, BGR and NV12; preprocess_frames of the same RGB tensor
(the table upload and the allocations on top); letterbox over the list of the same RGB frames (one launch, four host integers and
one ctypes call per frame); and out.copy_(x), which reads and writes the bytes of the output and is the floor of writing it. From
host frames: FrameStager.stage (one pinned copy) against letterbox (one pageable copy per frame). Windows alternate round by round
between the variants, every window as many calls as fill 200 ms (at least 5) and ended by a device synchronise: "wall" is the
window's time per call, "device" the time between two events recorded around the window's calls, per call (for the one-launch
variants that is the kernel and the launch gap behind it). The median of the rounds is reported with min .. max. Every variant's
output is compared with letterbox's before it is timed. Prints one JSON line per measurement.
    python tools/frames_bench.py [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import yolo_for_turbines_amd as yt
from yolo_for_turbines_amd import _lib as L

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WINDOW_MS = 200.0
CASES = (("1080p_32_to_416", 32, 1080, 1920, 416, False), ("1080p_32_to_416_rect", 32, 1080, 1920, 416, True),
         ("2160p_8_to_608", 8, 2160, 3840, 608, False))


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
    tw, th = L.C.c_int(), L.C.c_int()
    L.lib().yolo_frames_tile(L.C.byref(tw), L.C.byref(th))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "window_ms": WINDOW_MS, "tile": [tw.value, th.value]}))
    for seed, (name, b, h, w, size, rect) in enumerate(CASES):
        g = torch.Generator().manual_seed(seed)
        rgb_host = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
        nv12_host = torch.randint(0, 256, (b, h * 3 // 2, w), generator=g, dtype=torch.uint8)
        rgb, nv12 = rgb_host.cuda(), nv12_host.cuda()
        bgr = rgb.flip(-1).contiguous()
        rgb_list, host_list = [rgb[i] for i in range(b)], [rgb_host[i] for i in range(b)]
        stagers = {f: yt.FrameStager(b, h, w, f, size, rect=rect) for f in ("rgb", "bgr", "nv12")}
        host_stager = yt.FrameStager(b, h, w, "rgb", size, rect=rect)
        want, _ = yt.letterbox(rgb_list, size, rect=rect)
        floor_dst = torch.empty_like(want)
        variants = {
            "copy_of_output": lambda: floor_dst.copy_(want),
            "stage_rgb": lambda: stagers["rgb"].stage(rgb),
            "stage_bgr": lambda: stagers["bgr"].stage(bgr),
            "stage_nv12": lambda: stagers["nv12"].stage(nv12),
            "preprocess_frames_rgb": lambda: yt.preprocess_frames(rgb, size, "rgb", rect=rect),
            "letterbox_loop_rgb": lambda: yt.letterbox(rgb_list, size, rect=rect),
            "host_stage_rgb": lambda: host_stager.stage(host_list),
            "host_letterbox_loop_rgb": lambda: yt.letterbox(host_list, size, rect=rect),
        }
        for k in ("stage_rgb", "stage_bgr", "preprocess_frames_rgb", "host_stage_rgb"):      # same bits as the loop, before any timing
            assert torch.equal(variants[k]()[0], want), k
        assert tuple(stagers["nv12"].stage(nv12)[0].shape) == tuple(want.shape)
        for fn in variants.values():
            for _ in range(3):
                fn()
        calls = {k: calls_for(fn) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):                            # alternating: every round times every variant once
            for k, fn in variants.items():
                times[k].append(window(fn, calls[k]))
        med = {k: (statistics.median(t[0] for t in v), statistics.median(t[1] for t in v)) for k, v in times.items()}
        out_bytes = want.numel() * 4
        src_bytes = {"rgb": rgb.numel(), "bgr": rgb.numel(), "nv12": nv12.numel()}
        for k, v in times.items():
            wall, dev = [t[0] for t in v], [t[1] for t in v]
            parent = "host_letterbox_loop_rgb" if k.startswith("host_") else "letterbox_loop_rgb"
            print(json.dumps({"case": name, "frames": b, "hw": [h, w], "size": size, "canvas": list(want.shape[2:]), "variant": k,
                              "wall_ms_median": round(med[k][0], 4), "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                              "device_ms_median": round(med[k][1], 4), "device_ms_min": round(min(dev), 4), "device_ms_max": round(max(dev), 4),
                              "spread_pct": round(100 * (max(wall) - min(wall)) / med[k][0], 1), "calls_per_window": calls[k],
                              "device_ratio_to_floor": round(med[k][1] / med["copy_of_output"][1], 2),
                              "wall_ratio_to_parent": round(med[k][0] / med[parent][0], 4),
                              "device_ratio_to_parent": round(med[k][1] / med[parent][1], 4),
                              "output_GBps_device": round(out_bytes / med[k][1] / 1e6, 1),
                              "source_MB": round(src_bytes[k.split("_")[1]] / 1e6, 1) if k.startswith("stage_") else None}), flush=True)
        # the two conditions of the kernel: faster than the loop by more than the spread; NV12 not slower than RGB
        lo_parent = min(t[0] for t in times["letterbox_loop_rgb"])
        hi_batched = max(t[0] for t in times["stage_rgb"])
        print(json.dumps({"case": name, "batched_beats_loop_beyond_spread": hi_batched < lo_parent, "stage_rgb_wall_max": round(hi_batched, 4),
                          "loop_wall_min": round(lo_parent, 4),
                          "nv12_not_slower_than_rgb": med["stage_nv12"][1] <= max(t[1] for t in times["stage_rgb"]),
                          "nv12_over_rgb_device": round(med["stage_nv12"][1] / med["stage_rgb"][1], 3)}), flush=True)
        del rgb, nv12, bgr, rgb_list, stagers, host_stager, want, floor_dst, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
