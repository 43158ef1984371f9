#!/usr/bin/env python3
"""Rectangular vs square canvases: images/s of
  * fp16 ``detect_images`` (forward + decode + NMS, the Config-5 path) at batch 16, 608 x 352 vs 608 x 608;
  * the fp32 forward at batch 32, 416 x 256 vs 416 x 416;
and the per-layer time ratio (HIP events around each launch) where the speed-up falls short of the pixel ratio.
Prints one JSON line. Usage: python tools/rect_bench.py [--steps N] [--warmup W] [--per-layer]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import yolo_for_turbines_amd as yt
from oracle import net as onet

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)],
           [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]


def model(dtype):
    m = yt.YOLOv3(num_classes=80)
    m.load_state_dict(onet.synth_state_dict(0, 3, 80, gain=0.8))
    m = m.cuda().eval()
    m._engine.compute_dtype = dtype
    return m


def images_per_s(fn, batch, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return batch * steps / (time.perf_counter() - t0)


def per_layer(m, x, reps=5):
    """ms per launch of the eval plan for x (HIP events on the launch stream), in plan order. (bench.per_launch_times
    allocates square head buffers: the head launches of an H != W plan need (B, 3, Ho, Wo, .) ones.)"""
    from yolo_for_turbines_amd import _lib as L
    with torch.no_grad():
        m(x)
    plan = m._engine._plans[next(k for k in reversed(m._engine._plans) if k[0] == "eval" and k[2] == tuple(x.shape[2:4]))]
    lib, stream, n = L.lib(), L.current_stream(), len(plan.table)
    alive = []
    for k in range(plan.prog.n_pred):
        i, gh, c3 = plan.pred_ops[k]
        alive.append(torch.empty((plan.prog.B, 3, gh, plan.prog.ops[i]["Wo"], c3), dtype=torch.float32, device=plan.device))
        plan.table[i].y = alive[-1].data_ptr()
    acc = [0.0] * n
    for _ in range(reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        evs[0].record()
        for i in range(n):
            if i < plan.first:
                plan.load_input(x, stream)
            else:
                e = plan.table[i]
                L.check(lib.yolo_conv_fwd_ws(e.d, e.x, e.w_packed, e.scale, e.shift, e.residual, e.y, e.workspace, e.workspace_bytes,
                                             plan.nan_flag.data_ptr(), stream), "yolo_conv_fwd_ws")
            evs[i + 1].record()
        torch.cuda.synchronize()
        for i in range(n):
            acc[i] += evs[i].elapsed_time(evs[i + 1]) / reps
    return [round(t, 4) for t in acc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-layer", action="store_true")
    a = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    out = {}
    gen = torch.Generator().manual_seed(1)
    m16 = model("fp16")
    for H, W in ((608, 608), (352, 608)):
        x = torch.rand((16, 3, H, W), generator=gen).cuda()
        sa = [t.cuda() for t in yt.scaled_anchors(ANCHORS, H, W)]
        out[f"fp16_detect_b16_{W}x{H}_img_s"] = round(images_per_s(lambda: yt.detect_images(m16, x, sa), 16, a.steps, a.warmup), 1)
    m32 = model("fp32")
    for H, W in ((416, 416), (256, 416)):
        x = torch.rand((32, 3, H, W), generator=gen).cuda()

        def fwd():
            with torch.no_grad():
                m32(x)
        out[f"fp32_fwd_b32_{W}x{H}_img_s"] = round(images_per_s(fwd, 32, a.steps, a.warmup), 1)
        if a.per_layer:
            out[f"fp32_fwd_b32_{W}x{H}_layer_ms"] = per_layer(m32, x)
    out["detect_speedup"] = round(out["fp16_detect_b16_608x352_img_s"] / out["fp16_detect_b16_608x608_img_s"], 3)
    out["detect_pixel_ratio"] = round(608 / 352, 3)
    out["fp32_speedup"] = round(out["fp32_fwd_b32_416x256_img_s"] / out["fp32_fwd_b32_416x416_img_s"], 3)
    out["fp32_pixel_ratio"] = round(416 / 256, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
