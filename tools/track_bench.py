#!/usr/bin/env python3
"""Multi-object tracking (``Tracker.update``, ``track_images``): what it costs. Nothing here is a pass / fail bar. Device times are
from HIP events around --calls calls (after a warm-up of as many), per round; every figure is the median [min..max] of --rounds.

  python tools/track_bench.py                      all parts
  python tools/track_bench.py --part a --rounds 5

(a) microseconds per ``update`` for b in {1, 8, 32, 64} streams, n in {32, 256, 2048} rows and max_tracks in {128, 512}: synthetic
    streams with about n / 2 live objects per stream that swing around their places with a period of --frames frames (so the timed
    loop over the frames is a steady state), the other rows zero; every row is passed (no keep, no count).
(b) the worst case for the matching rounds: a chain track 0, detection 0, track 1, detection 1, ... of equal boxes on a line whose
    gaps grow, so that every detection prefers the track on its left, every track the detection on ITS left, and only the first pair
    of the chain is mutual: one pair per round. The state is restored before every timed call (outside the events).
(c) ``track_images`` against ``detect_images`` at batch 32, 416 x 416 (synthetic weights; thresholds at quantiles of the scores),
    alternating round by round, ms per call closed by a device synchronise.
(d) for scale: the numpy reference of the tests (tests/track_ref.py) on the host, one stream.
Writes one JSON line per measurement to --out as well."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)], [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]


def swinging_streams(np, b, n, frames, seed):
    """(frames, b, n, 6): n // 2 objects per stream (at least one) whose sizes shrink with their number (a sparse scene: an object
    overlaps few others), swinging on a circle of a quarter of their size; scores in (0.62, 0.99); three classes; the other rows 0."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 2)
    pos = rng.uniform(0.05, 0.95, (b, k, 2))
    size = rng.uniform(0.5, 1.0, (b, k, 2)) * 0.7 / np.sqrt(k)
    phase = rng.uniform(0, 2 * np.pi, (b, k))
    score = rng.uniform(0.62, 0.99, (b, k))
    cls = rng.integers(0, 3, (b, k))
    out = np.zeros((frames, b, n, 6), np.float32)
    for t in range(frames):
        a = phase + 2 * np.pi * t / frames
        out[t, :, :k, 0] = pos[..., 0] + 0.25 * size[..., 0] * np.cos(a)
        out[t, :, :k, 1] = pos[..., 1] + 0.25 * size[..., 1] * np.sin(a)
        out[t, :, :k, 2:4] = size * (1 + rng.normal(0, 0.02, (b, k, 2)))
        out[t, :, :k, 4], out[t, :, :k, 5] = score, cls
    return out


def chain(np, links):
    """Tracks' and detections' rows (links, 6) each, for the worst case of (b)."""
    w = 0.9 / (0.35 * 2 * links + 1)
    gaps = w * (0.1 + 0.5 * np.arange(2 * links) / (2 * links))            # strictly growing, all below 0.6 w: IoU >= 0.25
    x = 0.02 + w / 2 + np.concatenate([[0.0], np.cumsum(gaps)[:-1]])
    rows = np.zeros((2 * links, 6), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = x, 0.5, w, 0.2, 0.9
    return rows[0::2].copy(), rows[1::2].copy()


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abcd")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=192, help="calls per timed round of (a); a multiple of --frames")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=0.5, help="least work per timed round of (c)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("track_bench needs the GPU: a CPU run has no timing to report")
    import yolo_for_turbines_amd as yt
    from tests import track_ref

    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def report(name, values, unit, **extra):
        med, lo, hi = summary(values)
        print(f"{name:64s} {med:10.2f} {unit}  [{lo:.2f} .. {hi:.2f}]  " + "  ".join(f"{k}={v}" for k, v in extra.items()), flush=True)
        if sink:
            sink.write(json.dumps(dict(name=name, unit=unit, median=med, min=lo, max=hi, per_round=values, **extra)) + "\n")
            sink.flush()

    def event_us(fn, calls):
        """microseconds per call of `calls` calls between two events."""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(calls):
            fn(i)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / calls

    if "a" in args.part:
        for max_tracks in (128, 512):
            for n in (32, 256, 2048):
                for b in (1, 8, 32, 64):
                    frames = torch.from_numpy(swinging_streams(np, b, n, args.frames, seed=n + b)).to(dev)
                    tr = yt.Tracker(b, max_tracks=max_tracks)
                    step = lambda i: tr.update(frames[i % args.frames])
                    event_us(step, args.calls)                             # warm-up: the tracks exist, the table is in its steady state
                    us = [event_us(step, args.calls) for _ in range(args.rounds)]
                    s = tr.slots()
                    report(f"(a) update: b = {b}, n = {n}, max_tracks = {max_tracks}", us, "us", objects=max(1, n // 2),
                           tracked_mean=round(float((s["state"] == 2).sum()) / b, 1), overflow_mean=round(float(s["overflow"].sum()) / b, 1))

    if "b" in args.part:
        for links in (32, 128, 512):
            tracks, dets = chain(np, links)
            iou = track_ref.iou_matrix(track_ref.kf_found(tracks[:, :4])[0], dets, True)
            pairs, rounds = track_ref.mutual_best_match(iou, iou > np.float32(0.2))
            assert rounds == links == len(pairs), "the chain does not need one round per pair"
            for b in (1, 64):
                tr = yt.Tracker(b, max_tracks=512)
                tr.update(torch.from_numpy(tracks).to(dev).expand(b, -1, -1))      # frame 0: confirmed at once
                saved = tr.state_dict()
                d = torch.from_numpy(dets).to(dev).expand(b, -1, -1).contiguous()
                us = []
                for _ in range(args.rounds):
                    one = []
                    for _ in range(16):
                        tr.load_state_dict(saved)
                        one.append(event_us(lambda i: tr.update(d), 1))
                    us.append(sorted(one)[len(one) // 2])
                report(f"(b) chain of {links} tracks and detections: b = {b}, max_tracks = 512", us, "us", rounds=rounds)
                tr.load_state_dict(saved)
                assert int(tr.update(d).count[0]) == links, "a track of the chain went without its detection"

    if "c" in args.part:
        torch.manual_seed(0)
        m = yt.YOLOv3(num_classes=80)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 4:
                    p.normal_(0, (0.8 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
        m = m.to(dev).eval()
        x = torch.rand((args.batch, 3, args.size, args.size), generator=torch.Generator().manual_seed(3)).to(dev)
        sa = yt.scaled_anchors(ANCHORS, args.size).to(dev)
        scores = yt.detect_images(m, x, sa, 0.45, 0.0)[0][..., 4].double().flatten().cpu()[::7]
        high, low = float(torch.quantile(scores, 0.99)), float(torch.quantile(scores, 0.97))     # synthetic weights have no meaningful 0.5
        tr = yt.Tracker(args.batch, max_tracks=512, high_threshold=high, low_threshold=low, new_threshold=high)

        def timed(fn):
            torch.cuda.synchronize()
            k, t0 = 0, time.perf_counter()
            while True:
                fn()
                k += 1
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.seconds:
                    return dt / k * 1e3

        fns = {"detect_images": lambda: yt.detect_images(m, x, sa, 0.45, low), "track_images": lambda: yt.track_images(m, x, sa, tr, 0.45)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        ms = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        res, boxes, keep, count = yt.track_images(m, x, sa, tr, 0.45)
        for k, v in ms.items():
            report(f"(c) B = {args.batch}, {args.size} x {args.size}: {k}", v, "ms", kept_mean=round(float(count.float().mean()), 1),
                   listed_mean=round(float(res.count.float().mean()), 1))

    if "d" in args.part:
        for n, max_tracks in ((32, 128), (256, 128), (2048, 512)):
            frames = swinging_streams(np, 1, n, args.frames, seed=n + 1)
            ref = track_ref.TrackerRef(1, max_tracks)
            for f in frames:
                ref.update(f)
            t = []
            for f in frames[:max(3, args.rounds)]:
                t0 = time.perf_counter()
                ref.update(f)
                t.append((time.perf_counter() - t0) * 1e3)
            report(f"(d) numpy reference on the host: b = 1, n = {n}, max_tracks = {max_tracks}", t, "ms")


if __name__ == "__main__":
    main()
