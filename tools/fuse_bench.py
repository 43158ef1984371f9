#!/usr/bin/env python3
"""Weighted box fusion (``fuse_boxes``) and test-time augmented detection (``detect_tta``): what they cost. Nothing here is a
pass / fail bar; every figure is the median [min..max] of --rounds rounds of at least --seconds of calls closed by a device
synchronise, after a warm-up, with the compared calls alternating round by round in one process.

  python tools/fuse_bench.py                      both parts
  python tools/fuse_bench.py --part a --rounds 5

(a) ``fuse_boxes`` against ``nms_indices`` on the SAME candidates, and the numpy reference of the tests (tests/fuse_ref.py) on the
    host for one image of them:
      * 16 images x 10,000 clustered boxes, 2 and 80 classes: the generator of bench.py's clustered NMS leg (60 objects per image,
        every box a jittered copy of one of them), restated below;
      * the candidates of one ``detect_tiled(scales=(1.0, 0.5))`` frame (--frame-height x --frame-width, random pixels, synthetic
        weights; the objectness threshold is the score that --pass-rate of the candidates pass).
(b) ``detect_tta`` with 2 views (none, lr) and 4 views (none, lr at scales 1.0 and 0.75) at 416 x 416, B = 8, against the same
    number of ``detect_images`` calls on the frame: the difference is what views, unmapping and fusion cost beyond the forwards.
Writes one JSON line per measurement to --out as well."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)], [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]


def boxes_clustered(np, n, nc, seed, n_gt=60, jitter=0.05):
    """bench.py's clustered NMS boxes: n_gt objects, each box a jittered same-class copy of one of them, scores in (0.5, 1]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gcx, gcy = rng.random(n_gt), rng.random(n_gt)
    gw, gh = 0.05 + 0.3 * rng.random(n_gt), 0.05 + 0.3 * rng.random(n_gt)
    gcls = rng.integers(0, nc, n_gt)
    owner = rng.integers(0, n_gt, n)
    cx = gcx[owner] + jitter * gw[owner] * rng.standard_normal(n)
    cy = gcy[owner] + jitter * gh[owner] * rng.standard_normal(n)
    w = gw[owner] * (1.0 + 0.05 * rng.standard_normal(n))
    h = gh[owner] * (1.0 + 0.05 * rng.standard_normal(n))
    obj = 0.5 + 0.5 * rng.beta(2, 2, n)
    obj = np.where(obj <= 0.5, 0.75, obj)
    return np.stack([cx, cy, w, h, obj, gcls[owner].astype(np.float64)], 1).astype(np.float32)


def timed_round(fn, seconds, torch):
    """ms per call of at least `seconds` of calls, closed by a device synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e3


def alternate(fns, rounds, seconds, torch):
    """{name: [ms per call, one per round]}: warm-up, then the calls alternate round by round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed_round(fn, seconds, torch))
    return out


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="least work per timed round")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--frame-height", type=int, default=1824)
    ap.add_argument("--frame-width", type=int, default=2736)
    ap.add_argument("--pass-rate", type=float, default=0.02, help="share of a tiled frame's candidates above the threshold of the fusion")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("fuse_bench needs the GPU: a CPU run has no timing to report")
    import yolo_for_turbines_amd as yt
    from tests import fuse_ref

    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None

    def report(name, rounds_ms, **extra):
        med, lo, hi = summary(rounds_ms)
        print(f"{name:58s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  " + "  ".join(f"{k}={v}" for k, v in extra.items()), flush=True)
        if sink:
            sink.write(json.dumps(dict(name=name, median_ms=med, min_ms=lo, max_ms=hi, rounds_ms=rounds_ms, **extra)) + "\n")
            sink.flush()

    def model(nc):
        torch.manual_seed(0)
        m = yt.YOLOv3(num_classes=nc)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 4:
                    p.normal_(0, (0.8 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
        return m.to(dev).eval()

    def part_a_case(name, cand, obj_thr, host_image):
        B, N, _ = cand.shape
        res = alternate({"nms": lambda: yt.nms_indices(cand, 0.45, obj_thr, "center"),
                         "fuse": lambda: yt.fuse_boxes(cand, 0.55, obj_thr),
                         "fuse_agnostic": lambda: yt.fuse_boxes(cand, 0.55, obj_thr, class_agnostic=True)}, args.rounds, args.seconds, torch)
        keep, kc = yt.nms_indices(cand, 0.45, obj_thr, "center")
        fused, fc, members = yt.fuse_boxes(cand, 0.55, obj_thr)
        ncand = int((cand[..., 4].double() > obj_thr).sum())
        extra = dict(images=B, boxes=N, candidates=ncand, kept_mean=round(float(kc.float().mean()), 1),
                     fused_mean=round(float(fc.float().mean()), 1))
        for k, v in res.items():
            report(f"(a) {name}: {k}", v, **extra)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = fuse_ref.fuse_ref(host_image, 0.55, obj_thr)
            t.append((time.perf_counter() - t0) * 1e3)
        assert ref[2] == int(fc[0]), "the reference and the kernel disagree on image 0"
        report(f"(a) {name}: numpy reference on the host, ONE image", t, boxes=N, fused=ref[2])

    if "a" in args.part:
        for nc, jitter in ((2, 0.15), (80, 0.05)):                        # bench.py: clustered_2_classes, clustered_80_classes
            host = np.stack([boxes_clustered(np, args.boxes, nc, 1000 + b, jitter=jitter) for b in range(args.images)])
            part_a_case(f"{args.images} x {args.boxes} clustered, {nc} classes", torch.from_numpy(host).to(dev), 0.5, host[0])
        m = model(80)
        frame = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (args.frame_height, args.frame_width, 3), dtype=np.uint8)).to(dev)
        sa = yt.scaled_anchors(ANCHORS, args.size).to(dev)
        probe = torch.rand((4, 3, args.size, args.size), generator=torch.Generator().manual_seed(2)).to(dev)
        with torch.no_grad():
            scores = yt.detect_images(m, probe, sa, 0.45, 0.0)[0][..., 4]
        thr = float(torch.quantile(scores.double().flatten().cpu()[::3], 1.0 - args.pass_rate))
        cand, _, _, ncand = yt.detect_tiled(m, frame, sa, tile=args.size, obj_threshold=thr, max_candidates=131072, scales=(1.0, 0.5))
        n = int(ncand[0])
        cand = cand[:, :n].contiguous()
        part_a_case(f"detect_tiled frame {args.frame_height} x {args.frame_width}, scales (1.0, 0.5)", cand, thr, cand[0].cpu().numpy())

    if "b" in args.part:
        m = model(80)
        x = torch.rand((args.batch, 3, args.size, args.size), generator=torch.Generator().manual_seed(3)).to(dev)
        sa = yt.scaled_anchors(ANCHORS, args.size).to(dev)
        with torch.no_grad():
            boxes = yt.detect_images(m, x, sa, 0.45, 0.0)[0]
        thr = float(torch.quantile(boxes[..., 4].double().flatten().cpu()[::7], 0.98))      # synthetic weights have no meaningful 0.5

        def images(k):
            for _ in range(k):
                yt.detect_images(m, x, sa, 0.45, thr)

        for views, kw in ((2, dict(flips=("none", "lr"), scales=(1.0,))), (4, dict(flips=("none", "lr"), scales=(1.0, 0.75)))):
            res = alternate({f"{views} x detect_images": lambda: images(views),
                             f"detect_tta, {views} views": lambda: yt.detect_tta(m, x, ANCHORS, obj_threshold=thr, **kw),
                             f"nms_indices(tta_boxes), {views} views": lambda: yt.nms_indices(yt.tta_boxes(m, x, ANCHORS, **kw), 0.45, thr, "center")},
                            args.rounds, args.seconds, torch)
            fused, fc, members = yt.detect_tta(m, x, ANCHORS, obj_threshold=thr, **kw)
            for k, v in res.items():
                report(f"(b) B = {args.batch}, {args.size} x {args.size}: {k}", v, fused_mean=round(float(fc.float().mean()), 1),
                       views=str(yt.tta_views(args.size, args.size, **kw)).replace(" ", ""))


if __name__ == "__main__":
    main()
