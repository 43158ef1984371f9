#!/usr/bin/env python3
"""Wall time of detection evaluation: one ``evaluate_detections`` at ten IoU thresholds against the ten ``calc_mAP`` calls it replaces.

  python tools/eval_bench.py                      both workloads, 7 rounds
  python tools/eval_bench.py --workloads A --rounds 3

Workloads (seeded rows of tests/eval_ref.seeded_case, already on the device, both below the 262,144-row limit of the one-sort
ordering):
  A: 2 classes, 2,000 images, about 8 ground truths and 60 detections per image;
  B: 80 classes, 500 images, about 7 ground truths and 100 detections per image.
After one warm-up of each of the three, every round runs, in this order and in the same process: one ``evaluate_detections`` at
0.50 .. 0.95; ten ``calc_mAP`` calls at the same thresholds (``calc_mAP`` and its kernels are unchanged, so this is also the figure of
the commit before ``evaluate_detections`` existed); a single ``calc_mAP`` at 0.5. Each of them ends in its own read-back, so a host
clock around the call measures all of it: class filter, sort, offsets, kernels, the copy to the host. Figures are the median
[min..max] of the rounds, in ms. The ten values of the two ways are compared for bit equality before anything is printed.
The text goes to stdout and to --out (default profiles/eval/bench.txt)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"A": dict(images=2000, nc=2, gt_mean=8, det_mean=60, seed=21), "B": dict(images=500, nc=80, gt_mean=7, det_mean=100, seed=22)}


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("eval_bench: no GPU (nothing is measured without one)")
    import yolo_for_turbines_amd as yt
    from tests import eval_ref as er
    dev = torch.device("cuda", torch.cuda.current_device())
    thr = er.DEFAULT_THRESHOLDS
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()                                          # ends in its own read-back
        return (time.perf_counter() - t0) * 1e3, out

    say(f"# {torch.cuda.get_device_name(dev)}; host clock around calls that end in their own read-back, ms, median [min..max] of {a.rounds} "
        f"rounds after one warm-up; the three alternate inside a round")
    for name in a.workloads.split(","):
        w = WORKLOADS[name]
        preds, trues = er.seeded_case(w["images"], w["nc"], w["gt_mean"], w["det_mean"], w["seed"])
        nc = w["nc"]
        pd, td = torch.tensor(preds, dtype=torch.float32, device=dev), torch.tensor(trues, dtype=torch.float32, device=dev)

        def one_pass():
            return yt.evaluate_detections(pd, td, nc, thr)

        def ten_calls():
            return torch.stack([yt.calc_mAP(pd, td, t, "center", nc) for t in thr])

        def single():
            return yt.calc_mAP(pd, td, 0.5, "center", nc)
        res, ten, _ = one_pass(), ten_calls(), single()    # warm-up
        assert torch.equal(res.map, ten), "evaluate_detections and ten calc_mAP calls disagree"
        t_one, t_ten, t_single = [], [], []
        for _ in range(a.rounds):
            t_one.append(wall_ms(one_pass)[0])
            t_ten.append(wall_ms(ten_calls)[0])
            t_single.append(wall_ms(single)[0])
        say(f"workload {name}: {nc} classes, {w['images']} images, {len(trues)} ground truths, {len(preds)} detections; "
            f"mAP@[.5:.95] {float(res.map_50_95):.4f}, mAP@.5 {float(res.map[0]):.4f} (the two ways agree bit for bit)")
        m_one = summary(t_one)[0]
        for label, t in (("evaluate_detections, ten thresholds", t_one), ("ten calc_mAP calls", t_ten), ("one calc_mAP call", t_single)):
            md, lo, hi = summary(t)
            say(f"  {label:38s} {md:10.3f} [{lo:10.3f}..{hi:10.3f}] ms   {md / m_one:7.2f} x the one pass")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
