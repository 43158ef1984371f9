#!/usr/bin/env python3
"""Small-batch latency of the fp32 detector, end to end (single-image detection: demo.py:41-42).

  python tools/latency_bench.py                         416 and 608, batch 1, 2, 4, 8
  python tools/latency_bench.py --sizes 416 --batches 1 --rounds 7
  rocprofv3 --kernel-trace --stats ... -- python3 tools/latency_bench.py --trace latency      (25 batch-1 forwards of one setting, untimed)

Per (size, batch) three settings are timed, ``detect_images`` (forward + decode + NMS + the NaN-flag read) and ``model(x)`` alone:
  default        ModelState.latency = False
  latency        ModelState.latency = True (the layers yolo_conv_splitk_eligible lists run cut along K)
  no_winograd    a child process with YOLO_NO_WINOGRAD=1 (the switch is read when the library is loaded), the remedy from before the
                 latency mode; timed between the rounds of the other two
The settings alternate round by round in one run; every round is at least --seconds of work, closed by a device synchronise, after a
warm-up of the shape. Printed: the median and the range of the rounds in ms per call, and whether the slowest latency round beats
the fastest round of the other two (a difference larger than the spread of the same code)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)], [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]


class Leg:
    """One model in one setting; `round(what)` times at least `seconds` of calls and returns ms per call."""

    def __init__(self, latency, classes, seconds):
        import torch
        import yolo_for_turbines_amd as yt
        from oracle import net as onet
        self.torch, self.yt, self.seconds = torch, yt, seconds
        m = yt.YOLOv3(num_classes=classes)
        m.load_state_dict(onet.synth_state_dict(0, 3, classes, gain=0.8))
        self.m = m.cuda().eval()
        self.m._engine.latency = latency
        self.x = self.sa = None

    def shape(self, size, batch):
        from oracle import net as onet
        torch = self.torch
        self.x = onet.synth_input(1, batch, size).cuda()
        self.sa = [torch.tensor(a) * (size // s) for a, s in zip(ANCHORS, (32, 16, 8))]
        for what in ("detect", "forward"):                # warm-up: plan, packed weights, code objects
            for _ in range(5):
                self.call(what)
        torch.cuda.synchronize()

    def call(self, what):
        if what == "detect":
            return self.yt.detect_images(self.m, self.x, self.sa, 0.45, 0.5, "center")
        with self.torch.no_grad():
            return self.m(self.x)

    def round(self, what):
        torch = self.torch
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                self.call(what)
            n += 10
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= self.seconds:
                return dt / n * 1e3


def child_main(a):
    """The YOLO_NO_WINOGRAD=1 leg: reads "size batch what" lines, answers one ms figure per line."""
    leg = Leg(False, a.classes, a.seconds)
    cur = None
    print("ready", flush=True)
    for line in sys.stdin:
        size, batch, what = line.split()
        if cur != (size, batch):
            leg.shape(int(size), int(batch))
            cur = (size, batch)
        print(f"{leg.round(what):.6f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="416,608")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0, help="least work per timed round")
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--mode", default="true", choices=["true", "all"], help="ModelState.latency of the latency leg (all: every supported layer)")
    ap.add_argument("--trace", choices=["default", "latency"], help="run 25 forwards of one setting at the first size and batch and exit (for a kernel trace)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child_main(a)
        return
    if a.trace:
        leg = Leg(False if a.trace == "default" else (True if a.mode == "true" else "all"), a.classes, a.seconds)
        leg.shape(int(a.sizes.split(",")[0]), int(a.batches.split(",")[0]))         # (10 warm-up calls, 5 of them forwards alone)
        for _ in range(20):
            leg.call("forward")
        leg.torch.cuda.synchronize()
        return
    # the child is started before this process touches the GPU
    env = dict(os.environ, YOLO_NO_WINOGRAD="1")
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--classes", str(a.classes), "--seconds", str(a.seconds)],
                             env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        import torch
        if not torch.cuda.is_available():
            sys.exit("latency_bench: no GPU (nothing is measured without one)")
        if child.stdout.readline().strip() != "ready":
            sys.exit("latency_bench: the YOLO_NO_WINOGRAD=1 child did not start")

        def child_round(size, batch, what):
            child.stdin.write(f"{size} {batch} {what}\n")
            child.stdin.flush()
            line = child.stdout.readline()
            if not line:
                sys.exit("latency_bench: the YOLO_NO_WINOGRAD=1 child ended early")
            return float(line)
        legs = {"default": Leg(False, a.classes, a.seconds), "latency": Leg(True if a.mode == "true" else "all", a.classes, a.seconds)}
        print(f"# fp32, {a.classes} classes, latency = {a.mode}; ms per call: median [min..max] of {a.rounds} alternating rounds of >= {a.seconds} s each")
        for size in (int(s) for s in a.sizes.split(",")):
            for batch in (int(b) for b in a.batches.split(",")):
                for leg in legs.values():
                    leg.shape(size, batch)
                for what in ("detect", "forward"):
                    t = {"default": [], "latency": [], "no_winograd": []}
                    for _ in range(a.rounds):
                        t["default"].append(legs["default"].round(what))
                        t["latency"].append(legs["latency"].round(what))
                        t["no_winograd"].append(child_round(size, batch, what))
                    for v in t.values():
                        v.sort()
                    med = {k: v[len(v) // 2] for k, v in t.items()}
                    wins = t["latency"][-1] < min(t["default"][0], t["no_winograd"][0])
                    print(f"{size:4d} b{batch} {what:8s} " + "  ".join(f"{k} {med[k]:7.3f} [{t[k][0]:7.3f}..{t[k][-1]:7.3f}]" for k in t)
                          + f"  latency/default {med['latency'] / med['default']:.3f}  latency/no_winograd {med['latency'] / med['no_winograd']:.3f}"
                          + f"  beyond_spread {int(wins)}", flush=True)
                    print(json.dumps({"size": size, "batch": batch, "what": what, "ms": t}), file=sys.stderr, flush=True)
    finally:
        child.stdin.close()
        child.wait(timeout=60)


if __name__ == "__main__":
    main()
