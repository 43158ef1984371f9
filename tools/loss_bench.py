#!/usr/bin/env python3
"""Device time of the per-scale loss with and without its options (``yt.FusedYOLOLoss(box_loss=..., ...)``, `csrc/loss_iou.hip`).

  python tools/loss_bench.py                      the loss alone: three scales, batch 32, 416 x 416, nc = 2 and nc = 80
  python tools/loss_bench.py --whole-step         also GraphedTrainStep at batch 32, 416 x 416, bf16, default loss against options

Legs (forward and backward of the three scales, dL/dpred of the summed loss; predictions are fp32 normal deviates, targets
``golden_inputs.synth_targets``):
  default   ``FusedYOLOLoss()``: the reference's terms, `csrc/loss_fused.hip`
  options   ``FusedYOLOLoss("ciou", "bce", 1.5, 0.1)``; also one row per box kind
  torch     the same terms as the options leg composed from PyTorch ops under GPU autograd (`tests/loss_ref.py` on the device, fp32):
            boolean-mask gathers, so data-dependent shapes and a wait for the host at every mask
"graph" rows replay a captured HIP graph of the leg (device time of the nine launches and the autograd glue, no host in it);
"eager" rows run the Python calls (what a training loop without capture pays; the torch leg exists only in this form, it cannot
be captured). A figure is the time between device events around ``steps`` repetitions, legs alternate inside a round, rounds
repeat; printed is the median [min..max] of the rounds in microseconds per repetition.

The text goes to stdout and to --out (default profiles/loss/bench.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTIONS = dict(box_loss="ciou", obj_loss="bce", focal_gamma=1.5, label_smoothing=0.1)


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--whole-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("loss_bench: no GPU (nothing is measured without one)")
    import yolo_for_turbines_amd as yt
    from tests import golden_inputs as gi
    from tests import loss_ref
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed_us(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps

    say(f"# {torch.cuda.get_device_name(dev)}; device events around {a.steps} repetitions, us per repetition, median [min..max] of "
        f"{a.rounds} rounds; the legs alternate inside a round")
    B, S = 32, 416
    anchors = gi.TRAIN_CASE["anchors"]
    grids = [S // 32, S // 16, S // 8]
    sa = (torch.tensor(anchors) * torch.tensor(grids).view(3, 1, 1)).to(dev)

    for nc in (2, 80):
        tg = [torch.from_numpy(v).to(dev) for v in gi.synth_targets(B, S, nc, anchors, 3)]
        gen = torch.Generator().manual_seed(nc)
        preds = [torch.randn((B, 3, g, g, 5 + nc), generator=gen).to(dev).requires_grad_(True) for g in grids]
        n_obj = [int((t[..., 4] == 1).sum()) for t in tg]

        def body(loss_fn):
            def run():
                for p in preds:
                    p.grad = None
                sum(sum(loss_fn(preds[i], tg[i], sa[i])) for i in range(3)).backward()
            return run

        def graphed(run):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    run()
            torch.cuda.current_stream(dev).wait_stream(side)
            for p in preds:
                p.grad = None
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()
            return g.replay

        legs = {"default": body(yt.FusedYOLOLoss()), "options": body(yt.FusedYOLOLoss(**OPTIONS))}
        for kind in ("giou", "diou", "ciou"):
            legs[f"box_loss={kind}"] = body(yt.FusedYOLOLoss(box_loss=kind))
        runs = {f"{k}, graph": graphed(v) for k, v in legs.items()}
        runs.update({f"{k}, eager": v for k, v in legs.items() if k in ("default", "options")})
        runs["torch, eager"] = body(lambda p, t, an: loss_ref.yolo_loss_opts(p, t, an, **OPTIONS))
        t = {k: [] for k in runs}
        for k in runs:
            timed_us(runs[k], 5)
        for _ in range(a.rounds):
            for k in runs:
                t[k].append(timed_us(runs[k], a.steps))
        med = {k: summary(v)[0] for k, v in t.items()}
        say(f"loss alone, forward + backward of three scales: batch {B}, {S} x {S}, nc = {nc}, {sum(3 * B * g * g for g in grids)} cells, "
            f"object cells per scale {n_obj}")
        for k in runs:
            md, lo, hi = summary(t[k])
            say(f"  {k:22s} {md:9.1f} [{lo:9.1f}..{hi:9.1f}] us")
        say(f"  options / default (graph) = {med['options, graph'] / med['default, graph']:.3f}; options / default (eager) = "
            f"{med['options, eager'] / med['default, eager']:.3f}; torch / options (eager) = {med['torch, eager'] / med['options, eager']:.2f}; "
            f"torch (eager) / options (graph) = {med['torch, eager'] / med['options, graph']:.1f}")
        del runs, legs
        torch.cuda.empty_cache()

    if a.whole_step:
        from bench import seeded_model
        x = torch.rand(B, 3, S, S, device=dev)
        tg = [torch.from_numpy(v).to(dev) for v in gi.synth_targets(B, S, 2, anchors, 3)]

        def graphed_step(loss_fn):
            m = seeded_model(yt, 2, dev).train()
            opt = yt.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
            return yt.GraphedTrainStep(m, opt, sa, x, tg, autocast_dtype=torch.bfloat16, loss_fn=loss_fn)
        steps = {"default loss": graphed_step(yt.FusedYOLOLoss()), "with options": graphed_step(yt.FusedYOLOLoss(**OPTIONS))}
        tw = {k: [] for k in steps}
        for k, st in steps.items():
            timed_us(lambda: st(x, tg), 3)
        for _ in range(a.rounds):
            for k, st in steps.items():
                tw[k].append(timed_us(lambda: st(x, tg), 20))
        say(f"whole step: GraphedTrainStep, batch {B}, {S} x {S}, nc = 2, bf16 autocast, 20 replays per figure")
        for k in steps:
            md, lo, hi = summary(tw[k])
            say(f"  {k:14s} {md / 1e3:8.3f} [{lo / 1e3:8.3f}..{hi / 1e3:8.3f}] ms/step = {B / md * 1e6:7.1f} img/s")
        m0, m1 = summary(tw["default loss"])[0], summary(tw["with options"])[0]
        say(f"  the options add {m1 - m0:.0f} us = {(m1 - m0) / m0 * 100:.2f} % of the step")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
