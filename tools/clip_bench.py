#!/usr/bin/env python3
"""Device time of gradient clipping by global norm (``yt.SGD(max_grad_norm=...)``) on the real network's parameter set, and of the
whole captured step with it.

  python tools/clip_bench.py                       the legs of the optimizer step, 5 rounds of 50 steps
  python tools/clip_bench.py --whole-step          also GraphedTrainStep at batch 32, 416 x 416, bf16, with and without max_grad_norm

Legs, on ``YOLOv3(num_classes=2)`` (222 parameters, 62 M elements), every parameter with a gradient, lr 1e-4, momentum 0.9, weight
decay 5e-4, max_grad_norm 1.0 (which bites: the multiply is the same work either way):
  launches only - the launches ``step()`` issues, re-issued from its tables without the host's walk over the parameters:
    (a0) loss-scaled, no clipping: the non-finite check + the scaled step        (what ``scaler.step`` is without max_grad_norm)
    (a1) loss-scaled, clipped: check + fp64 partial sums in one read, finalize, the clip step
    (b0) no scaler, no clipping: the plain step
    (b1) no scaler, clipped: partial sums, finalize, the clip step               (one more read of the gradients than b0)
  whole calls - what a training loop writes, host walk included, ``scaler.update()`` after each:
    (A0) ``scaler.step(opt)``                          no clipping
    (A1) ``scaler.step(opt)`` with max_grad_norm set
    (C)  ``scaler.unscale_(opt)``; ``torch.nn.utils.clip_grad_norm_``; ``scaler.step(opt)``      the only way to clip before
    (F)  ``scaler.unscale_(opt)``; ``yt.clip_grad_norm_``; ``scaler.step(opt)``                    the free function in that pattern
A leg is timed with device events around ``steps`` steps; the legs alternate inside a round and the rounds repeat. Figures are the
median [min..max] of the rounds in microseconds per step. Bytes: a step moves 20 per parameter element; the check, the partial
sums, and both in one launch each read 4.

--whole-step: two models, two captured steps, 20 replays each per round between device events, alternating.
The text goes to stdout and to --out (default profiles/clip/bench.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--whole-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip", "bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_bench: no GPU (nothing is measured without one)")
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import _lib as L
    from bench import seeded_model
    from tests import golden_inputs as gi
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = L.lib()
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

    say(f"# {torch.cuda.get_device_name(dev)}; device events around {a.steps} steps, us per step, median [min..max] of {a.rounds} rounds; "
        "the legs alternate inside a round")

    def setup(clipped, scaled):
        m = seeded_model(yt, 2, dev).train()
        gen = torch.Generator().manual_seed(1)
        for p in m.parameters():
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
        opt = yt.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0 if clipped else None)
        # a scale of 1 keeps the gradients where they are through the in-place unscale of legs C and F; growth is switched off
        scaler = yt.GradScaler(init_scale=1.0, growth_interval=10 ** 9) if scaled else None
        return m, opt, scaler

    def call(opt, scaler, clip=None):
        def run():
            if clip is not None:
                scaler.unscale_(opt)
                clip(opt.param_groups[0]["params"], 1.0)
            if scaler is None:
                opt.step()
            else:
                scaler.step(opt)
                scaler.update()
        return run

    def launches(kind):
        clipped, scaled = kind[1] == "1", kind[0] == "a"
        m, opt, scaler = setup(clipped, scaled)
        if scaled:
            scaler.scale(torch.ones((), device=dev))        # creates the scale
        real = call(opt, scaler)
        for _ in range(3):                                  # real calls: momentum buffers, tables, uploads, the clip state
            real()
        tab, st = opt._tables[0], L.current_stream()
        items, chunks, n = tab.items.data_ptr(), tab.chunks.data_ptr(), tab.chunks.shape[0]
        scale = scaler._scale.data_ptr() if scaled else 0
        flag = scaler._native_flags[id(opt)].data_ptr() if scaled else 0
        words = (flag, tab.written.data_ptr()) if scaled else (0, 0)
        cs = opt._clip

        def run():
            if clipped:
                L.check(lib.yolo_clip_norm_partials(items, chunks, n, scale, 0, cs.partials.data_ptr(), flag, 1, st))
                L.check(lib.yolo_clip_finalize(cs.partials.data_ptr(), n, 0, cs.words.data_ptr(), st))
            elif scaled:
                L.check(lib.yolo_sgd_check_finite(items, chunks, n, flag, 1, st))
            L.check(lib.yolo_sgd_step(items, len(tab.params), chunks, n, tab.hyper.data_ptr(), cs.words.data_ptr() if clipped else 0, scale, *words,
                                      0, 0, 0, 0, st))
        return run, (m, opt, scaler), sum(p.numel() for p in m.parameters())

    legs = {k: launches(k) for k in ("a0", "a1", "b0", "b1")}
    n_par = legs["a0"][2]
    for tag, clip in (("A0", None), ("A1", None), ("C", torch.nn.utils.clip_grad_norm_), ("F", yt.clip_grad_norm_)):
        m, opt, scaler = setup(tag == "A1", True)
        scaler.scale(torch.ones((), device=dev))
        legs[tag] = (call(opt, scaler, clip), (m, opt, scaler), n_par)
    t = {k: [] for k in legs}
    for k in legs:
        timed_us(legs[k][0], 5)
    for _ in range(a.rounds):
        for k in legs:
            t[k].append(timed_us(legs[k][0], a.steps))
    names = {"a0": "(a0) launches: check + scaled step", "a1": "(a1) launches: check+norm, finalize, clip step",
             "b0": "(b0) launches: plain step", "b1": "(b1) launches: norm, finalize, clip step",
             "A0": "(A0) calls: scaler.step", "A1": "(A1) calls: scaler.step, max_grad_norm=1",
             "C": "(C)  calls: unscale_ + torch clip_grad_norm_ + step", "F": "(F)  calls: unscale_ + yt.clip_grad_norm_ + step"}
    bytes_of = {"a0": 24 * n_par, "a1": 24 * n_par, "b0": 20 * n_par, "b1": 24 * n_par}
    med = {k: summary(v)[0] for k, v in t.items()}
    say(f"optimizer step: {n_par} parameter elements in {len(list(legs['a0'][1][0].parameters()))} tensors; one read of the gradients = {4 * n_par / 1e6:.0f} MB")
    for k in legs:
        md, lo, hi = summary(t[k])
        bw = f"   {bytes_of[k] / 1e9:6.3f} GB -> {bytes_of[k] / md / 1e6:5.2f} TB/s" if k in bytes_of else ""
        say(f"  {names[k]:56s} {md:9.1f} [{lo:9.1f}..{hi:9.1f}] us{bw}")
    say(f"  (a) clipping under the scaler costs {med['a1'] - med['a0']:.1f} us = {(med['a1'] - med['a0']) / med['a0'] * 100:.1f} % of check + step "
        f"(a1 / a0 = {med['a1'] / med['a0']:.3f}); the check pass alone is a0 - b0 = {med['a0'] - med['b0']:.1f} us")
    say(f"  (b) clipping without a scaler costs {med['b1'] - med['b0']:.1f} us (b1 / b0 = {med['b1'] / med['b0']:.3f}); one extra gradient read at the "
        f"check pass's rate would be {med['a0'] - med['b0']:.1f} us")
    say(f"  (c) whole calls: A1 / C = {med['A1'] / med['C']:.3f}, A1 / A0 = {med['A1'] / med['A0']:.3f}, F / C = {med['F'] / med['C']:.3f}")
    del legs
    torch.cuda.empty_cache()

    if a.whole_step:
        B, S = 32, 416
        anchors = gi.TRAIN_CASE["anchors"]
        sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).to(dev)
        x = torch.rand(B, 3, S, S, device=dev)
        tg = [torch.from_numpy(v).to(dev) for v in gi.synth_targets(B, S, 2, anchors, 3)]

        def graphed(max_norm):
            m = seeded_model(yt, 2, dev).train()
            opt = yt.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
            return yt.GraphedTrainStep(m, opt, sa, x, tg, autocast_dtype=torch.bfloat16), opt
        steps = {"max_grad_norm=None": graphed(None), "max_grad_norm=10.0": graphed(10.0)}
        tw = {k: [] for k in steps}
        for k, (st, _) in steps.items():
            timed_us(lambda: st(x, tg), 3)
        for _ in range(a.rounds):
            for k, (st, _) in steps.items():
                tw[k].append(timed_us(lambda: st(x, tg), 20))
        say(f"whole step: GraphedTrainStep, batch {B}, {S} x {S}, bf16 autocast, 20 replays per figure")
        for k in steps:
            md, lo, hi = summary(tw[k])
            say(f"  {k:20s} {md / 1e3:8.3f} [{lo / 1e3:8.3f}..{hi / 1e3:8.3f}] ms/step = {B / md * 1e6:7.1f} img/s")
        m0, m1 = summary(tw["max_grad_norm=None"])[0], summary(tw["max_grad_norm=10.0"])[0]
        opt = steps["max_grad_norm=10.0"][1]
        say(f"  (d) clipping adds {m1 - m0:.0f} us = {(m1 - m0) / m0 * 100:.2f} % of the step; last grad_norm {float(opt.grad_norm):.4g}, "
            f"clip_coef {float(opt.clip_coef):.4g}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
