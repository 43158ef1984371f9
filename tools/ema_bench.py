#!/usr/bin/env python3
"""Device time of the weight average (``yt.ModelEMA``) on the real network's parameter set, and of the whole captured step with it.

  python tools/ema_bench.py                       the four legs of the optimizer step, 5 rounds of 50 steps
  python tools/ema_bench.py --whole-step          also GraphedTrainStep at batch 32, 416 x 416, bf16, with and without ema=

Legs, on ``YOLOv3(num_classes=2)`` (222 parameters, 366 floating-point state entries), every parameter with a gradient, lr 1e-4,
momentum 0.9, weight decay 5e-4:
  (a) the ``yt.SGD`` step alone;
  (b) the step with the average attached: the fused launch plus the launch over the entries left over (BatchNorm statistics, counters);
  (c) the plain step, then one standalone ``ema.update()`` launch over everything;
  (d) the plain step, then ``torch._foreach_mul_`` / ``torch._foreach_add_`` over the 366 float entries: what a user bolts on.
Each leg first takes real ``optimizer.step()`` / ``ema.update()`` calls, which build and upload its tables. The timed part re-issues
exactly the launches those calls issue, from the same tables, without the host's walk over the parameters in front of them: that walk
takes about as long as the kernel and would be what an eager figure shows. A leg is timed with device events around 50 such steps;
the legs alternate inside a round and the rounds repeat. Figures are the median [min..max] of the rounds in microseconds per step.
Bytes: a step moves 20 per parameter element (p, g, buffer read; p, buffer written), the fused step 28 (the average read and written),
a standalone update 12 per float entry (source and average read, average written).

--whole-step: two models, two captured steps, ``steps`` replays each per round between device events, alternating.
The text goes to stdout and to --out (default profiles/ema/bench.txt)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema", "bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ema_bench: no GPU (nothing is measured without one)")
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

    # ---- the four legs of the optimizer step
    def leg(kind):
        m = seeded_model(yt, 2, dev).train()
        gen = torch.Generator().manual_seed(1)
        for p in m.parameters():
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
        opt = yt.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
        ema = yt.ModelEMA(m) if kind in "bc" else None
        if kind == "b":
            ema.attach(opt)
        src = [v for v in m.state_dict().values() if v.dtype == torch.float32]
        shadow = [v.clone() for v in src] if kind == "d" else None
        for _ in range(3):                                  # real calls: momentum buffers, tables, uploads
            opt.step()
            if kind == "c":
                ema.update()
        tab = opt._tables[0]
        st = L.current_stream()
        # yolo_sgd_step up to its options: no clip state, no scale, no found_inf, no written words
        plain = (tab.items.data_ptr(), len(tab.params), tab.chunks.data_ptr(), tab.chunks.shape[0], tab.hyper.data_ptr(), 0, 0, 0, 0)
        rest = next(iter(ema._tables.values())) if ema is not None else None
        assert ema is None or len(ema._tables) == 1

        def update_rest():
            L.check(lib.yolo_ema_update(rest.rows.data_ptr(), rest.chunks.data_ptr(), rest.chunks.shape[0], ema._state.data_ptr(), 0, 1, st))

        def run():
            if kind == "b":
                L.check(lib.yolo_sgd_step(*plain, tab.shadows.data_ptr(), ema._state.data_ptr(), 0, 0, st))
                update_rest()
                return
            L.check(lib.yolo_sgd_step(*plain, 0, 0, 0, 0, st))
            if kind == "c":
                update_rest()
            elif kind == "d":
                torch._foreach_mul_(shadow, 0.9998)
                torch._foreach_add_(shadow, src, alpha=1.0 - 0.9998)
        n_par = sum(p.numel() for p in m.parameters())
        n_float = sum(v.numel() for v in src)
        return run, n_par, n_float, (m, opt, ema, shadow)

    legs = {k: leg(k) for k in "abcd"}
    n_par, n_float = legs["a"][1], legs["a"][2]
    t = {k: [] for k in legs}
    for k in legs:
        timed_us(legs[k][0], 5)
    for _ in range(a.rounds):
        for k in legs:
            t[k].append(timed_us(legs[k][0], a.steps))
    names = {"a": "(a) yt.SGD step alone", "b": "(b) step with the average attached (fused)", "c": "(c) step + standalone ema.update()",
             "d": "(d) step + torch._foreach_mul_/_add_"}
    bytes_of = {"a": 20 * n_par, "b": 28 * n_par + 12 * (n_float - n_par), "c": 20 * n_par + 12 * n_float, "d": 20 * n_par + 20 * n_float}
    med = {k: summary(v)[0] for k, v in t.items()}
    say(f"optimizer step: {n_par} parameter elements, {n_float} float state elements")
    for k in legs:
        md, lo, hi = summary(t[k])
        say(f"  {names[k]:46s} {md:9.1f} [{lo:9.1f}..{hi:9.1f}] us   {bytes_of[k] / 1e9:6.3f} GB -> {bytes_of[k] / md / 1e6:5.2f} TB/s   "
            f"({k} - a) / a = {(md - med['a']) / med['a']:6.3f}")
    say(f"  worth fusing (b < c): {'yes' if med['b'] < med['c'] else 'NO'}; the average costs {med['b'] - med['a']:.1f} us fused, "
        f"{med['c'] - med['a']:.1f} us standalone, {med['d'] - med['a']:.1f} us as two foreach passes")
    del legs
    torch.cuda.empty_cache()

    # ---- the whole captured step
    if a.whole_step:
        B, S = 32, 416
        anchors = gi.TRAIN_CASE["anchors"]
        sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).to(dev)
        x = torch.rand(B, 3, S, S, device=dev)
        tg = [torch.from_numpy(v).to(dev) for v in gi.synth_targets(B, S, 2, anchors, 3)]

        def graphed(with_ema):
            m = seeded_model(yt, 2, dev).train()
            opt = yt.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4)
            ema = yt.ModelEMA(m) if with_ema else None
            return yt.GraphedTrainStep(m, opt, sa, x, tg, autocast_dtype=torch.bfloat16, ema=ema), ema
        steps = {"without ema=": graphed(False), "with ema=": graphed(True)}
        tw = {k: [] for k in steps}
        for k, (st, _) in steps.items():
            timed_us(lambda: st(x, tg), 3)
        for _ in range(a.rounds):
            for k, (st, _) in steps.items():
                tw[k].append(timed_us(lambda: st(x, tg), 20))
        say(f"whole step: GraphedTrainStep, batch {B}, {S} x {S}, bf16 autocast, 20 replays per figure")
        for k in steps:
            md, lo, hi = summary(tw[k])
            say(f"  {k:14s} {md / 1e3:8.3f} [{lo / 1e3:8.3f}..{hi / 1e3:8.3f}] ms/step = {B / md * 1e6:7.1f} img/s")
        m0, m1 = summary(tw["without ema="])[0], summary(tw["with ema="])[0]
        say(f"  the average adds {m1 - m0:.0f} us = {(m1 - m0) / m0 * 100:.2f} % of the step; updates counted: {steps['with ema='][1].updates}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
