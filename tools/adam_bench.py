#!/usr/bin/env python3
"""Device time of the ``yt.AdamW`` step on the real network's parameter set, against PyTorch's two implementations on the same GPU,
and of the whole captured step with it.

  python tools/adam_bench.py                       the legs of the optimizer step, 5 rounds of 50 steps
  python tools/adam_bench.py --whole-step          also GraphedTrainStep at batch 32, 416 x 416, bf16: yt.AdamW against yt.SGD

Legs, on ``YOLOv3(num_classes=2)`` (222 parameters, 62 M elements), every parameter with a gradient, lr 1e-4, weight decay 0.05:
  launches only - the launches ``yt.AdamW.step()`` issues, re-issued from its tables without the host's walk over the parameters:
    (p) plain: prepare + step                                   28 bytes per element
    (s) loss-scaled: the non-finite check, prepare + step       32
    (c) clipped (max_grad_norm 1.0): partial sums, finalize, prepare + step     32
    (e) with the weight average: prepare + step, the left-over entries and the counter   36
  whole calls - ``optimizer.step()`` as a training loop writes it, host walk included:
    (Y) ``yt.AdamW``   (T) ``torch.optim.AdamW(foreach=True)``   (F) ``torch.optim.AdamW(fused=True)``
A leg is timed with device events around ``steps`` steps; the legs alternate inside a round and the rounds repeat. Figures are the
median [min..max] of the rounds in microseconds per step. A whole call whose host side is slower than its kernels measures the host.

--whole-step: two models, two captured steps, 20 replays each per round between device events, alternating.
The text goes to stdout and to --out (default profiles/adam/bench.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SGD_STEP_US, SGD_STEP_GB = 212.0, 1.2                       # the plain SGD step on this parameter set (profiles/clip/bench.txt, leg b0)


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--whole-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam", "bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("adam_bench: no GPU (nothing is measured without one)")
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
    cfg = dict(lr=1e-4, weight_decay=0.05)

    def model():
        m = seeded_model(yt, 2, dev).train()
        gen = torch.Generator().manual_seed(1)
        for p in m.parameters():
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
        return m

    def launches(kind):
        m = model()
        opt = yt.AdamW(m.parameters(), max_grad_norm=1.0 if kind == "c" else None, **cfg)
        # a scale of 1 keeps the arithmetic that of the other legs; growth is switched off
        scaler = yt.GradScaler(init_scale=1.0, growth_interval=10 ** 9) if kind == "s" else None
        ema = yt.ModelEMA(m).attach(opt) if kind == "e" else None
        for _ in range(3):                                  # real calls: the moments, tables, uploads, the clip state
            if scaler is None:
                opt.step()
            else:
                scaler.scale(torch.ones((), device=dev))
                scaler.step(opt)
                scaler.update()
        tab, st = opt._tables[0], L.current_stream()
        items, chunks, n, k = tab.items.data_ptr(), tab.chunks.data_ptr(), tab.chunks.shape[0], len(tab.params)
        scale = scaler._scale.data_ptr() if scaler is not None else 0
        flag = scaler._native_flags[id(opt)].data_ptr() if scaler is not None else 0
        cs = opt._clip
        avg = (tab.shadows.data_ptr(), ema._state.data_ptr()) if ema is not None else (0, 0)
        rest = ema._rest({id(p) for p in tab.params}) if ema is not None else None

        def run():
            if kind == "c":
                L.check(lib.yolo_clip_norm_partials(items, chunks, n, 0, 0, cs.partials.data_ptr(), 0, 1, st))
                L.check(lib.yolo_clip_finalize(cs.partials.data_ptr(), n, 0, cs.words.data_ptr(), st))
            if kind == "s":
                L.check(lib.yolo_sgd_check_finite(items, chunks, n, flag, 1, st))
            L.check(lib.yolo_adam_prepare(items, k, tab.hyper.data_ptr(), tab.steps.data_ptr(), tab.words.data_ptr(), flag, st))
            L.check(lib.yolo_adam_step(items, k, chunks, n, tab.words.data_ptr(), scale, flag, cs.words.data_ptr() if kind == "c" else 0, *avg,
                                       1, 0, st))
            if ema is not None:
                ema._finish(rest)
        return run, (m, opt, scaler, ema), sum(p.numel() for p in m.parameters())

    def whole(make):
        m = model()
        opt = make(m.parameters())
        return opt.step, (m, opt), 0

    legs = {k: launches(k) for k in ("p", "s", "c", "e")}
    n_par = legs["p"][2]
    legs["Y"] = whole(lambda ps: yt.AdamW(ps, **cfg))
    legs["T"] = whole(lambda ps: torch.optim.AdamW(ps, foreach=True, **cfg))
    legs["F"] = whole(lambda ps: torch.optim.AdamW(ps, fused=True, **cfg))
    t = {k: [] for k in legs}
    for k in legs:
        timed_us(legs[k][0], 5)
    for _ in range(a.rounds):
        for k in legs:
            t[k].append(timed_us(legs[k][0], a.steps))
    names = {"p": "(p) launches: prepare + step", "s": "(s) launches: check, prepare + step (loss-scaled)",
             "c": "(c) launches: norm, finalize, prepare + step (clipped)", "e": "(e) launches: prepare + step + rest of the average",
             "Y": "(Y) calls: yt.AdamW.step()", "T": "(T) calls: torch.optim.AdamW(foreach=True).step()",
             "F": "(F) calls: torch.optim.AdamW(fused=True).step()"}
    bytes_of = {"p": 28 * n_par, "s": 32 * n_par, "c": 32 * n_par, "e": 36 * n_par}
    med = {k: summary(v)[0] for k, v in t.items()}
    say(f"optimizer step: {n_par} parameter elements in {len(list(legs['p'][1][0].parameters()))} tensors; 28 bytes per element = {28 * n_par / 1e9:.3f} GB")
    for k in legs:
        md, lo, hi = summary(t[k])
        bw = f"   {bytes_of[k] / 1e9:6.3f} GB -> {bytes_of[k] / md / 1e6:5.2f} TB/s" if k in bytes_of else ""
        say(f"  {names[k]:60s} {md:9.1f} [{lo:9.1f}..{hi:9.1f}] us{bw}")
    say(f"  (a) against the SGD step ({SGD_STEP_GB} GB in {SGD_STEP_US:.0f} us measured earlier, profiles/clip/bench.txt): bytes x {28 * n_par / 1e9 / SGD_STEP_GB:.2f}, "
        f"time x {med['p'] / SGD_STEP_US:.2f}")
    say(f"  (b) against PyTorch: p / T = {med['p'] / med['T']:.3f}, p / F = {med['p'] / med['F']:.3f}; whole calls Y / T = {med['Y'] / med['T']:.3f}, "
        f"Y / F = {med['Y'] / med['F']:.3f}")
    say(f"  (c) the scaler's check costs {med['s'] - med['p']:.1f} us, clipping {med['c'] - med['p']:.1f} us, the average {med['e'] - med['p']:.1f} us")
    del legs
    torch.cuda.empty_cache()

    if a.whole_step:
        B, S = 32, 416
        anchors = gi.TRAIN_CASE["anchors"]
        sa = (torch.tensor(anchors) * torch.tensor([S // 32, S // 16, S // 8]).view(3, 1, 1)).to(dev)
        x = torch.rand(B, 3, S, S, device=dev)
        tg = [torch.from_numpy(v).to(dev) for v in gi.synth_targets(B, S, 2, anchors, 3)]

        def graphed(make):
            m = seeded_model(yt, 2, dev).train()
            return yt.GraphedTrainStep(m, make(m.parameters()), sa, x, tg, autocast_dtype=torch.bfloat16)
        steps = {"yt.SGD": graphed(lambda ps: yt.SGD(ps, lr=1e-4, momentum=0.9, weight_decay=5e-4)),
                 "yt.AdamW": graphed(lambda ps: yt.AdamW(ps, **cfg))}
        tw = {k: [] for k in steps}
        for k, st in steps.items():
            timed_us(lambda: st(x, tg), 3)
        for _ in range(a.rounds):
            for k, st in steps.items():
                tw[k].append(timed_us(lambda: st(x, tg), 20))
        say(f"whole step: GraphedTrainStep, batch {B}, {S} x {S}, bf16 autocast, 20 replays per figure")
        for k in steps:
            md, lo, hi = summary(tw[k])
            say(f"  {k:20s} {md / 1e3:8.3f} [{lo / 1e3:8.3f}..{hi / 1e3:8.3f}] ms/step = {B / md * 1e6:7.1f} img/s")
        m0, m1 = summary(tw["yt.SGD"])[0], summary(tw["yt.AdamW"])[0]
        say(f"  (d) AdamW in place of SGD adds {m1 - m0:.0f} us = {(m1 - m0) / m0 * 100:.2f} % of the step")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
