#!/usr/bin/env python3
"""Device time of anchor clustering (``kmeans_anchors`` / ``yolo_anchor_kmeans``).

  python tools/anchors_bench.py                         n = 10^4 and 10^6, k = 9, restarts 1 and 8, max_iter 300
  python tools/anchors_bench.py --sizes 10000 --restarts 8 --rounds 5

Per (n, restarts), boxes of tests/anchors_ref.make_boxes already on the device, one warm-up call, then --rounds rounds; every figure is
the median [min..max] of the rounds, in ms between two HIP events:
  * ``call``: the whole ``kmeans_anchors`` (row filter, upload of the draws, the launches, the one read-back that ends it);
  * ``kernels``: ``yolo_anchor_kmeans`` alone on prepared buffers (k - 1 seeding steps, max_iter Lloyd steps of two launches each, the
    fitness), the second event recorded behind the last launch;
  * ``kernels, max_iter = steps taken``: the same with max_iter set to the largest step count of the restarts, i.e. without the
    early-exit launches that follow convergence (the library enqueues max_iter steps, it never asks the device whether it is done).
Also printed: the steps every restart took, and boxes x centroids x steps per second (n k sum of the steps / kernel time).
For perspective, the wall time of the numpy restatement (tests/anchors_ref.kmeans, the same boxes and draws) at --numpy-size on this
host's CPU. The text goes to stdout and to --out (default profiles/anchors/bench.txt)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,1000000")
    ap.add_argument("--restarts", default="1,8")
    ap.add_argument("-k", type=int, default=9)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--numpy-size", type=int, default=10000, help="0: skip the numpy restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchors", "bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("anchors_bench: no GPU (nothing is measured without one)")
    import yolo_for_turbines_amd as yt
    from tests import anchors_ref as ar
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    k = a.k
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    say(f"# {torch.cuda.get_device_name(dev)}; k {k}, max_iter {a.max_iter}; ms between two HIP events, median [min..max] of {a.rounds} rounds "
        f"after one warm-up call")
    for n in (int(v) for v in a.sizes.split(",")):
        wh_host = ar.make_boxes(n, 7)
        wh = torch.from_numpy(wh_host).to(dev)
        for R in (int(v) for v in a.restarts.split(",")):
            draws = yt.anchor_draws(R, k, torch.Generator().manual_seed(11))
            res = yt.kmeans_anchors(wh, k=k, restarts=R, max_iter=a.max_iter, draws=draws)            # warm-up
            steps = res.iterations.tolist()
            t_call = [event_ms(lambda: yt.kmeans_anchors(wh, k=k, restarts=R, max_iter=a.max_iter, draws=draws)) for _ in range(a.rounds)]
            dd = draws.to(dev)
            cen = torch.empty((R, k, 2), dtype=torch.float32, device=dev)
            fit = torch.empty(R, dtype=torch.float64, device=dev)
            ints = torch.empty((2 + k, R), dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.yolo_anchor_kmeans_workspace_bytes(n, k, R)), dtype=torch.uint8, device=dev)
            stream = L.current_stream()

            def kernels(max_iter):
                L.check(lib.yolo_anchor_kmeans(wh.data_ptr(), n, k, R, dd.data_ptr(), max_iter, cen.data_ptr(), fit.data_ptr(), ints[0].data_ptr(),
                                               ints[1].data_ptr(), ints[2:].data_ptr(), ws.data_ptr(), ws.numel(), stream), "yolo_anchor_kmeans")
            t_kern, t_tight = [], []
            kernels(a.max_iter)
            for _ in range(a.rounds):                                   # the two alternate
                t_kern.append(event_ms(lambda: kernels(a.max_iter)))
                t_tight.append(event_ms(lambda: kernels(max(steps))))
            assert torch.equal(cen.cpu(), res.centroids), "the tight run must end where the full one does"
            work = n * k * sum(steps)
            say(f"n {n} restarts {R}: steps {steps} converged {res.converged.tolist()} best {res.best} fitness {float(res.fitness[res.best]):.4f}")
            for name, t in (("call", t_call), ("kernels", t_kern), (f"kernels, max_iter = steps taken ({max(steps)})", t_tight)):
                md, lo, hi = summary(t)
                say(f"  {name:44s} {md:9.3f} [{lo:9.3f}..{hi:9.3f}] ms   {work / (md * 1e-3):.3e} boxes x centroids x steps / s")
            say(f"  launches per call: {1 + 2 * (k - 1) + 2 * a.max_iter + 2}; workspace {ws.numel()} bytes")
    if a.numpy_size:
        n = a.numpy_size
        wh_host = ar.make_boxes(n, 7)
        for R in (int(v) for v in a.restarts.split(",")):
            draws = yt.anchor_draws(R, k, torch.Generator().manual_seed(11)).numpy()
            t0 = time.perf_counter()
            ref = ar.kmeans(wh_host, draws, a.max_iter)
            dt = time.perf_counter() - t0
            say(f"numpy restatement on this host's CPU, n {n} restarts {R}: {dt * 1e3:.1f} ms wall (steps {ref['iterations'].tolist()})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
