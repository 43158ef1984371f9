#!/usr/bin/env python3
"""Tiled detection of full drone frames (``detect_tiled``), end to end and stage by stage.

  python tools/tiles_bench.py                           3648 x 5472, one frame and four, fp32 and bf16, tile 416, overlap 0.2, batch 32
  python tools/tiles_bench.py --frames 1 --dtypes fp32 --rounds 5
  python tools/tiles_bench.py --frames 1 --scales 1.0,0.5,0.25 --edge-margin 2.0      the pyramid and the seam test as well

Per (dtype, frames):
  * the whole ``detect_tiled`` call on frames that are already on the device, against ``detect_images`` looped over the same tiles cut
    beforehand (same model, same batch, same process). The two alternate round by round; every round is at least --seconds of calls
    closed by a device synchronise, after a warm-up. Printed: median [min..max] of the rounds in ms per call and per tile.
  * one round of ``detect_tiled`` on frames in pageable host memory (adds the pinned staging copy and the upload).
  * each stage alone, HIP events around --reps back-to-back launches on one full chunk: gather, forward, decode, collect, and the one NMS
    over (frames, max_candidates, 6). ``exposed`` is what the stages do not account for: (call - sum of the stages) per chunk, i.e. host
    time and idle gaps that the device sees. (``decode`` now marshals its arguments on every launch: not comparable with older records.)
With --scales (more than the native level) or --edge-margin, per (dtype, frames) in addition:
  * ``yolo_tile_gather_scaled`` on one chunk of tiles of every level that is not the frame itself, beside the plain gather (the
    origins of the level's grid, repeated when the level has fewer tiles than a chunk);
  * ``yolo_tile_collect_ex`` beside ``yolo_tile_collect`` on the same chunk, the seam test off and on;
  * the whole call with ``scales=(1.0,)`` against the pyramid without and with ``edge_margin``, alternating round by round as above.
The objectness threshold is taken from the model's own scores on the first chunk (--pass-rate of the rows pass), since synthetic
weights have no meaningful 0.5."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = [[(0.28, 0.22), (0.38, 0.48), (0.9, 0.78)], [(0.07, 0.15), (0.15, 0.11), (0.14, 0.29)], [(0.02, 0.03), (0.04, 0.07), (0.08, 0.06)]]


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


def event_ms(fn, reps, torch):
    """ms per launch of `reps` back-to-back launches between two events."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3648)
    ap.add_argument("--width", type=int, default=5472)
    ap.add_argument("--frames", default="1,4")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--tile", type=int, default=416)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="least work per timed round")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per stage timing")
    ap.add_argument("--pass-rate", type=float, default=0.005, help="share of the decoded rows above the objectness threshold")
    ap.add_argument("--max-candidates", type=int, default=65536)
    ap.add_argument("--scales", default="1.0", help="pyramid levels of detect_tiled, e.g. 1.0,0.5,0.25")
    ap.add_argument("--edge-margin", type=float, default=None, help="seam test of detect_tiled, pixels of the tile")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tiles_bench: no GPU (nothing is measured without one)")
    import yolo_for_turbines_amd as yt
    from oracle import net as onet
    from yolo_for_turbines_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    T_, B, cap = a.tile, a.batch, a.max_candidates
    scales = [float(v) for v in a.scales.split(",")]
    pyramid = scales != [1.0] or a.edge_margin is not None
    m = yt.YOLOv3(num_classes=a.classes)
    m.load_state_dict(onet.synth_state_dict(0, 3, a.classes, gain=0.8))
    m = m.cuda().eval()
    eng = m._engine
    sa = [s.cuda() for s in yt.scaled_anchors(ANCHORS, T_)]
    origins = yt.tile_grid(a.height, a.width, T_, a.overlap)
    per_frame = len(origins)
    gen = torch.Generator().manual_seed(1)
    host_frame = torch.randint(0, 256, (a.height, a.width, 3), dtype=torch.uint8, generator=gen)
    frame = host_frame.cuda()
    d_origins = origins.cuda()
    stream = L.current_stream()
    print(f"# {a.height} x {a.width} frame, tile {T_}, overlap {a.overlap}: {per_frame} tiles per frame; batch {B}, {a.classes} classes; "
          f"ms: median [min..max] of {a.rounds} alternating rounds of >= {a.seconds} s")

    # the tiles of one frame cut beforehand (the baseline's input), by the gather itself
    pre = torch.empty((per_frame, 3, T_, T_), dtype=torch.float32, device=dev)
    L.check(lib.yolo_tile_gather(frame.data_ptr(), a.height, a.width, d_origins.data_ptr(), per_frame, T_, T_, pre.data_ptr(), stream), "yolo_tile_gather")

    for dt in a.dtypes.split(","):
        eng.compute_dtype = None if dt == "fp32" else dt
        with torch.no_grad():
            scores = yt.detect_images(m, pre[:B], sa, 0.45, 0.0, "center")[0][..., 4].reshape(-1)
        thr = float(torch.quantile(scores.double()[:1 << 20], 1.0 - a.pass_rate))

        def baseline(frames):
            for _ in range(frames):
                for s in range(0, per_frame, B):
                    yt.detect_images(m, pre[s:s + B], sa, 0.45, thr, "center")

        for frames in (int(f) for f in a.frames.split(",")):
            imgs = [frame] * frames
            tiles, chunks = frames * per_frame, -(-frames * per_frame // B)

            def tiled(images=imgs):
                return yt.detect_tiled(m, images, sa, tile=T_, overlap=a.overlap, iou_threshold=0.45, obj_threshold=thr, batch=B,
                                       max_candidates=cap)
            for _ in range(2):                                  # warm-up: both plans, packed weights, code objects, pinned buffers
                out = tiled()
                baseline(1)
            ncand, kept = out[3].tolist(), out[2].tolist()
            t = {"detect_tiled": [], "detect_images": []}
            for _ in range(a.rounds):
                t["detect_tiled"].append(timed_round(tiled, a.seconds, torch))
                t["detect_images"].append(timed_round(lambda: baseline(frames), a.seconds, torch))
            host_ms = timed_round(lambda: tiled([host_frame] * frames), 0.0, torch)
            host_ms = timed_round(lambda: tiled([host_frame] * frames), 0.0, torch)      # the second call: pinned buffers are cached

            # ---- the stages, on one full chunk
            x = pre[:B].contiguous()
            with eng.deferred_nan(), torch.no_grad():
                preds = m(x)
                fwd = event_ms(lambda: m(x), a.reps, torch)
            n_per = sum(3 * p.shape[2] * p.shape[3] for p in preds)
            boxes = torch.empty((B, n_per, 6), dtype=torch.float32, device=dev)
            xg = torch.empty_like(x)
            gather = event_ms(lambda: L.check(lib.yolo_tile_gather(frame.data_ptr(), a.height, a.width, d_origins.data_ptr(), B, T_, T_,
                                                                   xg.data_ptr(), stream)), a.reps, torch)
            gather_scaled = {}
            for (lh, lw), org in (yt.tile_pyramid(a.height, a.width, T_, a.overlap, scales) if pyramid else []):
                if (lh, lw) == (a.height, a.width):
                    continue
                d_org = org.repeat(-(-B // len(org)), 1)[:B].contiguous().cuda()
                gather_scaled[f"{lh}x{lw}"] = event_ms(
                    lambda: L.check(lib.yolo_tile_gather_scaled(frame.data_ptr(), a.height, a.width, lh, lw, d_org.data_ptr(), B, T_, T_,
                                                                xg.data_ptr(), stream)), a.reps, torch)
            decode = event_ms(lambda: yt.boxes._decode3(preds, sa, B, boxes, n_per, stream=stream), a.reps, torch)
            d_tiles = torch.tensor([[0, int(y), int(x0), 0] for y, x0 in origins[:B].tolist()], dtype=torch.int32).cuda()
            d_hw = torch.tensor([[a.height, a.width]], dtype=torch.int32).cuda()
            cand1 = torch.zeros((1, cap, 6), dtype=torch.float32, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.yolo_tile_collect_workspace_bytes(B, n_per)), dtype=torch.uint8, device=dev)

            def collect_once():
                cnt.zero_()                                     # (a fill of 4 bytes rides along: the count must not run past cap)
                L.check(lib.yolo_tile_collect(boxes.data_ptr(), B, n_per, d_tiles.data_ptr(), d_hw.data_ptr(), 1, T_, T_, thr, cand1.data_ptr(),
                                              cap, cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream))
            collect = event_ms(collect_once, a.reps, torch)
            cand = out[0]
            nms = event_ms(lambda: yt.nms_indices(cand, 0.45, thr, "center"), max(3, a.reps // 4), torch)

            med = {k: summary(v) for k, v in t.items()}
            stages = gather + fwd + decode + collect
            call = med["detect_tiled"][0]
            exposed = (call - stages * tiles / B - nms) / chunks
            wins = min(t["detect_tiled"]) > max(t["detect_images"])
            print(f"{dt} frames {frames} ({tiles} tiles, {chunks} chunks), threshold {thr:.6f}: candidates {ncand}, kept {kept}")
            for k in t:
                md, lo, hi = med[k]
                print(f"  {k:13s} {md:9.3f} [{lo:9.3f}..{hi:9.3f}] ms per call   {md / tiles:7.4f} [{lo / tiles:7.4f}..{hi / tiles:7.4f}] ms per tile")
            print(f"  detect_tiled / detect_images {med['detect_tiled'][0] / med['detect_images'][0]:.4f}   slower beyond the spread of the rounds: {int(wins)}")
            print(f"  detect_tiled, frames in pageable host memory: {host_ms:9.3f} ms per call ({host_ms - call:+.3f} ms)")
            print(f"  stages on a chunk of {B} tiles, ms per launch (per tile): gather {gather:.4f} ({gather / B:.5f})  forward {fwd:.4f} ({fwd / B:.5f})  "
                  f"decode {decode:.4f} ({decode / B:.5f})  collect {collect:.4f} ({collect / B:.5f})  | NMS over ({frames}, {cap}, 6): {nms:.4f}")
            print(f"  share of the forward: gather {100 * gather / fwd:.2f} %  collect {100 * collect / fwd:.2f} %   exposed per chunk {exposed:.4f} ms", flush=True)
            rec = {"dtype": dt, "frames": frames, "tiles": tiles, "chunks": chunks, "threshold": thr, "candidates": ncand, "kept": kept,
                   "ms_per_call": t, "host_frames_ms": host_ms,
                   "stage_ms": {"gather": gather, "forward": fwd, "decode": decode, "collect": collect, "nms": nms},
                   "exposed_ms_per_chunk": exposed}
            if pyramid:
                # ---- the pyramid: the scaled gather beside the plain one, and whole calls against the native level alone
                for k, v in gather_scaled.items():
                    print(f"  gather of a chunk of {B} tiles of the {k} level: {v * 1e3:.1f} us (plain gather {gather * 1e3:.1f} us), "
                          f"{100 * v / fwd:.2f} % of the forward")
                per_frame_p = sum(len(o) for _, o in yt.tile_pyramid(a.height, a.width, T_, a.overlap, scales))

                def tiled_p(margin):
                    return yt.detect_tiled(m, imgs, sa, tile=T_, overlap=a.overlap, iou_threshold=0.45, obj_threshold=thr, batch=B,
                                           max_candidates=cap, scales=scales, edge_margin=margin)
                name = "pyramid" if scales != [1.0] else "scales=(1.0,)"
                variants = {"scales=(1.0,)": (tiled, tiles)}
                if scales != [1.0]:                             # with the native level alone this would be the first call again
                    variants["pyramid"] = (lambda: tiled_p(None), frames * per_frame_p)
                if a.edge_margin is not None:
                    variants[f"{name}, edge_margin={a.edge_margin:g}"] = (lambda: tiled_p(a.edge_margin), frames * per_frame_p)
                # yolo_tile_collect_ex beside yolo_tile_collect on the same chunk (level table = the frame), seam test off and on
                collect_ex = {}
                for mg in [-1.0] + ([a.edge_margin] if a.edge_margin is not None else []):
                    def collect_ex_once(mg=mg):
                        cnt.zero_()
                        L.check(lib.yolo_tile_collect_ex(boxes.data_ptr(), B, n_per, d_tiles.data_ptr(), d_hw.data_ptr(), 1, 1, T_, T_, thr, mg,
                                                         cand1.data_ptr(), cap, cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream))
                    collect_ex["off" if mg < 0 else f"{mg:g}"] = event_ms(collect_ex_once, a.reps, torch)
                print("  collect of the chunk: yolo_tile_collect %.1f us; yolo_tile_collect_ex %s" % (
                    collect * 1e3, ", ".join(f"edge_margin {k}: {v * 1e3:.1f} us" for k, v in collect_ex.items())))
                outs = {}
                for k, (fn, _) in variants.items():
                    for _ in range(2):
                        outs[k] = fn()
                tp = {k: [] for k in variants}
                for _ in range(a.rounds):
                    for k, (fn, _) in variants.items():
                        tp[k].append(timed_round(fn, a.seconds, torch))
                print(f"  levels {scales}: {per_frame_p} tiles per frame")
                for k, (_, nt) in variants.items():
                    md, lo, hi = summary(tp[k])
                    print(f"  {k:28s} {md:9.3f} [{lo:9.3f}..{hi:9.3f}] ms per call   {md / nt:7.4f} [{lo / nt:7.4f}..{hi / nt:7.4f}] ms per tile"
                          f"   candidates {outs[k][3].tolist()}, kept {outs[k][2].tolist()}")
                rec.update({"scales": scales, "edge_margin": a.edge_margin, "gather_scaled_ms": gather_scaled, "collect_ex_ms": collect_ex,
                            "pyramid_tiles": frames * per_frame_p, "pyramid_ms_per_call": tp,
                            "pyramid_candidates": {k: o[3].tolist() for k, o in outs.items()},
                            "pyramid_kept": {k: o[2].tolist() for k, o in outs.items()}})
            print(json.dumps(rec), file=sys.stderr, flush=True)
    eng.compute_dtype = None


if __name__ == "__main__":
    main()
