#!/usr/bin/env python3
"""Single-layer conv micro-benchmark (tuning aid; calls the C-ABI directly).

  python tools/conv_bench.py --layer c52_3x3 --tile 0 --reps 20
  python tools/conv_bench.py --layer c52_s2 --tile 1,2,4 --split3 --rounds 5      (YOLO_FLAG_SPLIT_BF16; median and spread of 5 rounds)
  python tools/conv_bench.py --layer c52_s2 --tile 1,2,4 --split3-ready --rounds 5    (the same on weights split once: yolo_split3_weights)
  python tools/conv_bench.py --layer c13_3x3 --filters-ready --rounds 7 --reps 20    (tile 15 on filters transformed once: yolo_wino4_filters)
  python tools/conv_bench.py --layer c13_3x3,c19_3x3 --tile 0 --filters-appended --rounds 7    (the eval plan's route on the small maps)
  python tools/conv_bench.py --layer c52_3x3 --filters-ready --wino-split both --rounds 7 --reps 20    (tile 15 with its GEMMs on f32 MFMAs,
                                                                  then on bf16 planes: YOLO_FLAG_WINO_SPLIT_BF16, one process)
  python tools/conv_bench.py --layer c13_3x3 --tile 0 --filters-appended --wino-split both --filter-planes both --rounds 7 --reps 20
                                                                 (... and then on filter planes made once: YOLO_FLAG_FILTER_PLANES)
  python tools/conv_bench.py --splitk --rounds 7 --reps 100      (batch 1: every fp32 conv shape of the 416 and 608 networks on the
                                                                  default plan's launch and as YOLO_FLAG_SPLIT_K, alternating)
  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES ... -- python3 tools/conv_bench.py ...

Layers are the dominant YOLOv3 shapes at batch 32, 416x416.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from yolo_for_turbines_amd import _lib as L  # noqa: E402

LAYERS = {   # name: (H, cin, cout, k, stride)
    "c416_first": (416, 3, 32, 3, 1),
    "c416_s2": (416, 32, 64, 3, 2),
    "c208_1x1": (208, 64, 32, 1, 1),
    "c208_3x3": (208, 32, 64, 3, 1),
    "c208_s2": (208, 64, 128, 3, 2),
    "c104_1x1": (104, 128, 64, 1, 1),
    "c104_3x3": (104, 64, 128, 3, 1),
    "c104_s2": (104, 128, 256, 3, 2),
    "c52_1x1": (52, 256, 128, 1, 1),
    "c52_3x3": (52, 128, 256, 3, 1),
    "c52_s2": (52, 256, 512, 3, 2),
    "c26_1x1": (26, 512, 256, 1, 1),
    "c26_3x3": (26, 256, 512, 3, 1),
    "c26_s2": (26, 512, 1024, 3, 2),
    "c13_1x1": (13, 1024, 512, 1, 1),
    "c13_3x3": (13, 512, 1024, 3, 1),
    "c13_head": (13, 1024, 255, 1, 1),
    "c19_3x3": (19, 512, 1024, 3, 1),          # the 13x13 layer's place in the 608 network
    # the remaining 1x1 shapes of the neck and the other two heads
    "c52_1x1_384": (52, 384, 128, 1, 1),
    "c26_1x1_768": (26, 768, 256, 1, 1),
    "c26_1x1_256": (26, 256, 128, 1, 1),
    "c13_1x1_512": (13, 512, 256, 1, 1),
    "c26_head": (26, 512, 255, 1, 1),
    "c52_head": (52, 256, 255, 1, 1),
}
OUT_MODES = {"nhwc": L.OUT_NHWC, "up2x": L.OUT_UPSAMPLE2X, "head": L.OUT_HEAD}


def run(name, batch, tile, reps, residual, dev, dtype="fp32", split3=False, out="nhwc", rounds=1, ready=False, filters_ready=False, filters_appended=False,
        wino_split=False, filter_planes=False):
    H, cin, cout, k, s = LAYERS[name]
    lib = L.lib()
    cpad = (cin + 3) // 4 * 4
    Ho = (H + 2 * (k // 2) - k) // s + 1
    code, tdt = {"fp32": (L.F32, torch.float32), "fp16": (L.F16, torch.float16), "bf16": (L.BF16, torch.bfloat16)}[dtype]
    x = torch.randn(batch * H * H * cpad, device=dev).to(tdt)
    w = torch.randn(cout, cin, k, k, device=dev) * (1.0 / (cin * k * k)) ** 0.5
    wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, k, code), dtype=torch.uint8, device=dev)
    stream = L.current_stream()
    L.check(lib.yolo_pack_weights(w.data_ptr(), wp.data_ptr(), cout, cin, k, code, stream))
    scale = torch.rand(cout, device=dev) + 0.5
    shift = torch.randn(cout, device=dev) * 0.1
    y = torch.empty(batch * Ho * Ho * cout * (4 if out == "up2x" else 1), device=dev, dtype=tdt if out != "head" else torch.float32)
    r = torch.randn(batch * Ho * Ho * cout, device=dev).to(tdt) if residual else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    d = L.ConvDesc(n=batch, h=H, w=H, cin=cin, cout=cout, ksize=k, stride=s, x_ld=cpad, x_off=0, y_ld=cout, y_off=0,
                   r_ld=cout, r_off=0, act=L.ACT_NONE if out == "head" else L.ACT_LEAKY, out_mode=OUT_MODES[out], dtype=code,
                   flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK | (L.FLAG_SPLIT_BF16 if split3 else 0), tile=tile)
    if ready:                                                     # the bf16 planes of the weights, made once, in place of wp
        d.flags |= L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY
        ws3 = torch.empty(lib.yolo_split3_weight_bytes(d), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_split3_weights(d, wp.data_ptr(), ws3.data_ptr(), stream), "yolo_split3_weights")
        wp = ws3
    if filters_ready:                                             # Winograd F(4x4) on filters transformed once, in place of wp
        d.flags |= L.FLAG_FILTERS_READY
        d.tile = 15
        nu = lib.yolo_wino4_filter_bytes(d)
        u4 = torch.empty(nu + (lib.yolo_wino4_filter_plane_bytes(d) if filter_planes else 0), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_wino4_filters(d, wp.data_ptr(), u4.data_ptr(), stream), "yolo_wino4_filters")
        wp, u4_at = u4, u4.data_ptr()
    if filters_appended:                                         # the route of the eval plan: U4 in place behind the packed weights, tile as given
        d.flags |= L.FLAG_FILTERS_APPENDED
        na, nu = lib.yolo_wino4_appended_bytes(d), lib.yolo_wino4_filter_bytes(d)
        wa = torch.empty(na + (lib.yolo_wino4_filter_plane_bytes(d) if filter_planes else 0), dtype=torch.uint8, device=dev)
        wa[:wp.numel()] = wp
        L.check(lib.yolo_wino4_filters(d, wa.data_ptr(), wa.data_ptr() + na - nu, stream), "yolo_wino4_filters")
        wp, u4_at = wa, wa.data_ptr() + na - nu
    if filter_planes:                                             # the bf16 planes of U4 made once, directly behind it
        d.flags |= L.FLAG_FILTER_PLANES
        L.check(lib.yolo_wino4_filter_planes(d, u4_at, u4_at + nu, stream), "yolo_wino4_filter_planes")

    if wino_split:                                                # the 36 GEMMs of tile 15 on bf16 planes (with either filter flag)
        d.flags |= L.FLAG_WINO_SPLIT_BF16

    need = lib.yolo_conv_workspace_bytes(d)                       # > 0: Winograd (tile 13, or the heuristic's choice for tile 0)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def launch():
        L.check(lib.yolo_conv_fwd_ws(d, x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(), L.ptr(r),
                                     y.data_ptr(), ws.data_ptr() if need else 0, need, flag.data_ptr(), stream), "conv")
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps)
    times.sort()
    ms = times[len(times) // 2]                                   # median round
    run.rounds = list(times)                                      # (for drivers that want the spread as numbers)
    gflop = 2.0 * batch * Ho * Ho * cout * cin * k * k / 1e9
    picked = (lib.yolo_conv_pick_tile(d) if dtype == "fp32" else 0) if d.tile == 0 else d.tile
    cut = ""
    if split3 or ready:
        cut += f"  split3{'-ready' if ready else ''} (tile {tile})"
    if out != "nhwc" or residual:
        cut += f"  out={out}" + (" +res" if residual else "")
    if rounds > 1:
        cut += f"  rounds min/max {times[0] * 1e3:.1f}/{times[-1] * 1e3:.1f} us"
    if picked == 15:                                              # Winograd F(4x4): how the launch is cut on this device
        whole, half = C.c_int(), C.c_int()
        L.check(lib.yolo_conv_wino4_blocks(d, C.byref(whole), C.byref(half)), "yolo_conv_wino4_blocks")
        cut += f"  tile blocks: {whole.value} whole + {half.value} in halves" + ("  filters ready" if filters_ready else "") + ("  filters appended" if filters_appended else "") + ("  bf16 planes" if wino_split else "") + ("  filter planes once" if filter_planes else "")
    print(f"{name:12s} tile={picked} {ms * 1e3:8.1f} us  {gflop / ms:7.2f} TFLOP/s  ({gflop:.1f} GFLOP){cut}", flush=True)
    return ms


def splitk_table(dev, reps, rounds, sizes=(416, 608)):
    """Batch 1, every distinct fp32 conv launch of the default eval plan (its flags, its prepared weights, its workspace) against the
    same launch with YOLO_FLAG_SPLIT_K, on the plan's own buffers after one forward. The two are timed in alternating rounds of
    `reps` back-to-back launches; a shape counts as faster cut along K when the slowest split-K round beats the fastest default
    round, i.e. by more than the spread that rounds of the same code show."""
    import yolo_for_turbines_amd as yt
    lib = L.lib()
    stream = L.current_stream()
    model = yt.YOLOv3(num_classes=80).to(dev).eval()
    print(f"# batch 1, {rounds} alternating rounds of {reps} launches; us per launch: median [min..max]; S = K slices, blocks = workgroups "
          "of the first split-K launch; wins = max(split-K) < min(default)")
    print("# size  h    w   cin  cout k s out res | default: tile flags   med     min     max | split-K: S blocks   med     min     max | ratio wins")
    for size in sizes:
        x = torch.rand(1, 3, size, size, device=dev)
        with torch.no_grad():
            preds = model(x)                                          # builds the plan, packs the weights, leaves real activations
        plan = list(model._engine._plans.values())[-1]
        seen = set()
        for i in range(plan.first, len(plan.table)):
            e = plan.table[i]
            d = e.d
            res = bool(d.flags & L.FLAG_RESIDUAL)
            key = (d.h, d.w, d.cin, d.cout, d.ksize, d.stride, d.out_mode, res, d.act)
            if key in seen or not lib.yolo_conv_splitk_supported(C.byref(d)):
                continue
            seen.add(key)
            base = (L.ConvOp * 1)()
            C.memmove(base, C.byref(e), C.sizeof(L.ConvOp))
            sk = (L.ConvOp * 1)()
            C.memmove(sk, C.byref(e), C.sizeof(L.ConvOp))
            sk[0].d.flags = (d.flags & (L.FLAG_RESIDUAL | L.FLAG_NANCHECK)) | L.FLAG_SPLIT_K
            sk[0].w_packed = model._engine.packed(plan.blocks[i], dev).w.data_ptr()
            need = lib.yolo_conv_workspace_bytes(C.byref(sk[0].d))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            sk[0].workspace, sk[0].workspace_bytes = ws.data_ptr(), need
            flag = plan.nan_flag.data_ptr()

            def timed(op):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    L.check(lib.yolo_conv_fwd_batch(op, 1, flag, stream), "conv")
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps * 1e3
            for op in (base, sk):
                for _ in range(5):
                    L.check(lib.yolo_conv_fwd_batch(op, 1, flag, stream), "conv")
            torch.cuda.synchronize()
            tb, tk = [], []
            for _ in range(rounds):
                tb.append(timed(base))
                tk.append(timed(sk))
            tb.sort()
            tk.sort()
            S = lib.yolo_conv_splitk_slices(C.byref(d))
            pad = d.ksize // 2
            ho, wo = (d.h + 2 * pad - d.ksize) // d.stride + 1, (d.w + 2 * pad - d.ksize) // d.stride + 1
            blocks = -(-ho * wo // 64) * -(-d.cout // 64) * S
            mb, mk = tb[len(tb) // 2], tk[len(tk) // 2]
            print(f"{size:5d} {d.h:4d} {d.w:4d} {d.cin:5d} {d.cout:5d} {d.ksize} {d.stride} {d.out_mode:3d} {int(res):3d} | "
                  f"{lib.yolo_conv_pick_tile(C.byref(d)):13d} {d.flags:5d} {mb:7.1f} {tb[0]:7.1f} {tb[-1]:7.1f} | "
                  f"{S:10d} {blocks:6d} {mk:7.1f} {tk[0]:7.1f} {tk[-1]:7.1f} | {mk / mb:5.2f} {int(tk[-1] < tb[0])}", flush=True)
        del preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layer", default="all")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile", default="0", help="tile id, comma list, or 'all'")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--residual", action="store_true")
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--split3", action="store_true", help="set YOLO_FLAG_SPLIT_BF16 (tile 0, 1, 2 or 4)")
    ap.add_argument("--split3-ready", action="store_true", help="YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY on prepared weights")
    ap.add_argument("--filters-ready", action="store_true", help="tile 15 with YOLO_FLAG_FILTERS_READY on filters made once (yolo_wino4_filters)")
    ap.add_argument("--filters-appended", action="store_true", help="YOLO_FLAG_FILTERS_APPENDED: U4 made in place behind the packed weights (tile 0: the eval plan's route)")
    ap.add_argument("--wino-split", nargs="?", const="on", default="off", choices=["off", "on", "both"],
                    help="YOLO_FLAG_WINO_SPLIT_BF16 on a --filters-ready / --filters-appended launch; 'both': without it, then with it")
    ap.add_argument("--filter-planes", nargs="?", const="on", default="off", choices=["off", "on", "both"],
                    help="YOLO_FLAG_FILTER_PLANES on a --wino-split launch: the planes of U4 made once (yolo_wino4_filter_planes); 'both': "
                         "every launch splitting its filters, then on the planes made once")
    ap.add_argument("--out", default="nhwc", choices=list(OUT_MODES))
    ap.add_argument("--rounds", type=int, default=1, help="timed rounds of --reps launches; the median is reported")
    ap.add_argument("--splitk", action="store_true", help="batch-1 table: the default plan's launch against YOLO_FLAG_SPLIT_K, per conv shape")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.splitk:
        splitk_table(dev, a.reps, a.rounds)
        return
    names = list(LAYERS) if a.layer == "all" else a.layer.split(",")
    nt = L.lib().yolo_conv_num_tiles()
    tiles = list(range(1, nt + 1)) if a.tile == "all" else [int(t) for t in a.tile.split(",")]
    for n in names:
        for t in tiles:
            for ws in {"off": (False,), "on": (True,), "both": (False, True)}[a.wino_split]:
                for fp in {"off": (False,), "on": (True,), "both": (False, True)}[a.filter_planes] if ws else (False,):
                    run(n, a.batch, t, a.reps, a.residual, dev, a.dtype, a.split3, a.out, a.rounds, a.split3_ready, a.filters_ready, a.filters_appended,
                        ws, fp)


if __name__ == "__main__":
    main()
