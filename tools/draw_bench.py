"""Times draw_boxes against frames.clone() of the same tensor (the floor of the out-of-place call: it moves the same bytes) and against
the host path it replaces, in the same process: 32 frames of 1920 x 1080 with 20 and with 300 boxes each, 8 frames of 3840 x 2160 with
300 boxes each; every case in place and out of place, with and without labels. Windows alternate round by round between the
variants, every window as many calls as fill 200 ms (at least 5) and ended by a device synchronise; the median of the rounds is
reported with their spread. The host path, per frame: the copy to the host, then the numpy restatement of the contract
(tests/draw_ref.py) and, where PIL imports, PIL.ImageDraw rectangles and text. Prints one JSON line per measurement.
    python tools/draw_bench.py [rounds]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import yolo_for_turbines_amd as yt
from yolo_for_turbines_amd import _lib as L
from tests import draw_ref as R

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
WINDOW_MS = 200.0
NAMES = ["turbine", "blade", "nacelle", "tower", "dirt", "damage"]
CASES = (("1080p_32x20", 32, 1080, 1920, 20), ("1080p_32x300", 32, 1080, 1920, 300), ("2160p_8x300", 8, 2160, 3840, 300))
HOST_FRAMES = 2                # frames the host path is timed on (it is per frame and slow)


def window(fn, calls=5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def calls_for(fn):
    return max(5, min(2000, int(WINDOW_MS / window(fn)) + 1))


def make_case(b, h, w, n, seed):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    wh = 0.04 + 0.16 * torch.rand((b, n, 2), generator=g)
    xy = wh / 2 + (1 - wh) * torch.rand((b, n, 2), generator=g)
    boxes = torch.cat([xy, wh, torch.rand((b, n, 1), generator=g), torch.randint(0, len(NAMES), (b, n, 1), generator=g).float()], 2)
    return frames.cuda(), boxes.cuda()


def pil_draw(frame, rows, thickness, palette):
    from PIL import Image, ImageDraw
    im = Image.fromarray(frame)
    d = ImageDraw.Draw(im)
    h, w = frame.shape[:2]
    for x, y, bw, bh, score, cls in rows:
        colour = palette[int(cls)]
        x0, y0 = (x - bw / 2) * w, (y - bh / 2) * h
        d.rectangle([x0, y0, x0 + bw * w, y0 + bh * h], outline=colour, width=thickness)
        text = "%s %02d%%" % (NAMES[int(cls)], int(score * 100 + 0.5))
        box = d.textbbox((x0, y0), text, anchor="lb")
        d.rectangle(box, fill=colour)
        d.text((x0, y0), text, fill=(255, 255, 255), anchor="lb")
    return np.asarray(im)


def host_path(frames, boxes, font):
    """ms per frame: device -> host copy of the frame and its boxes, then the draw on the host."""
    h, w = frames.shape[1:3]
    thickness, scale = yt.draw.default_style(h, w)
    palette = yt.draw.default_palette(len(NAMES))
    out = {}
    try:
        import PIL  # noqa: F401
        kinds = ("numpy_restatement", "pil_imagedraw")
    except ImportError:
        kinds = ("numpy_restatement",)
    for kind in kinds:
        ms = []
        for i in range(HOST_FRAMES):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f, r = frames[i].cpu().numpy(), boxes[i].cpu().numpy()
            t1 = time.perf_counter()
            if kind == "numpy_restatement":
                R.draw_frame(f, r, font, class_names=NAMES, palette=palette, thickness=thickness, font_scale=scale)
            else:
                pil_draw(f, r, thickness, palette)
            ms.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        out[kind] = {"copy_ms_per_frame": round(statistics.median(m[0] for m in ms), 3), "draw_ms_per_frame": round(statistics.median(m[1] for m in ms), 3)}
    return out


def main():
    buf = L.C.create_string_buffer(95 * 8)
    L.lib().yolo_draw_font(buf)
    font = np.frombuffer(buf.raw, dtype=np.uint8).reshape(95, 8)
    tw, th = L.C.c_int(), L.C.c_int()
    L.lib().yolo_draw_tile(L.C.byref(tw), L.C.byref(th))
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "window_ms": WINDOW_MS, "tile": [tw.value, th.value],
                      "chunk": L.lib().yolo_draw_chunk()}))
    for seed, (name, b, h, w, n) in enumerate(CASES):
        frames, boxes = make_case(b, h, w, n, seed)
        work = frames.clone()                              # the in-place variants draw here, over and over: same bytes moved every call
        variants = {"clone": lambda: frames.clone()}
        for labels in (True, False):
            for inplace in (False, True):
                key = ("inplace" if inplace else "outofplace") + ("_labels" if labels else "_nolabels")
                variants[key] = (lambda labels=labels, inplace=inplace:
                                 yt.draw_boxes(work if inplace else frames, boxes, class_names=NAMES, labels=labels, inplace=inplace))
        for fn in variants.values():                       # warm-up: code objects, the name table, the palette, the allocator
            for _ in range(3):
                fn()
        changed = float((yt.draw_boxes(frames, boxes, class_names=NAMES) != frames).any(-1).float().mean())
        calls = {k: calls_for(fn) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):                            # alternating: every round times every variant once
            for k, fn in variants.items():
                times[k].append(window(fn, calls[k]))
        base = statistics.median(times["clone"])
        nbytes = frames.numel()
        for k, v in times.items():
            med = statistics.median(v)
            moved = 2 * nbytes if k == "clone" or k.startswith("outofplace") else None
            print(json.dumps({"case": name, "frames": b, "hw": [h, w], "boxes_per_frame": n, "variant": k, "ms_per_call_median": round(med, 4),
                              "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "spread_pct": round(100 * (max(v) - min(v)) / med, 1),
                              "calls_per_window": calls[k], "ratio_to_clone": round(med / base, 3),
                              "GBps_read_plus_written": round(moved / med / 1e6, 1) if moved else None,
                              "pixels_changed_share": round(changed, 4)}), flush=True)
        host = host_path(frames, boxes, font)
        dev_ms = statistics.median(times["outofplace_labels"]) / b
        for kind, v in host.items():
            total = v["copy_ms_per_frame"] + v["draw_ms_per_frame"]
            print(json.dumps({"case": name, "variant": "host_" + kind, "frames_timed": HOST_FRAMES, **v, "device_ms_per_frame": round(dev_ms, 5),
                              "host_over_device": round(total / dev_ms, 1)}), flush=True)
        del frames, boxes, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
