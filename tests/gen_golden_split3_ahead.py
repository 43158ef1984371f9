"""Generate ``tests/golden/split3_ahead.json``: the sha256 of the output buffer, and the NaN flag, of conv_split3_f32 per case of
``CASES``, per tile (1, 2, 4: 128x128, 128x64, 64x64) and per weight route (split in flight, prepared planes), on the library that
``YOLO_MI355X_LIB`` names (default: the tree's own). Needs the GPU.

Run from the repo root:  ``YOLO_MI355X_LIB=/path/to/libyolo_mi355x.so python tests/gen_golden_split3_ahead.py``

The committed file was written by the library of the commit before the K step of conv_split3_f32 was rewritten to measure two and
three K steps of activations in flight (one step was kept): tests/test_gpu_split3_ahead.py asserts that the kernel
still computes those bits. Operands come from seeds, so the file holds digests only. Regenerate it only together with a change that
is meant to change the bits of the kernel.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_gpu_split3 as s3  # noqa: E402
from tests import test_gpu_split3_ready as s3r  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "split3_ahead.json")
TILES = (1, 2, 4)
ROUTES = ("inflight", "ready")
_case = s3._case

# A K step is 32 input channels of one tap. A look-ahead of AHEAD steps asks for step kt + AHEAD at the top of step kt, runs whole
# laps of AHEAD steps and writes the last AHEAD .. 2 AHEAD - 1 steps out (AHEAD = 1 in the tree: a loop and one last step; 2 and 3
# were measured against these cases too), so the number of K steps decides the path:
#   1x1 with cin 32 .. 288    1, 2, 3, 4, 5, 9 K steps: below, at and above every depth, odd and even laps (162 pixels: two M tiles of 128)
#   the others                the edges of the staging that the unconditional loads touch: ragged M and N tiles, M tiles that straddle
#                             images, taps that are padding at every border or throughout, views, residual, the upsampling store
CASES = {
    "1x1_k32": _case(2, 9, 9, 32, 64, 1, 1),
    "1x1_k64": _case(2, 9, 9, 64, 64, 1, 1),
    "1x1_k96": _case(2, 9, 9, 96, 64, 1, 1, act=2),
    "1x1_k128": _case(2, 9, 9, 128, 64, 1, 1),
    "1x1_k160": _case(2, 9, 9, 160, 64, 1, 1),
    "1x1_k288": _case(2, 9, 9, 288, 64, 1, 1),
    "1x1_25px": _case(1, 5, 5, 64, 384, 1, 1),                                               # one ragged M tile
    "1x1_straddle_cout24": _case(3, 13, 13, 96, 24, 1, 1, act=0),                            # M tiles straddle images; ragged N tile
    "1x1_cout255_head": _case(2, 13, 13, 128, 255, 1, 1, act=0, out=2),                      # ragged N tile behind a full one
    "3x3s2_7x9_k32": _case(5, 7, 9, 32, 96, 3, 2),                                           # 9 K steps, padding taps at every border
    "3x3s2_13x13_k64": _case(3, 13, 13, 64, 64, 3, 2, act=2),                                # 18 K steps
    "3x3s2_13x13_k32": _case(4, 13, 13, 32, 48, 3, 2),
    "3x3s2_7x9_k64": _case(3, 7, 9, 64, 128, 3, 2),
    "3x3s1_one_row": _case(1, 1, 40, 32, 256, 3, 1),                                         # kh = 0 and 2 are padding throughout
    "1x1_views": _case(3, 13, 13, 160, 96, 1, 1, x_pad=32, x_off=16, y_pad=40, y_off=8),
    "1x1_residual": _case(3, 13, 13, 128, 96, 1, 1, act=2, res=True, r_pad=16, r_off=4),
    "1x1_upsample": _case(2, 13, 13, 128, 128, 1, 1, out=1, y_pad=256, y_off=128),
}
# a value that is not finite in x, in a K step (6 of 9) that every depth measured asks for from inside the loop
SPECIAL = {"1x1_k288_inf": ("1x1_k288", float("inf")), "1x1_k288_nan": ("1x1_k288", float("nan"))}
NAMES = list(CASES) + list(SPECIAL)


def operands(name):
    """(case, operands) of a name of NAMES; a SPECIAL name is its base case with the value in two pixels of x."""
    base, value = SPECIAL.get(name, (name, None))
    c = CASES[base]
    ops = s3._operands(c, 9000 + sum(ord(ch) for ch in base))
    if value is not None:
        x = ops[0].clone()
        x[1, c["h"] // 2, 3, c["x_off"] + 6 * 32 + 5] = value
        x[0, 0, 0, c["x_off"] + 6 * 32] = value
        ops = (x,) + tuple(ops[1:])
    return c, ops


def launch(L, c, ops, tile, route, ready=None):
    """(output buffer on the host, NaN flag) of one launch; ready: the prepared buffer of route "ready" """
    if route == "ready":
        y, flag, rc = s3r._launch(L, c, ops, L.FLAG_SPLIT_BF16 | L.FLAG_SPLIT_WEIGHTS_READY, tile, ready=ready)
    else:
        y, flag, rc = s3._launch(L, c, ops, L.FLAG_SPLIT_BF16, tile)
    assert rc == 0, L.lib().yolo_last_error()
    return y, flag


def digest(y):
    return hashlib.sha256(y.contiguous().numpy().tobytes()).hexdigest()


def key(name, tile, route):
    return f"{name}/tile{tile}/{route}"


if __name__ == "__main__":
    from yolo_for_turbines_amd import _lib as L
    out = {}
    for name in NAMES:
        c, ops = operands(name)
        ready = s3r._prepared(L, c, ops[1])[0]
        for tile in TILES:
            for route in ROUTES:
                y, flag = launch(L, c, ops, tile, route, ready)
                if name in CASES:
                    assert flag == 0 and bool(torch.isfinite(s3._view(c, y)).all())
                else:
                    assert not bool(torch.isfinite(s3._view(c, y)).all())
                out[key(name, tile, route)] = {"sha256": digest(y), "nan_flag": flag}
        print(name, out[key(name, 1, "ready")])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes; library", L.LIB_PATH)
