"""Generate ``tests/golden/wino4s_ring.json``: the sha256 of the output bytes of conv_wino4s_f32 (Winograd F(4x4) on bf16 planes made
once) per case of ``CASES``, on the library that ``YOLO_MI355X_LIB`` names (default: the tree's own). Needs the GPU.

Run from the repo root:  ``YOLO_MI355X_LIB=/path/to/libyolo_mi355x.so python tests/gen_golden_wino4s_ring.py``

The committed file was written by the library of the commit before the ring of conv_wino4s_f32 went from four slots drained at
every pass boundary to six slots carried across the passes: tests/test_gpu_wino4_ring.py asserts that the kernel still computes
those bits. Inputs come from seeds (``Case``), so the file holds digests only. Regenerate it only together with a change that is
meant to change the bits of the kernel.
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

OUT = os.path.join(ROOT, "tests", "golden", "wino4s_ring.json")

# (B, H, W, cin, cout, residual). A ring stage is one xi x 32 input channels and a pass is 6 * cin / 32 stages, requested five ahead:
#   cin 32    a pass is one lap of the ring: every request but the first of a pass crosses a pass boundary
#   cin 64, 96, 160    two, three and five (odd) laps
#   4 x 4 at batch 1      one tile
#   32 x 32 at batch 1    64 tiles: one tile block, full
#   24 x 24 at batch 2    72 tiles: a full tile block and one of 8 tiles, whose second half workgroup has no tile
#   cout 80   a partial channel block behind a full one
# On a device with more than four compute units all of these run as half workgroups (four computing waves, three that only move
# V pieces, one idle). The last case is 129 tile blocks of 64 tiles, more than half the compute units of any device this runs on:
# whole workgroups, all eight waves computing and moving.
CASES = [
    (1, 4, 4, 32, 64, False), (1, 32, 32, 32, 80, True), (2, 24, 24, 32, 64, True),
    (1, 4, 4, 64, 80, True), (1, 32, 32, 64, 64, False), (2, 24, 24, 64, 80, False),
    (1, 4, 4, 96, 64, True), (1, 32, 32, 96, 80, False), (2, 24, 24, 96, 80, True),
    (1, 4, 4, 160, 80, False), (1, 32, 32, 160, 64, True), (2, 24, 24, 160, 64, False),
    (2064, 8, 8, 32, 64, False),
]


def case_id(case):
    B, H, W, cin, cout, residual = case
    return f"{B}x{H}x{W}_{cin}to{cout}" + ("_res" if residual else "")


class Case:
    """One 3x3 stride-1 layer (leaky ReLU, NaN check) on the device: seeded operands, U4 and its bf16 planes made once."""

    def __init__(self, L, case):
        B, H, W, cin, cout, residual = case
        self.L, self.lib, self.dev, self.st, self.case = L, L.lib(), torch.device("cuda:0"), L.current_stream(), case
        g = torch.Generator().manual_seed(5150 + 7 * B + 11 * H + 13 * W + 17 * cin + 19 * cout + residual)
        self.x = torch.randn((B, H, W, cin), generator=g)
        self.w = torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5
        self.scale, self.shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        self.r = torch.randn((B, H, W, cout), generator=g) if residual else None
        dev, lib = self.dev, self.lib
        self.xd, self.sd, self.shd = self.x.to(dev), self.scale.to(dev), self.shift.to(dev)
        self.rd = self.r.to(dev) if residual else None
        d = self.desc(L.FLAG_FILTERS_READY)
        wp = torch.empty(lib.yolo_packed_weight_bytes(cout, cin, 3, L.F32), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_pack_weights(self.w.to(dev).data_ptr(), wp.data_ptr(), cout, cin, 3, L.F32, self.st), "yolo_pack_weights")
        nu = lib.yolo_wino4_filter_bytes(d)
        self.u4 = torch.empty(nu + lib.yolo_wino4_filter_plane_bytes(d), dtype=torch.uint8, device=dev)
        L.check(lib.yolo_wino4_filters(d, wp.data_ptr(), self.u4.data_ptr(), self.st), "yolo_wino4_filters")
        L.check(lib.yolo_wino4_filter_planes(d, self.u4.data_ptr(), self.u4.data_ptr() + nu, self.st), "yolo_wino4_filter_planes")
        self.ws = torch.empty(lib.yolo_conv_workspace_bytes(self.planes_desc()), dtype=torch.uint8, device=dev)

    def desc(self, flags):
        L = self.L
        B, H, W, cin, cout, residual = self.case
        return L.ConvDesc(n=B, h=H, w=W, cin=cin, cout=cout, ksize=3, stride=1, x_ld=cin, y_ld=cout, r_ld=cout if residual else 0, act=1,
                          out_mode=L.OUT_NHWC, dtype=L.F32, tile=15, flags=(L.FLAG_RESIDUAL if residual else 0) | L.FLAG_NANCHECK | flags)

    def planes_desc(self):
        L = self.L
        return self.desc(L.FLAG_FILTERS_READY | L.FLAG_WINO_SPLIT_BF16 | L.FLAG_FILTER_PLANES)

    def run(self, d=None):
        """(y on the device, in a fresh buffer of NaNs; the NaN flag) of one launch"""
        L, lib = self.L, self.lib
        B, H, W, cin, cout, residual = self.case
        d = d or self.planes_desc()
        assert lib.yolo_conv_workspace_bytes(d) <= self.ws.numel()
        y = torch.full((B, H, W, cout), float("nan"), device=self.dev)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        L.check(lib.yolo_conv_fwd_ws(d, self.xd.data_ptr(), self.u4.data_ptr(), self.sd.data_ptr(), self.shd.data_ptr(),
                                     self.rd.data_ptr() if residual else 0, y.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                     flag.data_ptr(), self.st), "yolo_conv_fwd_ws")
        return y, flag


def digest(y):
    return hashlib.sha256(y.cpu().contiguous().numpy().tobytes()).hexdigest()


if __name__ == "__main__":
    from yolo_for_turbines_amd import _lib as L
    out = {}
    for case in CASES:
        y, flag = Case(L, case).run()
        torch.cuda.synchronize()
        assert int(flag.item()) == 0 and bool(torch.isfinite(y).all())
        out[case_id(case)] = digest(y)
        print(case_id(case), out[case_id(case)])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes; library", L.LIB_PATH)
