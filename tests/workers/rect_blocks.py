#!/usr/bin/env python3
"""(Test infrastructure: used in-process by tests/test_gpu_rect.py and run as a child process under the kernel-selection
switches, which the library reads once at load.) Every conv kernel family the heuristics pick, on rectangular maps with odd
grids (11 x 19, 19 x 11, 22 x 38 ...), in fp32 / bf16 / fp16: eval forward (fp32 also with every forced tile), and the
train-mode forward with its input and weight gradients, against an fp64 CPU convolution. Prints one JSON line of the
worst errors relative to each bar (<= 1 passes)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import torch.nn.functional as F

# (name, B, H, W, cin, cout, k, stride, bn): what each is meant to reach in the default selection
CASES = [
    ("stem_3_32", 2, 22, 38, 3, 32, 3, 1, True),            # stem3x3_f32 / stem3x3_mfma_h16, wgrad_stem_h16
    ("ws_32_64", 2, 22, 38, 32, 64, 3, 1, True),             # conv3_ws_h16 (<= 64 channels, weights in registers)
    ("s2_64_128", 2, 22, 38, 64, 128, 3, 2, True),           # stride 2: gathered-row conv1_dma_h16, dgrad_s2
    ("dma_128_256_11x19", 2, 11, 19, 128, 256, 3, 1, True),  # conv3_dma_h16; fp32 two-pass Winograd (<= 256 pixels)
    ("dma_128_256_19x11", 2, 19, 11, 128, 256, 3, 1, True),
    ("wino_64_128_22x38", 2, 22, 38, 64, 128, 3, 1, True),   # fp32 one-pass Winograd; conv3_dma_h16
    ("c1_256_128", 2, 11, 19, 256, 128, 1, 1, True),         # 1x1: conv1_dma_h16 / conv1_rs_f32, wgrad_dma_h16
    ("head_256_21", 2, 19, 11, 256, 21, 1, 1, False),        # detection head (conv + bias)
]
FWD_BAR = {"fp32": 1e-4, "bf16": 2.5e-2, "fp16": 4e-3}      # max abs error / max |ref|
GRAD_BAR = {"fp32": 2e-3, "bf16": 9e-2, "fp16": 6e-2}       # fp32: max error / max |ref|; 16-bit: relative L2 (LeakyReLU branch flips)


def _make(yt, c, seed):
    name, B, H, W, cin, cout, k, s, bn = c
    g = torch.Generator().manual_seed(seed)
    blk = yt.CNNBlock(cin, cout, batch_norm_act=bn, kernel_size=k, stride=s, padding=k // 2)
    with torch.no_grad():
        blk.conv.weight.copy_(torch.randn(blk.conv.weight.shape, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        if bn:
            blk.batch_norm.weight.copy_(1 + 0.2 * torch.randn(cout, generator=g))
            blk.batch_norm.bias.copy_(0.2 * torch.randn(cout, generator=g))
            blk.batch_norm.running_mean.copy_(0.1 * torch.randn(cout, generator=g))
            blk.batch_norm.running_var.copy_(1 + 0.5 * torch.rand(cout, generator=g))
        else:
            blk.conv.bias.copy_(0.1 * torch.randn(cout, generator=g))
    x = torch.randn((B, cin, H, W), generator=g)
    return blk, x


def _ref(blk, x, train):
    """fp64 CPU block: conv -> BatchNorm (eval: running statistics; train: batch statistics) -> LeakyReLU(0.1)."""
    w = blk.conv.weight.detach().double().requires_grad_(train)
    xd = x.double().requires_grad_(train)
    s, p = blk.conv.stride[0], blk.conv.padding[0]
    if blk.batch_norm_act:
        bn = blk.batch_norm
        z = F.conv2d(xd, w, None, s, p)
        if train:
            u = F.batch_norm(z, None, None, bn.weight.detach().double(), bn.bias.detach().double(), True, 0.0, bn.eps)
        else:
            u = F.batch_norm(z, bn.running_mean.double(), bn.running_var.double(), bn.weight.detach().double(),
                             bn.bias.detach().double(), False, 0.0, bn.eps)
        y = F.leaky_relu(u, 0.1)
    else:
        y = F.conv2d(xd, w, blk.conv.bias.detach().double(), s, p)
    return y, xd, w


def _rel_max(got, want):
    return float((got.double() - want).abs().max() / max(float(want.abs().max()), 1e-12))


def _rel_l2(got, want):
    return float((got.double() - want).norm() / max(float(want.norm()), 1e-30))


def run():
    import yolo_for_turbines_amd as yt
    from yolo_for_turbines_amd import engine
    worst = {}

    def note(key, ratio):
        worst[key] = max(worst.get(key, 0.0), ratio)

    for ci, c in enumerate(CASES):
        name, _, _, _, cin, _, k, s, bn = c
        for dt in ("fp32", "bf16", "fp16"):
            if dt != "fp32" and cin % 32 and cin != 3:
                continue
            blk, x = _make(yt, c, 900 + ci)
            ref, _, _ = _ref(blk, x, False)
            ref_t, xd, wd = _ref(blk, x, True) if bn else (None, None, None)
            blk = blk.cuda().eval()
            st = engine.module_state(blk)
            st.compute_dtype = dt
            tiles = [None] + ([1, 2, 3, 4, 5, 6, 7] if dt == "fp32" else [])
            for tile in tiles:
                if tile is not None and (cin == 3 and tile >= 5 or tile >= 5 and (s != 1 or cin % 32)):
                    continue
                st.tile_override = tile
                with torch.no_grad():
                    y = blk(x.cuda()).cpu()
                assert tuple(y.shape) == tuple(ref.shape), (name, tuple(y.shape), tuple(ref.shape))
                note(f"{name}/{dt}/eval" + (f"/tile{tile}" if tile else ""), _rel_max(y, ref) / FWD_BAR[dt])
            st.tile_override = None
            if not bn:
                st.compute_dtype = None
                continue
            # train mode: batch statistics forward, dx and dW for a fixed upstream gradient
            blk.train()
            gy = torch.randn(ref_t.shape, generator=torch.Generator().manual_seed(950 + ci))
            ref_t.backward(gy.double())
            xg = x.cuda().requires_grad_(True)
            y = blk(xg)
            y.backward(gy.cuda())
            st.compute_dtype = None
            note(f"{name}/{dt}/train_y", _rel_max(y.detach().cpu(), ref_t.detach()) / FWD_BAR[dt])
            for what, got, want in (("dx", xg.grad.cpu(), xd.grad), ("dw", blk.conv.weight.grad.cpu(), wd.grad)):
                err = _rel_max(got, want) if dt == "fp32" else _rel_l2(got, want)
                note(f"{name}/{dt}/{what}", err / GRAD_BAR[dt])
            blk.conv.weight.grad = None
    return worst


if __name__ == "__main__":
    print(json.dumps(run()))
