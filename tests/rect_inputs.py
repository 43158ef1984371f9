"""Seeded inputs of the rectangular (H != W) fixtures: shared by ``tests/gen_golden_rect.py`` (which runs the imported
reference on them) and ``tests/test_gpu_rect.py`` / ``tests/test_rect_host.py`` (which regenerate them).  No reference
code here: weights come from ``oracle.net.synth_state_dict``, images and targets from the generators below."""
from __future__ import annotations

import numpy as np
import torch

from tests import golden_inputs as gi

F32 = np.float32

# eval forward cases of net_rect.npz: (H, W) with H != W, each side a multiple of 32
RECT_NET_CASES = {
    "nc80_96x160_b2_leaky": dict(nc=80, H=96, W=160, batch=2, wseed=701, xseed=702, act="leaky_relu"),
    "nc2_160x96_b2_mish": dict(nc=2, H=160, W=96, batch=2, wseed=703, xseed=704, act="mish"),
    "nc2_224x96_b1_leaky": dict(nc=2, H=224, W=96, batch=1, wseed=705, xseed=706, act="leaky_relu"),
}
# one fine-tune step (gen_golden.gen_train's sequence) at 96 x 160
RECT_TRAIN_CASE = dict(nc=2, H=96, W=160, batch=2, wseed=711, xseed=712, tseed=713, anchors=gi.TRAIN_CASE["anchors"])
STRIDES = (32, 16, 8)


def rect_input(seed, batch, H, W, in_channels=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.random((batch, in_channels, H, W), dtype=np.float32))


def rect_scaled_anchors(anchors, H, W):
    """anchors[k] * (L / stride_k), L = max(H, W): the convention of INTEGRATION.md (restated, not imported)."""
    L = max(H, W)
    return torch.tensor(anchors, dtype=torch.float32) * torch.tensor([L // s for s in STRIDES]).view(3, 1, 1)


def rect_targets(batch, H, W, nc, anchors, seed, mean_boxes=7):
    """The target rule of dataset.py:119-161 restated per axis for an H x W canvas: boxes (x, y, w, h) normalised to the
    canvas, anchors (normalised to L = max(H, W)) ranked by IoU of (w W/L, h H/L); per scale i = int(gh y), j = int(gw x),
    row [gw x - j, gh y - i, w gw, h gh, 1, class]; the other free anchors of the scale with IoU > 0.5 are ignored (-1).
    Returns (three (B,3,gh,gw,6) float32 arrays, the boxes as (B, max_boxes, 5) float32, counts (B,) int32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = max(H, W)
    gh = [H // s for s in STRIDES]
    gw = [W // s for s in STRIDES]
    anc = np.asarray(anchors, np.float32).reshape(9, 2)
    out = [np.zeros((batch, 3, gh[s], gw[s], 6), F32) for s in range(3)]
    boxes = []
    for b in range(batch):
        n = max(1, rng.poisson(mean_boxes))
        bl = []
        for _ in range(n):
            a = rng.integers(0, 9)
            w, h = np.clip(anc[a].astype(np.float64) * np.exp(0.25 * rng.standard_normal(2)) * (L / W, L / H), 0.01, 0.99)
            x, y = rng.uniform(0.02, 0.98, 2)
            bl.append([x, y, w, h, float(rng.integers(0, nc))])
        boxes.append(np.asarray(bl, F32))
    for b, bl in enumerate(boxes):
        for x, y, w, h, c in bl:
            wl, hl = np.float32(w) * np.float32(W / L), np.float32(h) * np.float32(H / L)
            inter = np.minimum(anc[:, 0], wl) * np.minimum(anc[:, 1], hl)
            iou = inter / (wl * hl + anc[:, 0] * anc[:, 1] - inter)
            has = [False, False, False]
            for ai in np.argsort(-iou, kind="stable"):
                s, k = divmod(int(ai), 3)
                gx, gy = gw[s] * float(x), gh[s] * float(y)
                i, j = int(gy), int(gx)
                taken = out[s][b, k, i, j, 0]      # dataset.py:141 tests element 0 (x), not obj
                if not taken and not has[s]:
                    out[s][b, k, i, j] = [gx - j, gy - i, float(w) * gw[s], float(h) * gh[s], 1.0, c]
                    has[s] = True
                elif not taken and iou[ai] > 0.5:
                    out[s][b, k, i, j, 4] = -1.0
    mb = max(len(bl) for bl in boxes)
    padded = np.zeros((batch, mb, 5), F32)
    for b, bl in enumerate(boxes):
        padded[b, :len(bl)] = bl
    return out, padded, np.array([len(bl) for bl in boxes], np.int32)
