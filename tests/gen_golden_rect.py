"""Generate ``tests/golden/net_rect.npz`` by IMPORTING THE REFERENCE on rectangular (H != W) inputs (build container only).

Run from the repo root:  ``python tests/gen_golden_rect.py``

Same recipe as ``tests/gen_golden.py`` (whose import sets up the stand-ins and puts the reference on ``sys.path``): the
fixture holds output numbers of the reference's shape-generic forward (its head reshape reads ``x.shape[2], x.shape[3]``)
and of one fine-tune step, plus the targets that step was given; images and weights are regenerated from seeds by
``tests/rect_inputs.py`` / ``oracle.net.synth_state_dict``.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import gen_golden as gg          # noqa: E402  (imports the reference)
from tests import golden_inputs as gi       # noqa: E402
from tests import rect_inputs as ri         # noqa: E402
from oracle import net as onet              # noqa: E402


SAMPLE = 3


def gen_eval(out):
    for name, c in ri.RECT_NET_CASES.items():
        sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
        m = gg.ref_net(c["nc"], c["act"], sd).eval()
        x = ri.rect_input(c["xseed"], c["batch"], c["H"], c["W"])
        with torch.no_grad():
            preds = m(x)
        for i, p in enumerate(preds):
            if p.numel() > 100000:           # the 80-class 12 x 20 head: every 3rd element (3 and 85 are coprime), keeps the file < 1 MB
                out[f"{name}/p{i}_every{SAMPLE}"] = p.contiguous().reshape(-1)[::SAMPLE].numpy().copy()
            else:
                out[f"{name}/p{i}"] = p.contiguous().numpy()
            print(name, i, tuple(p.shape), float(p.abs().max()))


def gen_train(out):
    c = ri.RECT_TRAIN_CASE
    tg_np, boxes, counts = ri.rect_targets(c["batch"], c["H"], c["W"], c["nc"], c["anchors"], c["tseed"])
    for i, t in enumerate(tg_np):
        out[f"train/target{i}"] = t
    out["train/boxes"], out["train/counts"] = boxes, counts
    sa = ri.rect_scaled_anchors(c["anchors"], c["H"], c["W"])
    # mish_b4: the same step at batch 4 for the 16-bit test (the square 16-bit bars were set at batch 4: at batch 2 the deepest
    # BatchNorm layers see 30 values per channel and bf16 rounding alone moves layer 0's bias gradient to cos ~0.95)
    tg4, boxes4, counts4 = ri.rect_targets(4, c["H"], c["W"], c["nc"], c["anchors"], c["tseed"] + 1)
    for i, t in enumerate(tg4):
        out[f"train_b4/target{i}"] = t
    for tag, act, B, tgs in (("leaky", "leaky_relu", c["batch"], tg_np), ("mish", "mish", c["batch"], tg_np), ("mish_b4", "mish", 4, tg4)):
        tg_np_ = tgs
        sd = onet.synth_state_dict(c["wseed"], 3, c["nc"], gain=gi.NET_GAIN)
        m = gg.ref_net(c["nc"], act, sd).train()
        x = ri.rect_input(c["xseed"], B, c["H"], c["W"])
        lf = gg.ref_loss.YOLOLoss()
        opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
        opt.zero_grad()
        preds = m(x)
        out[f"{tag}/pred_sums"] = np.stack([gg.sums(p.detach()) for p in preds])
        parts = torch.stack([torch.stack(lf(preds[i], torch.from_numpy(tg_np_[i]).clone(), sa[i])) for i in range(3)])
        parts.sum().backward()
        out[f"{tag}/loss_parts"] = parts.detach().numpy()
        g = {k: p.grad for k, p in m.named_parameters()}
        for k in gg.TRAIN_GRAD_KEYS:
            out[f"{tag}/grad/{k}"] = g[k].reshape(-1)[::gi.TRAIN_GRAD_STRIDE].numpy().copy() if g[k].numel() > 4096 else g[k].numpy().copy()
        out[f"{tag}/gradnorm_all"] = np.array([float(p.grad.double().norm()) for p in m.parameters()])
        out[f"{tag}/rm0"] = m.state_dict()["layers.0.batch_norm.running_mean"].numpy().copy()
        out[f"{tag}/rv0"] = m.state_dict()["layers.0.batch_norm.running_var"].numpy().copy()
        opt.step()
        out[f"{tag}/w0_after_sgd"] = m.state_dict()["layers.0.conv.weight"].numpy().copy()
        print("train", tag, parts.detach().numpy().round(4).tolist())


if __name__ == "__main__":
    res = {}
    gen_eval(res)
    gen_train(res)
    path = os.path.join(gg.OUT, "net_rect.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
