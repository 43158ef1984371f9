"""Generate ``tests/golden/mosaic_boxes.npz`` by IMPORTING THE REFERENCE's ``mosaic_augmentation`` (build container only).

Run from the repo root:  ``python tests/gen_golden_augment.py``

``albumentations`` / ``cv2`` are absent here: ``cv2`` and ``albumentations.pytorch`` are ``MagicMock``s, and ``A`` is a
minimal stand-in whose ``Compose`` / ``LongestMaxSize`` / ``PadIfNeeded`` apply the letterbox rules to the boxes
(yolo -> (x_min, y_min, x_max, y_max) + clip, drop zero-area boxes, pixel mapping of the pad, back to yolo) and return an
image of the right shape (zeros; the fixture pins BOX arithmetic only). ``random`` is seeded per case and the 20 cutout
draws are recorded by replaying the same seed. The fixture holds inputs and the reference's output boxes only.
"""
from __future__ import annotations

import os
import random
import sys
from unittest.mock import MagicMock

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import augment_ref as ar  # noqa: E402


class _Compose:
    def __init__(self, transforms, bbox_params=None):
        self.transforms = transforms

    def __call__(self, image, bboxes):
        out = []
        for bx in np.asarray(bboxes, np.float64).reshape(-1, 5) if len(bboxes) else []:
            out.append([*ar.yolo_to_albu(*[float(v) for v in bx[:4]]), float(bx[4])])
        for t in self.transforms:
            image, out = t(image, out)
        return {"image": image, "bboxes": [((b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0, b[2] - b[0], b[3] - b[1], b[4]) for b in out]}


class _LongestMaxSize:
    def __init__(self, max_size):
        self.size = max_size

    def __call__(self, image, boxes):
        h, w = ar.resized_hw(image.shape[0], image.shape[1], self.size)
        return np.zeros((h, w, 3), np.uint8), [b for b in boxes if ar.area_nz(b, h, w)]


class _PadIfNeeded:
    def __init__(self, min_height, min_width, border_mode=None, value=0):
        self.H, self.W = min_height, min_width

    def __call__(self, image, boxes):
        h, w = image.shape[:2]
        H, W = max(self.H, h), max(self.W, w)
        top, left = (H - h) // 2, (W - w) // 2
        out = []
        for b in boxes:
            if not ar.area_nz(b[:4], h, w):
                continue
            nb = [(b[0] * w + left) / W, (b[1] * h + top) / H, (b[2] * w + left) / W, (b[3] * h + top) / H]
            if ar.area_nz(nb, H, W):
                out.append(nb + [b[4]])
        return np.zeros((H, W, 3), np.uint8), out


A = MagicMock()                      # config.py builds its other transforms at import time
A.Compose, A.LongestMaxSize, A.PadIfNeeded, A.BboxParams = _Compose, _LongestMaxSize, _PadIfNeeded, MagicMock()
sys.modules["albumentations"] = A
sys.modules["albumentations.pytorch"] = MagicMock()
sys.modules["cv2"] = MagicMock()
sys.path.insert(0, "/root/reference/code")
import utils as ref_utils  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, "tests", "golden", "mosaic_boxes.npz")


def _boxes(rng, n, far=False):
    b = []
    for _ in range(n):
        w, h = rng.uniform(0.04, 0.3), rng.uniform(0.04, 0.3)
        lo = 0.0 if not far else 0.85
        cx, cy = rng.uniform(lo, 1.0), rng.uniform(lo, 1.0)
        b.append([cx, cy, w, h, float(rng.integers(0, 3))])
    return b


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    shapes = [(480, 640), (375, 500), (416, 416), (640, 480), (300, 400)]
    for seed in range(40):
        S = 416 if seed % 3 else 320
        hw = shapes[seed % len(shapes)]
        # a few boxes per image; every 4th case holds only boxes near the far corner of quadrant 3, so early attempts miss
        far = seed % 4 == 3
        quads = [[] if far and q < 3 else _boxes(rng, int(rng.integers(0 if seed % 5 == 0 else 1, 4)), far) for q in range(4)]
        if sum(len(q) for q in quads) == 0:
            quads[3] = _boxes(rng, 1)
        out.append((seed, S, hw, quads))
    return out


def main():
    recs = {"S": [], "hw": [], "draws": [], "n_in": [], "boxes_in": [], "n_out": [], "boxes_out": []}
    for seed, S, hw, quads in cases():
        random.seed(seed)
        draws = [random.uniform(0.2, 0.3) for _ in range(20)]
        random.seed(seed)
        imgs = [np.zeros((hw[0], hw[1], 3), np.uint8) for _ in range(4)]
        res, boxes = ref_utils.mosaic_augmentation(imgs, [list(map(list, q)) for q in quads], S)
        boxes = np.zeros((0, 5)) if isinstance(res, int) else np.asarray(boxes, np.float64).reshape(-1, 5)
        recs["S"].append(S); recs["hw"].append(hw); recs["draws"].append(draws)
        recs["n_in"].append([len(q) for q in quads])
        recs["boxes_in"].append(np.concatenate([np.asarray(q, np.float64).reshape(-1, 5) for q in quads]))
        recs["n_out"].append(len(boxes)); recs["boxes_out"].append(boxes)
    np.savez_compressed(OUT, S=np.array(recs["S"]), hw=np.array(recs["hw"]), draws=np.array(recs["draws"]),
                        n_in=np.array(recs["n_in"]), boxes_in=np.concatenate(recs["boxes_in"]), n_out=np.array(recs["n_out"]),
                        boxes_out=np.concatenate(recs["boxes_out"]))
    print("wrote", OUT, "cases", len(recs["S"]), "boxes out", sum(recs["n_out"]))


if __name__ == "__main__":
    main()
