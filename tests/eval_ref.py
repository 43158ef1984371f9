"""Sequential restatement of detection evaluation at several IoU thresholds, for tests/test_eval_host.py and tests/test_gpu_eval.py.

Per threshold it runs the walk of ``oracle.metrics.calc_map``: per class, detections in objectness-descending stable order; each
looks at the ground truths of its image and class in list order, takes the first maximum IoU under a strict ``>`` against a running
best that starts at 0, and is a true positive iff that IoU > threshold and the ground truth is still unassigned. The IoUs come from
``oracle.postprocess.calc_iou`` on the ground-truth block of the image (elementwise fp32, so one call per (class, image) gives the
bits of one call per pair; the block does not depend on the threshold, so it is evaluated once and every threshold walks it again
with its own ``taken`` state). Thresholds are compared in fp32. AP is ``torch.trapz`` of the fp32 cumulative precision / recall with
(0, 1) in front, as in the oracle. Nothing here knows the closed form the device uses.

Also here: the case builders of the GPU tests and the precondition that makes an exact comparison of flags fair."""
import numpy as np
import torch

from oracle.postprocess import calc_iou

F32 = np.float32
DEFAULT_THRESHOLDS = [0.5 + 0.05 * i for i in range(10)]
MARGIN = 1e-6


def _rows(boxes):
    a = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    return a.astype(F32)                                              # what the device is given


def evaluate(pred_boxes, true_boxes, num_classes, iou_thresholds=None, conf_threshold=0.5, box_format="center"):
    """-> dict: ``order`` (D,) rows of pred_boxes in (class ascending, objectness descending, stable) order after rows with a class
    outside range(num_classes) are dropped; ``flags`` (T, D) bool; ``best_iou`` (D,) fp32; ``best_gt`` (D,) rows of true_boxes or
    -1; ``second`` (D,) fp32, the largest IoU among the ground truths of the block that are not bitwise equal to the best one (0
    without one); ``ap`` (T, nc) fp32, NaN without ground truth; ``map`` (T,) fp32; ``n_gt`` / ``n_det`` / ``n_det_at_conf`` (nc,)
    and ``tp_at_conf`` (T, nc) int64. Raises ZeroDivisionError when no class has ground truth."""
    thr = DEFAULT_THRESHOLDS if iou_thresholds is None else list(iou_thresholds)
    thr32 = [F32(t) for t in thr]
    T, nc = len(thr), int(num_classes)
    P, G = _rows(pred_boxes), _rows(true_boxes)
    conf = F32(conf_threshold)
    order, flags, best_iou, best_gt, second = [], [[] for _ in range(T)], [], [], []
    ap = np.full((T, nc), np.nan, F32)
    n_gt, n_det, n_conf = (np.zeros(nc, np.int64) for _ in range(3))
    tp_conf = np.zeros((T, nc), np.int64)
    for c in range(nc):
        di = [i for i in range(len(P)) if P[i, 6] == c]
        gi = [j for j in range(len(G)) if G[j, 6] == c]
        di.sort(key=lambda i: float(P[i, 5]), reverse=True)           # list.sort is stable, also with reverse=True
        n_gt[c], n_det[c] = len(gi), len(di)
        per_img = {}
        for j in gi:
            per_img.setdefault(float(G[j, 0]), []).append(j)
        # the IoU block of every image: detections of the image (rows) x its ground truths in list order (columns)
        by_img = {}
        for k, i in enumerate(di):
            by_img.setdefault(float(P[i, 0]), []).append(k)
        b_iou, b_gt, b_second = np.zeros(len(di), F32), np.full(len(di), -1, np.int64), np.zeros(len(di), F32)
        for img, ks in by_img.items():
            cand = per_img.get(img, [])
            if not cand:
                continue
            block = calc_iou(torch.from_numpy(P[[di[k] for k in ks], 1:5])[:, None, :], torch.from_numpy(G[cand, 1:5])[None, :, :],
                             box_format).numpy()
            for row, k in zip(block, ks):
                best, best_j = F32(0), -1
                for j, v in enumerate(row):                           # `if iou > best: best, best_j = iou, j`
                    if v > best:
                        best, best_j = v, j
                if best_j >= 0:
                    b_iou[k], b_gt[k] = best, cand[best_j]
                    same = G[cand[best_j]].tobytes()
                    others = [v for j, v in enumerate(row) if G[cand[j]].tobytes() != same]
                    b_second[k] = max(others, default=F32(0))
        above = np.array([P[i, 5] > conf for i in di], bool)
        n_conf[c] = int(above.sum())
        for t in range(T):
            taken = set()
            tp = np.zeros(len(di), bool)
            for k in range(len(di)):                                  # the walk: sequential, one `taken` set per threshold
                if b_gt[k] >= 0 and b_iou[k] > thr32[t] and b_gt[k] not in taken:
                    tp[k] = True
                    taken.add(b_gt[k])
            flags[t].append(tp)
            tp_conf[t, c] = int((tp & above).sum())
            if gi:
                tpf = torch.from_numpy(tp.astype(F32))
                ctp, cfp = torch.cumsum(tpf, 0), torch.cumsum(1 - tpf, 0)
                prec = torch.cat((torch.tensor([1.0]), ctp / (ctp + cfp)))
                rec = torch.cat((torch.tensor([0.0]), ctp / len(gi)))
                ap[t, c] = float(torch.trapz(prec, rec))
        order += di
        best_iou.append(b_iou)
        best_gt.append(b_gt)
        second.append(b_second)
    has = n_gt > 0
    if not has.any():
        raise ZeroDivisionError("division by zero")
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    aps = [[torch.tensor(ap[t, c]) for c in range(nc) if has[c]] for t in range(T)]
    return dict(order=np.array(order, np.int64), flags=np.stack([cat(f, bool) for f in flags]), best_iou=cat(best_iou, F32),
                best_gt=cat(best_gt, np.int64), second=cat(second, F32), ap=ap,
                map=np.array([float(sum(a) / len(a)) for a in aps], F32), n_gt=n_gt, n_det=n_det, n_det_at_conf=n_conf,
                tp_at_conf=tp_conf, thresholds=thr)


def margins(ref):
    """(distance of the positive best IoUs from the nearest threshold, their lead over the second-best IoU of a ground truth that is
    not a bitwise copy of the best one); inf where there is nothing to compare."""
    b = ref["best_iou"].astype(np.float64)
    pos = b > 0
    if not pos.any():
        return np.inf, np.inf
    thr = np.array([float(F32(t)) for t in ref["thresholds"]])
    to_thr = np.abs(b[pos][:, None] - thr[None, :]).min()
    lead = (b[pos] - ref["second"].astype(np.float64)[pos]).min()
    return float(to_thr), float(lead)


def check_precondition(ref):
    """Exact comparison of flags is claimed only where no rounding of an IoU can decide one: asserted on the restatement itself."""
    to_thr, lead = margins(ref)
    assert to_thr >= MARGIN, f"a best IoU lies {to_thr:.1e} from a threshold: choose other seeds"
    assert lead >= MARGIN, f"a best IoU leads the second-best by {lead:.1e}: choose other seeds"
    return to_thr, lead


# ---------------------------------------------------------------------------------------------------- case builders
HANDOVER = dict(
    preds=[[0, .58, .5, .4, .4, .9, 0], [0, .5, .5, .37, .4, .8, 0]],        # IoU 0.66666 and 0.92499 with the one ground truth
    trues=[[0, .5, .5, .4, .4, 1.0, 0]],
    flags={0.50: [1, 0], 0.55: [1, 0], 0.60: [1, 0], 0.65: [1, 0], 0.70: [0, 1], 0.75: [0, 1], 0.80: [0, 1], 0.85: [0, 1],
           0.90: [0, 1], 0.95: [0, 0]},
    ap={0.50: 1.0, 0.65: 1.0, 0.70: 0.25, 0.90: 0.25, 0.95: 0.0},
    map_50_95=0.525)


def _f(v):
    return float(F32(v))


def _jitter(rng, box, s):
    cx, cy, w, h = box
    return [_f(cx + s * w * rng.standard_normal()), _f(cy + s * h * rng.standard_normal()), _f(w * np.exp(s * rng.standard_normal())),
            _f(h * np.exp(s * rng.standard_normal()))]


def crowd_case(n_gt, dup_after, seed, nc=2):
    """``n_gt`` ground truths in one (image 0, class 0) block; the best ground truth of the first detection sits at row ``lead`` and
    a bitwise copy of it ``dup_after`` rows later (when that fits), so the first must win whatever the width a block is walked in.
    Detections: jittered copies of a few ground truths, the copied one first. -> (preds, trues, lead, lead + dup_after or None)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    trues = []
    for _ in range(n_gt):
        trues.append([0, _f(rng.uniform(0.1, 0.9)), _f(rng.uniform(0.1, 0.9)), _f(rng.uniform(0.03, 0.12)), _f(rng.uniform(0.03, 0.12)), 1.0, 0])
    lead = 0 if n_gt <= dup_after else min(3, n_gt - dup_after - 1)
    dup = lead + dup_after if lead + dup_after < n_gt else None
    if dup is not None:
        trues[dup] = list(trues[lead])
    trues.append([1, 0.5, 0.5, 0.2, 0.2, 1.0, 1])                                 # another image and class next to the block
    preds = [[0, *_jitter(rng, trues[lead][1:5], 0.03), 0.95, 0]]
    for j in rng.choice(n_gt, size=min(n_gt, 12), replace=False):
        preds.append([0, *_jitter(rng, trues[int(j)][1:5], 0.05), _f(rng.uniform(0.2, 0.9)), 0])
    preds.append([1, 0.5, 0.5, 0.21, 0.2, 0.7, 1])
    return preds, trues, lead, dup


def many_dets_case(n_det, seed, nc=2, images=5):
    """``n_det`` detections in class 0 (the scan's 256-row rounds and their carry) over a few images, every ground truth with
    several jittered copies, some of them better than an earlier, higher-scored one (owners change between thresholds)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    trues, preds = [], []
    for img in range(images):
        for _ in range(6):
            trues.append([img, _f(rng.uniform(0.15, 0.85)), _f(rng.uniform(0.15, 0.85)), _f(rng.uniform(0.06, 0.2)), _f(rng.uniform(0.06, 0.2)), 1.0, 0])
    trues.append([0, 0.3, 0.3, 0.1, 0.1, 1.0, 1])
    preds.append([0, 0.3, 0.3, 0.11, 0.1, 0.6, 1])
    while len(preds) < n_det + 1:
        g = trues[int(rng.integers(0, len(trues) - 1))]
        preds.append([g[0], *_jitter(rng, g[1:5], float(rng.choice([0.02, 0.06, 0.15]))), _f(rng.uniform(0.05, 0.99)), 0])
    return preds, trues


def seeded_case(images, nc, gt_mean, det_mean, seed):
    """A validation set: per image ~gt_mean ground truths and ~det_mean detections (jittered copies and noise), classes uniform."""
    rng = np.random.Generator(np.random.PCG64(seed))
    trues, preds = [], []
    for img in range(images):
        mine = []
        for _ in range(max(1, rng.poisson(gt_mean))):
            g = [img, _f(rng.uniform(0.1, 0.9)), _f(rng.uniform(0.1, 0.9)), _f(rng.uniform(0.04, 0.3)), _f(rng.uniform(0.04, 0.3)), 1.0,
                 int(rng.integers(0, nc))]
            mine.append(g)
        trues += mine
        for _ in range(max(1, rng.poisson(det_mean))):
            if rng.random() < 0.75:
                g = mine[int(rng.integers(0, len(mine)))]
                preds.append([img, *_jitter(rng, g[1:5], float(rng.choice([0.02, 0.07, 0.2]))), _f(rng.uniform(0.05, 0.99)), g[6]])
            else:
                preds.append([img, _f(rng.uniform(0.1, 0.9)), _f(rng.uniform(0.1, 0.9)), _f(rng.uniform(0.04, 0.3)), _f(rng.uniform(0.04, 0.3)),
                              _f(rng.uniform(0.05, 0.6)), int(rng.integers(0, nc))])
    return preds, trues
