"""numpy restatement of the anchor clustering contract of include/yolo_mi355x.h (IoU k-means++ with restarts, Lloyd steps, fitness,
the anchor layout), written from that statement: fp32 IoU with one rounding per operation, fp64 sums. It is the reference of
tests/test_gpu_anchors.py and the host-side yardstick of tools/anchors_bench.py.

The contract leaves the association of the fp64 sums to the implementation, so this file offers several (``ORDERS``) and reports how
far every seeding draw lay from the nearest running-sum boundary: a test compares bits only where the orders agree with each other
and the draws are clear of the boundaries."""
import math

import numpy as np

F32 = np.float32
ORDERS = ("pairwise", "fsum", "sequential")


def make_boxes(n, seed):
    """n (w, h) rows around nine log-uniform modes in 0.02 .. 0.95, each multiplied by exp(N(0, 0.25)), clipped to [1e-3, 1], fp32."""
    rng = np.random.default_rng(seed)
    modes = np.exp(rng.uniform(np.log(0.02), np.log(0.95), size=(9, 2)))
    which = rng.integers(0, 9, size=n)
    wh = modes[which] * np.exp(rng.normal(0.0, 0.25, size=(n, 2)))
    return np.clip(wh, 1e-3, 1.0).astype(F32)


def iou(bw, bh, cw, ch):
    """inter / (bw bh + cw ch - inter) in fp32 (numpy rounds every fp32 operation once); broadcasts."""
    bw, bh, cw, ch = (np.asarray(v, dtype=F32) for v in (bw, bh, cw, ch))
    inter = np.minimum(bw, cw) * np.minimum(bh, ch)
    return inter / (bw * bh + cw * ch - inter)


def iou_matrix(wh, c):
    """(n, k) fp32."""
    wh, c = np.asarray(wh, dtype=F32), np.asarray(c, dtype=F32).reshape(-1, 2)
    return iou(wh[:, None, 0], wh[:, None, 1], c[None, :, 0], c[None, :, 1])


def _draw_index(u, n):
    return min(int(float(u) * n), n - 1)


def seed_picks(wh, u):
    """k-means++ seeds of one restart: (picks [k], margin). margin = the smallest |running sum - u[j] T| / T over the draws that were
    resolved by a running sum (inf if none was)."""
    wh = np.asarray(wh, dtype=F32)
    n, k = len(wh), len(u)
    picks, margin, best = [_draw_index(u[0], n)], math.inf, None
    for j in range(1, k):
        s = wh[picks[-1]]
        v = iou(wh[:, 0], wh[:, 1], s[0], s[1])
        best = v if best is None else np.maximum(best, v)
        d = (F32(1.0) - best).astype(np.float64)
        cs = np.cumsum(d * d)
        T = float(cs[-1])
        if T == 0.0:
            picks.append(_draw_index(u[j], n))
            continue
        t = float(u[j]) * T
        picks.append(min(int(np.searchsorted(cs, t, side="right")), n - 1))
        margin = min(margin, float(np.min(np.abs(cs - t))) / T)
    return np.array(picks, dtype=np.int32), margin


def _sum64(v, order):
    v = np.ascontiguousarray(v, dtype=np.float64)
    if order == "pairwise":
        return float(v.sum())                      # numpy's pairwise blocks on a contiguous vector
    if order == "fsum":
        return math.fsum(v)                        # exactly rounded
    if order == "sequential":
        return float(np.cumsum(v)[-1])
    raise ValueError(order)


def lloyd(wh, centroids, max_iter, order="pairwise"):
    """(final centroids (k, 2) fp32, iterations, converged)."""
    wh = np.asarray(wh, dtype=F32)
    c = np.array(centroids, dtype=F32).reshape(-1, 2)
    for step in range(1, max_iter + 1):
        lab = np.argmax(iou_matrix(wh, c), axis=1)               # the first maximum
        new = c.copy()
        for j in range(len(c)):
            sel = wh[lab == j]
            if len(sel):
                cnt = float(len(sel))
                new[j, 0] = F32(_sum64(sel[:, 0], order) / cnt)
                new[j, 1] = F32(_sum64(sel[:, 1], order) / cnt)
        same = np.array_equal(new.view(np.uint32), c.view(np.uint32))
        c = new
        if same:
            return c, step, 1
    return c, max_iter, 0


def fitness(wh, c):
    """Mean over the boxes of the best IoU, fp64."""
    return math.fsum(iou_matrix(wh, c).max(axis=1).astype(np.float64)) / len(wh)


def layout(centroids):
    """Ascending by fp32 area (stable); k % 3 == 0: (3, k / 3, 2) with the group of the largest anchors first, else (k, 2)."""
    c = np.asarray(centroids, dtype=F32).reshape(-1, 2)
    s = c[np.argsort(c[:, 0] * c[:, 1], kind="stable")]
    return s.reshape(3, len(c) // 3, 2)[::-1].copy() if len(c) % 3 == 0 else s


def kmeans(wh, draws, max_iter=300, order="pairwise"):
    """All restarts: dict(picks (R, k), seeds / centroids (R, k, 2), fitness (R,), iterations, converged, best, anchors, margin)."""
    wh = np.asarray(wh, dtype=F32)
    draws = np.asarray(draws, dtype=np.float64)
    R, k = draws.shape
    out = dict(picks=np.zeros((R, k), np.int32), seeds=np.zeros((R, k, 2), F32), centroids=np.zeros((R, k, 2), F32),
               fitness=np.zeros(R, np.float64), iterations=np.zeros(R, np.int32), converged=np.zeros(R, np.int32), margin=math.inf)
    for r in range(R):
        picks, margin = seed_picks(wh, draws[r])
        out["picks"][r], out["margin"] = picks, min(out["margin"], margin)
        out["seeds"][r] = wh[picks]
        c, it, conv = lloyd(wh, wh[picks], max_iter, order)
        out["centroids"][r], out["iterations"][r], out["converged"][r] = c, it, conv
        out["fitness"][r] = fitness(wh, c)
    out["best"] = max(range(R), key=lambda r: (out["fitness"][r], -r))           # highest fitness, ties to the lowest index
    out["anchors"] = layout(out["centroids"][out["best"]])
    return out


def anchor_fitness(wh, anchors, iou_threshold=0.5):
    """dict(mean_iou, recall, counts (k,), labels (n,)) of any anchors."""
    m = iou_matrix(wh, anchors)
    lab = np.argmax(m, axis=1).astype(np.int32)
    best = m.max(axis=1)
    return dict(mean_iou=math.fsum(best.astype(np.float64)) / len(best), recall=float(np.count_nonzero(best > F32(iou_threshold))) / len(best),
                counts=np.bincount(lab, minlength=m.shape[1]).astype(np.int32), labels=lab)
