"""numpy restatement of weighted box fusion and of the test-time-augmentation views, written from the contract in
include/yolo_mi355x.h, step by step in ``dtype`` (np.float32: the kernel's bits; np.float64: the yardstick of the
fp32 walk). numpy's elementwise fp32 operations round once, like the kernels built without FMA contraction."""
import numpy as np


def _corners(rows, center, dtype):
    x, y, w, h = (rows[:, k].astype(dtype) for k in range(4))
    if center:
        x = x - w / dtype(2)
        y = y - h / dtype(2)
    return x, y, x + w, y + h, w * h


def fuse_ref(boxes, iou_threshold=0.55, obj_threshold=0.0, box_format="center", n_views=0, conf_type="avg", class_agnostic=False,
             dtype=np.float32, margins=None):
    """One image. boxes: (N, 6) float32 rows [x, y, w, h, obj, cls]. Returns (fused (N, 6) dtype, members (N,) int32, count,
    assign (N,) int32). ``margins``: a list that receives |iou - threshold| of every IoU the walk compared."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    N = boxes.shape[0]
    center = box_format == "center"
    thr = dtype(np.float32(iou_threshold))                       # the threshold is compared as (float) iou_threshold
    eps = dtype(np.float32(1e-6))
    # 1. candidates, in the order of the NMS: score descending (-0 = +0), ties by ascending row
    cand = [i for i in range(N) if float(boxes[i, 4]) > float(obj_threshold)]
    cand.sort(key=lambda i: (-(float(boxes[i, 4]) + 0.0), i))
    n = len(cand)
    rows = boxes[cand] if n else np.zeros((0, 6), np.float32)
    # 2. corners
    X1, Y1, X2, Y2, AREA = _corners(rows, center, dtype)
    SC, CLS = rows[:, 4].astype(dtype), rows[:, 5]
    # 3. the walk
    F = np.zeros((n, 4), dtype)
    A = np.zeros((n, 4), dtype)
    S = np.zeros(n, dtype)
    cnt = np.zeros(n, np.int64)
    ccls = np.zeros(n, np.float32)
    founder = np.zeros(n, np.int64)
    fscore = np.zeros(n, dtype)
    joined = np.zeros(n, np.int64)
    K = 0
    for g in range(n):
        c = np.array([X1[g], Y1[g], X2[g], Y2[g]], dtype)
        s = SC[g]
        k = -1
        if K:
            f = F[:K]
            # 4. IoU against the fused corners
            xa, ya = np.maximum(c[0], f[:, 0]), np.maximum(c[1], f[:, 1])
            xb, yb = np.minimum(c[2], f[:, 2]), np.minimum(c[3], f[:, 3])
            inter = np.maximum(xb - xa, dtype(0)) * np.maximum(yb - ya, dtype(0))
            ak = (f[:, 2] - f[:, 0]) * (f[:, 3] - f[:, 1])
            with np.errstate(all="ignore"):
                iou = inter / (((AREA[g] + ak) - inter) + eps)
            # 5. eligibility and choice: largest IoU above the threshold, ties to the earliest cluster (argmax: first maximum)
            elig = np.ones(K, bool) if class_agnostic else (ccls[:K] == CLS[g])
            if margins is not None:
                margins.extend(np.abs(iou[elig].astype(np.float64) - float(thr)).tolist())
            ok = elig & (iou > thr)
            if ok.any():
                k = int(np.argmax(np.where(ok, iou, dtype(-np.inf))))
        # 6. update
        if k >= 0:
            cnt[k] += 1
            S[k] = S[k] + s
            A[k] = A[k] + s * c
            F[k] = A[k] / S[k]
        else:
            k = K
            K += 1
            cnt[k], S[k], A[k], F[k], ccls[k], founder[k], fscore[k] = 1, s, s * c, c, CLS[g], g, s
        joined[g] = k
    # 7. scores
    score = np.zeros(K, dtype)
    for k in range(K):
        sc = S[k] / dtype(cnt[k]) if conf_type == "avg" else fscore[k]
        if n_views > 0:
            sc = sc * (dtype(min(int(cnt[k]), n_views)) / dtype(n_views))
        score[k] = sc
    # 8. output rows
    order = sorted(range(K), key=lambda k: (-(float(score[k]) + 0.0), int(founder[k])))
    fused = np.zeros((N, 6), dtype)
    members = np.zeros(N, np.int32)
    rowof = np.zeros(K, np.int64)
    for r, k in enumerate(order):
        w, h = F[k, 2] - F[k, 0], F[k, 3] - F[k, 1]
        x, y = (F[k, 0] + w / dtype(2), F[k, 1] + h / dtype(2)) if center else (F[k, 0], F[k, 1])
        fused[r] = (x, y, w, h, score[k], ccls[k])
        members[r] = cnt[k]
        rowof[k] = r
    assign = np.full(N, -1, np.int32)
    for g, i in enumerate(cand):
        assign[i] = rowof[joined[g]]
    return fused, members, K, assign


def fuse_ref_batch(boxes, **kw):
    """(B, N, 6) -> fused (B, N, 6), members (B, N), count (B,), assign (B, N)."""
    res = [fuse_ref(b, **kw) for b in np.asarray(boxes)]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32),
            np.stack([r[3] for r in res]))


def clustered(rng, n=480, copies=12, classes=2, center_sigma=0.012, size_sigma=0.036):
    """ceil(n / copies) objects x ``copies`` jittered reports, shuffled and cut to n rows: (n, 6) float32, centre format.
    Object centres U(0.1, 0.9), sides U(0.06, 0.2); a report moves the centre by N(0, center_sigma) and scales each side by
    1 + N(0, size_sigma); scores U(0.05, 1); every report carries its object's class."""
    objects = -(-n // copies)
    cx, cy = rng.uniform(0.1, 0.9, objects), rng.uniform(0.1, 0.9, objects)
    w, h = rng.uniform(0.06, 0.2, objects), rng.uniform(0.06, 0.2, objects)
    cls = rng.integers(0, classes, objects).astype(np.float64)
    rows = np.zeros((objects, copies, 6))
    rows[..., 0] = cx[:, None] + rng.normal(0, center_sigma, (objects, copies))
    rows[..., 1] = cy[:, None] + rng.normal(0, center_sigma, (objects, copies))
    rows[..., 2] = w[:, None] * (1 + rng.normal(0, size_sigma, (objects, copies)))
    rows[..., 3] = h[:, None] * (1 + rng.normal(0, size_sigma, (objects, copies)))
    rows[..., 4] = rng.uniform(0.05, 1.0, (objects, copies))
    rows[..., 5] = cls[:, None]
    rows = rows.reshape(-1, 6)
    return rows[rng.permutation(rows.shape[0])[:n]].astype(np.float32)


# ---- views
def _coef(dst_n, src_n):
    """Per output index: source index s, its neighbour min(s + 1, src_n - 1) and the fp32 weight of the neighbour."""
    d = np.arange(dst_n, dtype=np.float64)
    f = (d + 0.5) * (np.float64(src_n) / np.float64(dst_n)) - 0.5
    s = np.floor(f)
    f = f - s
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= src_n - 1
    s = np.where(lo, 0, np.where(hi, src_n - 1, s))
    f = np.where(lo | hi, 0.0, f)
    return s, np.minimum(s + 1, src_n - 1), f.astype(np.float32)


def tta_view_ref(x, oh, ow, flip_lr=False, flip_ud=False):
    """yolo_tta_view: x (n, c, h, w) float32 -> (n, c, oh, ow) float32."""
    x = np.asarray(x, np.float32)
    h, w = x.shape[2:]
    if (oh, ow) == (h, w):
        v = x.copy()
    else:
        y0, y1, wy = _coef(oh, h)
        x0, x1, wx = _coef(ow, w)
        one = np.float32(1)
        top = (one - wx) * x[:, :, y0][:, :, :, x0] + wx * x[:, :, y0][:, :, :, x1]
        bot = (one - wx) * x[:, :, y1][:, :, :, x0] + wx * x[:, :, y1][:, :, :, x1]
        wy = wy[:, None]
        v = (one - wy) * top + wy * bot
        assert v.dtype == np.float32
    if flip_ud:
        v = v[:, :, ::-1]
    if flip_lr:
        v = v[:, :, :, ::-1]
    return np.ascontiguousarray(v)


def unflip_ref(boxes, row_offset, rows, flip_lr, flip_ud):
    """yolo_boxes_unflip on a copy of the (b, n_total, 6) float32 buffer."""
    out = np.array(boxes, np.float32, copy=True)
    blk = out[:, row_offset:row_offset + rows]
    if flip_lr:
        blk[..., 0] = np.float32(1) - blk[..., 0]
    if flip_ud:
        blk[..., 1] = np.float32(1) - blk[..., 1]
    return out


# ---- hand-worked cases: exactly representable numbers (scores 0.5 / 0.25 / 0.375, corners in eighths), corner format, so every
# sum, product and quotient below is exact and the expected rows are literals. (name, rows, keyword arguments, expected fused
# rows, expected members, expected assign)
_A = [0, 0, 1, 1, 0.5, 0]                  # the unit square
_B = [0.375, 0, 0.625, 1, 0.25, 0]         # its right 5/8: IoU with _A = 0.625
HAND_CASES = [
    # S = 0.75, A.x1 = 0.25 * 0.375 = 0.09375 -> F.x1 = 0.125; A.x2 = 0.5 + 0.25 = 0.75 -> F.x2 = 1; score 0.75 / 2
    ("two_box_merge", [_A, _B], dict(iou_threshold=0.5), [[0.125, 0, 0.875, 1, 0.375, 0]], [2], [0, 0]),
    # all 0.5: after B F = (0.1875, 1); C = A again has IoU 0.8125 with it; S = 1.5, A.x1 = 0.1875 -> 0.125, A.x2 = 1.5 -> 1
    ("three_box_merge", [_A, [0.375, 0, 0.625, 1, 0.5, 0], [0, 0, 1, 1, 0.5, 0]], dict(iou_threshold=0.5),
     [[0.125, 0, 0.875, 1, 0.5, 0]], [3], [0, 0, 0]),
    # drift towards: A (0..1) + B (0.25..1.25) -> F (0.125..1.125); C (0.5..1.5) has IoU 1/3 with the founder A but
    # 0.625 / 1.375 = 0.4545 with F: it joins. S = 1.5, A.x1 = 0.125 + 0.25 = 0.375 -> 0.25, A.x2 = 0.5 + 0.625 + 0.75 -> 1.25
    ("drift_joins_fused_not_founder", [_A, [0.25, 0, 1, 1, 0.5, 0], [0.5, 0, 1, 1, 0.5, 0]], dict(iou_threshold=0.4),
     [[0.25, 0, 1, 1, 0.5, 0]], [3], [0, 0, 0]),
    # drift away: C (-0.375..0.625) has IoU 0.625 / 1.375 with the founder A but 0.5 / 1.5 with F (0.125..1.125): a new cluster
    ("drift_leaves_founder", [_A, [0.25, 0, 1, 1, 0.5, 0], [-0.375, 0, 1, 1, 0.5, 0]], dict(iou_threshold=0.4),
     [[0.125, 0, 1, 1, 0.5, 0], [-0.375, 0, 1, 1, 0.5, 0]], [2, 1], [0, 0, 1]),
    # C (0.75..1.75) overlaps P (0..1) and Q (1.5..2.5) by 0.25 each: the same IoU bits, so the cluster created first takes it.
    # P first: S = 0.75, A.x1 = 0.1875 -> 0.25, A.x2 = 0.5 + 0.4375 -> 1.25, score 0.375, behind Q's 0.5
    ("iou_tie_earlier_cluster_p", [_A, [1.5, 0, 1, 1, 0.5, 0], [0.75, 0, 1, 1, 0.25, 0]], dict(iou_threshold=0.125),
     [[1.5, 0, 1, 1, 0.5, 0], [0.25, 0, 1, 1, 0.375, 0]], [1, 2], [1, 0, 1]),
    # Q first: S = 0.75, A.x1 = 0.75 + 0.1875 -> 1.25, A.x2 = 1.25 + 0.4375 -> 2.25
    ("iou_tie_earlier_cluster_q", [[1.5, 0, 1, 1, 0.5, 0], _A, [0.75, 0, 1, 1, 0.25, 0]], dict(iou_threshold=0.125),
     [[0, 0, 1, 1, 0.5, 0], [1.25, 0, 1, 1, 0.375, 0]], [1, 2], [1, 0, 1]),
    # equal scores: the lower row founds, and the cluster keeps the founder's class
    ("score_tie_lower_row_founds", [[0, 0, 1, 1, 0.5, 2], [0, 0, 1, 1, 0.5, 1]], dict(iou_threshold=0.5, class_agnostic=True),
     [[0, 0, 1, 1, 0.5, 2]], [2], [0, 0]),
    ("class_aware_keeps_apart", [[0, 0, 1, 1, 0.5, 2], [0, 0, 1, 1, 0.5, 1]], dict(iou_threshold=0.5),
     [[0, 0, 1, 1, 0.5, 2], [0, 0, 1, 1, 0.5, 1]], [1, 1], [0, 1]),
    # final scores tie at 0.375: {0.5, 0.25} founded at rank 0 comes before the single 0.375 box of rank 1
    ("output_tie_founder_rank", [[4, 0, 1, 1, 0.375, 0], _B, _A], dict(iou_threshold=0.5),
     [[0.125, 0, 0.875, 1, 0.375, 0], [4, 0, 1, 1, 0.375, 0]], [2, 1], [1, 0, 0]),
    # n_views: three members of two views count as two (factor 1), a single report of two views halves
    ("n_views_clamp", [_A, [0.375, 0, 0.625, 1, 0.5, 0], [0, 0, 1, 1, 0.5, 0], [4, 0, 1, 1, 0.5, 0]], dict(iou_threshold=0.5, n_views=2),
     [[0.125, 0, 0.875, 1, 0.5, 0], [4, 0, 1, 1, 0.25, 0]], [3, 1], [0, 0, 0, 1]),
    ("n_views_four", [_A, _B], dict(iou_threshold=0.5, n_views=4), [[0.125, 0, 0.875, 1, 0.1875, 0]], [2], [0, 0]),
    ("conf_max", [_A, _B], dict(iou_threshold=0.5, conf_type="max"), [[0.125, 0, 0.875, 1, 0.5, 0]], [2], [0, 0]),
    # a filtered row, and the strict comparison of the objectness threshold
    ("obj_threshold_strict", [_A, _B, [0, 0, 1, 1, 0.125, 0]], dict(iou_threshold=0.5, obj_threshold=0.125),
     [[0.125, 0, 0.875, 1, 0.375, 0]], [2], [0, 0, -1]),
]


def to_center(rows):
    """Corner-format rows as centre-format rows (exact for the hand cases: halves of eighths)."""
    r = np.array(rows, np.float32).reshape(-1, 6)
    r[:, 0] += r[:, 2] / np.float32(2)
    r[:, 1] += r[:, 3] / np.float32(2)
    return r
