"""numpy restatement of yolo_soft_nms, written from the contract in include/yolo_mi355x.h, step by step in ``dtype``
(np.float32: the kernel's bits; np.float64: the yardstick of the fp32 walk, with the library's exp for w). numpy's elementwise fp32
operations round once, like the kernels built without FMA contraction. The walk is the literal global loop over the whole image;
``soft_nms_ref_segments`` walks every class on its own and merges, which is how the kernel works and must give the same."""
import numpy as np

F32 = np.float32
METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def w_ref(t, dtype=np.float32):
    """Step 4: w(t) ~ exp(-t). fp32: the header's sequence, operation by operation, on an array; fp64: exp itself."""
    shape = np.shape(t)
    t = np.asarray(t, dtype).reshape(-1)
    if dtype is not np.float32:
        with np.errstate(all="ignore"):
            return np.exp(-t).reshape(shape)
    f = np.float32
    with np.errstate(all="ignore"):
        kf = np.rint(t * f(float.fromhex("0x1.715476p+0")))                        # half to even
        big = ~(kf <= f(125.0))                                                   # also NaN
        k = np.where(big, f(0), kf)
        r = (t - k * f(float.fromhex("0x1.63p-1"))) - k * f(float.fromhex("-0x1.bd0106p-13"))
        p = np.full(t.shape, f(float.fromhex("-0x1.a01a02p-13")), f)
        for c in ("0x1.6c16c2p-10", "-0x1.111112p-7", "0x1.555556p-5", "-0x1.555556p-3", "0x1p-1", "-0x1p+0", "0x1p+0"):
            p = p * r + f(float.fromhex(c))
        assert p.dtype == np.float32 and r.dtype == np.float32
        w = (np.ascontiguousarray(p).view(np.int32) - (k.astype(np.int32) << 23)).view(np.float32)
    w = np.where(big, f(0), w)
    return np.where(np.isnan(t), t, w).astype(f).reshape(shape)


def _corners(rows, center, dtype):
    x, y, w, h = (rows[:, k].astype(dtype) for k in range(4))
    if center:
        x = x - w / dtype(2)
        y = y - h / dtype(2)
    return x, y, x + w, y + h, w * h


def soft_nms_ref(boxes, iou_threshold=0.45, obj_threshold=0.5, score_threshold=None, box_format="corners", method="gaussian", sigma=0.5,
                 class_agnostic=False, max_det=None, dtype=np.float32, margins=None, only=None):
    """One image. boxes: (N, 6) float32 rows [x, y, w, h, obj, cls]. Returns (keep (N,) int32 with -1 behind the emitted rows, count,
    scores (N,) dtype with 0 behind them, rescored (N, 6) float32 copy of boxes with column 4 of the emitted rows replaced).
    ``margins``: a dict whose lists ``iou`` (|iou - threshold| of every IoU compared with it), ``pick`` (best score minus the
    runner-up's, of every pick with a runner-up), ``score`` (|s - score_threshold| of every rescored row) and ``t`` (every argument of
    w) are extended.
    ``only``: restrict the candidates to these input rows (the per-segment walk)."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    N = boxes.shape[0]
    center = box_format == "center"
    m = METHODS[method]
    thr = dtype(np.float32(iou_threshold))                       # compared as (float) iou_threshold
    sg = dtype(np.float32(sigma))
    eps = dtype(np.float32(1e-6))
    sthr = float(obj_threshold if score_threshold is None else score_threshold)
    cap = int(max_det) if max_det else 0
    # 1. candidates
    cand = np.array([i for i in range(N) if float(boxes[i, 4]) > float(obj_threshold) and (only is None or i in only)], np.int64)
    rows = boxes[cand] if len(cand) else np.zeros((0, 6), np.float32)
    X1, Y1, X2, Y2, AREA = _corners(rows, center, dtype)
    CLS = rows[:, 5]
    S = (rows[:, 4] + np.float32(0.0)).astype(dtype)             # -0 -> +0
    # 3. the walk: live = not emitted, not removed, (double) s > score_threshold
    live = S.astype(np.float64) > sthr
    keep = np.full(N, -1, np.int32)
    scores = np.zeros(N, dtype)
    rescored = boxes.copy()
    count = 0
    while live.any() and not (cap and count == cap):
        idx = np.nonzero(live)[0]
        top = S[idx].max()
        g = int(idx[S[idx] == top][0])                            # ties to the lowest input row: cand is ascending
        if margins is not None and len(idx) > 1:
            rest = S[idx][idx != g]
            margins["pick"].append(float(top) - float(rest.max()))
        keep[count], scores[count] = cand[g], S[g]
        rescored[cand[g], 4] = np.float32(S[g])
        count += 1
        live[g] = False
        # 2. interaction
        j = np.nonzero(live & (np.ones(len(cand), bool) if class_agnostic else (CLS == CLS[g])))[0]
        if not len(j):
            continue
        xa, ya = np.maximum(X1[g], X1[j]), np.maximum(Y1[g], Y1[j])
        xb, yb = np.minimum(X2[g], X2[j]), np.minimum(Y2[g], Y2[j])
        inter = np.maximum(xb - xa, dtype(0)) * np.maximum(yb - ya, dtype(0))
        with np.errstate(all="ignore"):
            iou = inter / (((AREA[g] + AREA[j]) - inter) + eps)
            if margins is not None and m != 2:
                margins["iou"].extend(np.abs(iou.astype(np.float64) - float(thr)).tolist())
            if m == 0:
                live[j[~(iou < thr)]] = False
                continue
            if m == 1:
                hit = iou > thr
                S[j[hit]] = S[j[hit]] * (dtype(1.0) - iou[hit])
            else:
                t = (iou * iou) / sg
                if margins is not None:
                    margins["t"].extend(t.tolist())
                S[j] = S[j] * w_ref(t, dtype)
        if margins is not None:
            margins["score"].extend(np.abs(S[j].astype(np.float64) - sthr).tolist())
        live[j] = S[j].astype(np.float64) > sthr
    return keep, count, scores, rescored


def soft_nms_ref_segments(boxes, **kw):
    """The same result the way the kernel gets it: one walk per class (float equality; a NaN class is a walk of its own per row),
    each cut at max_det, merged by (emitted score descending, input row ascending), then max_det."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    N = boxes.shape[0]
    dtype = kw.get("dtype", np.float32)
    if kw.get("class_agnostic", False):
        groups = [set(range(N))]
    else:
        groups, seen = [], {}
        for i in range(N):
            c = boxes[i, 5]
            if c != c:
                groups.append({i})
            else:
                seen.setdefault(float(c), set()).add(i)
        groups += list(seen.values())
    em = []
    rescored = boxes.copy()
    for g in groups:
        k, c, s, _ = soft_nms_ref(boxes, only=g, **kw)
        em += [(-float(s[t]), int(k[t]), s[t]) for t in range(c)]
    em.sort(key=lambda e: (e[0], e[1]))
    if kw.get("max_det"):
        em = em[:int(kw["max_det"])]
    keep = np.full(N, -1, np.int32)
    scores = np.zeros(N, dtype)
    for t, (_, i, s) in enumerate(em):
        keep[t], scores[t] = i, s
        rescored[i, 4] = np.float32(s)
    return keep, len(em), scores, rescored


def soft_nms_ref_batch(boxes, **kw):
    """(B, N, 6) -> keep (B, N), count (B,), scores (B, N), rescored (B, N, 6)."""
    res = [soft_nms_ref(b, **kw) for b in np.asarray(boxes)]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32), np.stack([r[2] for r in res]),
            np.stack([r[3] for r in res]))


def new_margins():
    return {"iou": [], "pick": [], "score": [], "t": []}


# ---- inputs
def clustered(rng, n=300, copies=6, classes=2, center_sigma=0.02, size_sigma=0.08):
    """ceil(n / copies) objects x ``copies`` jittered reports, shuffled and cut to n rows: (n, 6) float32, centre format; scores
    U(0.05, 1); every report carries its object's class. Neighbouring reports overlap with IoUs spread over (0, 1)."""
    objects = -(-n // copies)
    cx, cy = rng.uniform(0.1, 0.9, objects), rng.uniform(0.1, 0.9, objects)
    w, h = rng.uniform(0.06, 0.25, objects), rng.uniform(0.06, 0.25, objects)
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


# The random cases of the GPU test: (seed, keyword arguments). Every one is walked in fp32 (the kernel's bits) and in fp64.
RANDOM_SEEDS = list(range(7000, 7060))


def random_case(seed):
    rng = np.random.default_rng(seed)
    method = ("hard", "linear", "gaussian")[seed % 3]
    kw = dict(iou_threshold=float(rng.choice([0.3, 0.45, 0.6])), obj_threshold=float(rng.choice([0.05, 0.25])), box_format="center",
              method=method, sigma=float(rng.choice([0.25, 0.5])), class_agnostic=bool(rng.integers(0, 2)),
              max_det=[None, 20][int(rng.integers(0, 2))])
    if rng.integers(0, 2):
        kw["score_threshold"] = kw["obj_threshold"] + 0.1
    rows = clustered(rng, n=int(rng.integers(150, 320)), classes=int(rng.choice([1, 2, 5])))
    return rows, kw


STEP = 1.4e-6       # relative error one decay adds to a score: w within 1e-6 of exp, its argument's two roundings (t <= 2: 2.4e-7), the
                    # product's 6e-8, the IoU's few roundings; a score takes at most one decay per emission


def compare_with_fp64(rows, kw):
    """Walk ``rows`` in fp32 and in fp64. Returns (fp32 result, status): "agree" - same kept rows in the same order and the emitted
    scores within STEP x emissions; "edge" - they differ and a recorded fp32 margin is below that same bound (rounding decides; the
    case is set aside); "differ" - they differ with every margin clear of it: an error in the contract or in this file."""
    mg = new_margins()
    r32 = soft_nms_ref(rows, dtype=np.float32, margins=mg, **kw)
    r64 = soft_nms_ref(rows, dtype=np.float64, **kw)
    tol = STEP * max(int(r32[1]), 1)
    same = r32[1] == r64[1] and np.array_equal(r32[0], r64[0]) and np.allclose(r32[2], r64[2], rtol=tol, atol=0)
    if same:
        return r32, "agree"
    low = min([min(v) for k, v in mg.items() if v and k != "t"] or [np.inf])
    return r32, "edge" if low < tol else "differ"


# ---- the hand cases of the GPU test: name -> (boxes (N, 6) or (B, N, 6), keyword arguments). C = yolo_soft_nms_onchip_rows().
_UNIT = [0, 0, 1, 1, 0.5, 0]                 # the unit square
_RIGHT = [0.375, 0, 0.625, 1, 0.25, 0]       # its right 5/8: inter = 0.625
PAIR_IOU = F32(0.625) / (((F32(1) + F32(0.625)) - F32(0.625)) + F32(1e-6))      # the contract's expression on the pair, in fp32
LENGTHS = ["0", "1", "63", "64", "65", "C-1", "C", "C+1"]
CASE_NAMES = ([f"len_{n}_{m}" for n in LENGTHS for m in METHODS] +
              [f"{c}_{m}" for c in ("ragged", "ties", "zeros", "nan", "lump", "identical", "corners", "agnostic") for m in METHODS] +
              [f"spill_{m}" for m in METHODS] + ["edge_hard", "edge_linear", "edge_below_hard", "edge_below_linear", "maxdet_1", "maxdet_exact", "maxdet_above",
               "maxdet_tie_cut", "maxdet_tie_cut_agnostic", "score_threshold_above_obj"])


def tied_boxes(seed, n=160):
    """Clustered boxes with score ties inside and across classes and exact duplicates."""
    rng = np.random.default_rng(seed)
    rows = clustered(rng, n=n, classes=3)
    rows[:, 4] = rng.choice(np.array([0.25, 0.5, 0.75, 0.875], F32), n)          # many equal scores
    rows[n // 2:n // 2 + 20] = rows[:20]                                          # duplicates of whole rows
    rows[n // 2 + 20:n // 2 + 30, :5] = rows[20:30, :5]                           # the same box under another class
    rows[n // 2 + 20:n // 2 + 30, 5] = (rows[20:30, 5] + 1) % 3
    return rows


def build_case(name, C):
    base, _, method = name.rpartition("_")
    kw = dict(iou_threshold=0.45, obj_threshold=0.25, box_format="center", method=method if method in METHODS else "gaussian", sigma=0.5)
    if base.startswith("len_"):
        # one class, L candidates (all scores above the threshold). The long ones end after a few dozen emissions: by max_det, or
        # for the Gaussian walk by a final threshold only the best rows pass - their spilled rows still take the first decays
        L = eval(base[4:], {"C": C})
        rng = np.random.default_rng(100 + sum(map(ord, base)))
        rows = clustered(rng, n=max(L, 1), classes=1)
        rows[:, 4] = rng.uniform(0.3, 1.0, len(rows)).astype(F32) if L else F32(0.1)
        if L > 1000:
            kw.update(dict(max_det=40) if method != "gaussian" else dict(score_threshold=0.93))
        return rows, kw
    rng = np.random.default_rng(sum(map(ord, base)))
    if base == "spill":
        # One class. C + 120 near-identical boxes with the highest scores fill the on-chip positions and the first of the spill: the
        # first pick takes all of them out (hard: removed; linear, Gaussian: decayed below the threshold), the spilled ones through
        # the write-back. 3,000 lower-score, mutually overlapping boxes sit behind them in the spill (two batches of loads per
        # thread): every later pick is a spilled winner, and under linear / Gaussian decay its score was rescored there before.
        top = np.tile(np.array([[0.5, 0.5, 0.1, 0.1, 0, 0]], F32), (C + 120, 1))
        top[:, :2] += rng.uniform(-1e-4, 1e-4, (len(top), 2)).astype(F32)
        top[:, 4] = rng.uniform(0.9, 1.0, len(top))
        low = clustered(rng, n=3000, classes=1)
        low[:, 4] = rng.uniform(0.3, 0.85, len(low))
        rows = np.concatenate([top, low])
        return rows[rng.permutation(len(rows))], dict(kw, iou_threshold=0.1, max_det=60)      # 0.1: the linear decay reaches mild overlaps too
    if base == "ragged":                                          # a batch of 3: plain | no candidate at all | candidates that all fail score_threshold
        rows = np.stack([clustered(rng, n=90), clustered(rng, n=90), clustered(rng, n=90)])
        rows[1, :, 4] = 0
        rows[2, :, 4] = rng.uniform(0.26, 0.39, 90)
        return rows, dict(kw, score_threshold=0.4)
    if base == "ties":
        return tied_boxes(21), kw
    if base == "zeros":                                           # -0.0 and +0.0 scores are candidates under obj_threshold -1, and equal
        rows = clustered(rng, n=40, classes=2)
        rows[::3, 4] = -0.0
        rows[1::3, 4] = 0.0
        return rows, dict(kw, obj_threshold=-1.0)
    if base == "nan":                                             # a NaN score is no candidate; a NaN class interacts with nothing
        rows = np.tile(clustered(rng, n=8, classes=1), (4, 1))
        rows[3, 4] = np.nan
        rows[5, 5] = rows[13, 5] = np.nan
        return rows, kw
    if base == "lump":                                            # 1.5, 4094, 5000, 1e9 and -1 share the ordering's last bucket and never interact
        rows = np.tile(clustered(rng, n=6, classes=1), (6, 1))
        rows[:, 5] = np.repeat(np.array([1.5, 4094, 5000, 1e9, -1, 7], F32), 6)
        rows[:, 4] = rng.uniform(0.3, 1, 36)
        return rows, kw
    if base == "identical":
        rows = np.tile(np.array([[0.5, 0.5, 0.2, 0.3, 0.8, 1]], F32), (70, 1))
        rows[:, 4] = rng.uniform(0.3, 1, 70)
        rows[10:20, 4] = 0.6
        return rows, dict(kw, obj_threshold=0.02)                 # low enough for the decayed copies to come out, one after the other
    if base == "corners":
        return clustered(rng, n=200), dict(kw, box_format="corners")
    if base == "agnostic":
        return clustered(rng, n=200, classes=4), dict(kw, class_agnostic=True)
    pair = np.array([_UNIT, _RIGHT], F32)
    if name.startswith("edge_"):                                  # thr == the pair's fp32 IoU: hard removes, linear leaves; one ulp below, linear rescales
        thr = PAIR_IOU if "below" not in name else np.nextafter(PAIR_IOU, F32(0))
        return pair, dict(kw, iou_threshold=float(thr), obj_threshold=0.05, box_format="corners", method=method)
    if name == "score_threshold_above_obj":
        return clustered(rng, n=150), dict(kw, obj_threshold=0.1, score_threshold=0.5)
    # max_det: disjoint boxes (nothing is suppressed), 12 rows, two classes, scores 0.9, 0.8, then a run of six 0.5 across both classes
    rows = np.zeros((12, 6), F32)
    rows[:, 0] = 0.05 + 0.07 * np.arange(12)
    rows[:, 1], rows[:, 2], rows[:, 3] = 0.5, 0.05, 0.05
    rows[:, 4] = [0.5, 0.9, 0.5, 0.3, 0.5, 0.8, 0.5, 0.3, 0.5, 0.3, 0.5, 0.3]
    rows[:, 5] = [1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1]
    kw["method"] = "linear"
    cut = {"maxdet_1": 1, "maxdet_exact": 12, "maxdet_above": 50, "maxdet_tie_cut": 5, "maxdet_tie_cut_agnostic": 5}[name]
    return rows, dict(kw, max_det=cut, class_agnostic=name.endswith("agnostic"))
