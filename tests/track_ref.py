"""numpy restatement of the tracking contract (include/yolo_mi355x.h, "multi-object tracking"): fp32, one rounding per
operation (numpy's elementwise float32 arithmetic), no fused multiply-add. `TrackerRef` is what yolo_track_update must equal bit for
bit; `kalman8_fp64` is the usual 8-state matrix filter in fp64, for comparison with the decoupled fp32 one. The matching is the
definition itself: a walk over the sorted eligible pairs."""
import numpy as np

F32 = np.float32
WP, WV = F32(0.05), F32(0.00625)
FREE, TENTATIVE, TRACKED, LOST = 0, 1, 2, 3
HDR_WORDS, SLOT_WORDS = 4, 26


# ------------------------------------------------------------------------------------------ the filter (any leading shape)
def kf_found(z):
    """mean (..., 8), cov (..., 12) of a track founded from z (..., 4) = (cx, cy, w, h)."""
    z = np.asarray(z, F32)
    mean = np.zeros(z.shape[:-1] + (8,), F32)
    cov = np.zeros(z.shape[:-1] + (12,), F32)
    two_wp, ten_wv = F32(2) * WP, F32(10) * WV
    for c in range(4):
        sc = z[..., 3] if c & 1 else z[..., 2]
        t, u = two_wp * sc, ten_wv * sc
        mean[..., c] = z[..., c]
        cov[..., 3 * c] = t * t
        cov[..., 3 * c + 2] = u * u
    return mean, cov


def kf_predict(mean, cov, lost=None):
    """One constant-velocity step; `lost` (bool, leading shape) marks the slots whose size velocities are zeroed first."""
    mean, cov = np.array(mean, F32), np.array(cov, F32)
    if lost is not None:
        mean[..., 6] = np.where(lost, F32(0), mean[..., 6])
        mean[..., 7] = np.where(lost, F32(0), mean[..., 7])
    sw, sh = mean[..., 2].copy(), mean[..., 3].copy()
    for c in range(4):
        sc = sh if c & 1 else sw
        a, b = WP * sc, WV * sc
        qp, qv = a * a, b * b
        p00, p01, p11 = cov[..., 3 * c].copy(), cov[..., 3 * c + 1].copy(), cov[..., 3 * c + 2].copy()
        mean[..., c] = mean[..., c] + mean[..., 4 + c]
        cov[..., 3 * c] = ((p00 + F32(2) * p01) + p11) + qp
        cov[..., 3 * c + 1] = p01 + p11
        cov[..., 3 * c + 2] = p11 + qv
    return mean, cov


def kf_update(mean, cov, z):
    mean, cov, z = np.array(mean, F32), np.array(cov, F32), np.asarray(z, F32)
    sw, sh = mean[..., 2].copy(), mean[..., 3].copy()
    with np.errstate(all="ignore"):
        for c in range(4):
            sc = sh if c & 1 else sw
            a = WP * sc
            r = a * a
            p00, p01, p11 = cov[..., 3 * c].copy(), cov[..., 3 * c + 1].copy(), cov[..., 3 * c + 2].copy()
            S = p00 + r
            k0, k1 = p00 / S, p01 / S
            y = z[..., c] - mean[..., c]
            mean[..., c] = mean[..., c] + k0 * y
            mean[..., 4 + c] = mean[..., 4 + c] + k1 * y
            cov[..., 3 * c] = p00 - k0 * p00
            cov[..., 3 * c + 1] = p01 - k0 * p01
            cov[..., 3 * c + 2] = p11 - k1 * p01
    return mean, cov


def kalman8_fp64(zs):
    """The usual 8-state filter with F, H, Q, R as matrices, in fp64, over measurements zs (T, 4): founded from zs[0], then
    predict + update per frame. Returns the means (T, 8) and full covariances (T, 8, 8) after every frame."""
    zs = np.asarray(zs, np.float64)
    wp, wv = float(WP), float(WV)                                     # the fp32 constants, exactly
    Fm = np.eye(8)
    Fm[:4, 4:] = np.eye(4)
    H = np.eye(4, 8)
    x = np.concatenate([zs[0], np.zeros(4)])
    s0 = np.array([zs[0, 2], zs[0, 3], zs[0, 2], zs[0, 3]])
    P = np.diag(np.concatenate([(float(F32(2) * WP) * s0) ** 2, (float(F32(10) * WV) * s0) ** 2]))
    means, covs = [x.copy()], [P.copy()]
    for z in zs[1:]:
        s = np.array([x[2], x[3], x[2], x[3]])
        Q = np.diag(np.concatenate([(wp * s) ** 2, (wv * s) ** 2]))
        x = Fm @ x
        P = Fm @ P @ Fm.T + Q
        s = np.array([x[2], x[3], x[2], x[3]])
        R = np.diag((wp * s) ** 2)
        S = H @ P @ H.T + R
        K = P @ H.T @ np.linalg.inv(S)
        x = x + K @ (z - H @ x)
        P = (np.eye(8) - K @ H) @ P
        means.append(x.copy())
        covs.append(P.copy())
    return np.array(means), np.array(covs)


# ------------------------------------------------------------------------------------------ IoU and matching
def det_corners(rows, center):
    """x1, y1, x2, y2, area of box rows (D, 6): the NMS's corners."""
    rows = np.asarray(rows, F32)
    x, y, w, h = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    if center:
        x, y = x - w / F32(2), y - h / F32(2)
    return x, y, x + w, y + h, w * h


def iou_matrix(mean, rows, center):
    """(S, D) fp32 IoU of the slots' boxes (mean (S, 8), centre form) against the detections rows (D, 6)."""
    mean = np.asarray(mean, F32)
    sx1 = mean[:, 0] - mean[:, 2] / F32(2)
    sy1 = mean[:, 1] - mean[:, 3] / F32(2)
    sx2, sy2, sa = sx1 + mean[:, 2], sy1 + mean[:, 3], mean[:, 2] * mean[:, 3]
    dx1, dy1, dx2, dy2, da = det_corners(rows, center)
    with np.errstate(all="ignore"):
        iw = np.maximum(np.minimum(dx2[None], sx2[:, None]) - np.maximum(dx1[None], sx1[:, None]), F32(0))
        ih = np.maximum(np.minimum(dy2[None], sy2[:, None]) - np.maximum(dy1[None], sy1[:, None]), F32(0))
        inter = iw * ih
        iou = inter / (((da[None] + sa[:, None]) - inter) + F32(1e-6))
    assert iou.dtype == F32
    return iou


def greedy_match(iou, eligible):
    """The definition: walk the eligible pairs by (iou descending, slot ascending, detection ascending); take a pair iff neither
    side is taken. Returns [(slot, det), ...] in the order taken."""
    si, di = np.nonzero(eligible)
    order = np.lexsort((di, si, -iou[si, di].astype(np.float64)))
    s_taken, d_taken, out = set(), set(), []
    for s, d in zip(si[order].tolist(), di[order].tolist()):
        if s not in s_taken and d not in d_taken:
            s_taken.add(s)
            d_taken.add(d)
            out.append((s, d))
    return out


def brute_force_match(iou, eligible):
    """The same walk over a Python sort of explicit tuples (no lexsort)."""
    pairs = sorted((-float(iou[s, d]), s, d) for s in range(iou.shape[0]) for d in range(iou.shape[1]) if eligible[s, d])
    s_taken, d_taken, out = set(), set(), []
    for _, s, d in pairs:
        if s not in s_taken and d not in d_taken:
            s_taken.add(s)
            d_taken.add(d)
            out.append((s, d))
    return out


def mutual_best_match(iou, eligible):
    """What the kernel does: repeatedly take every pair whose sides prefer each other among the unmatched (largest iou, ties to the
    lowest index). Returns (pairs, rounds)."""
    S, D = iou.shape
    s_free, d_free = np.ones(S, bool), np.ones(D, bool)
    out, rounds = [], 0
    while True:
        live = eligible & s_free[:, None] & d_free[None]
        if not live.any():
            return out, rounds
        rounds += 1
        v = np.where(live, iou.astype(np.float64), -np.inf)
        best_d = v.argmax(1)                                          # first maximum = lowest index
        best_s = v.argmax(0)
        for s in range(S):
            d = best_d[s]
            if live[s, d] and best_s[d] == s:
                out.append((s, int(d)))
                s_free[s] = d_free[d] = False


# ------------------------------------------------------------------------------------------ the tracker
class TrackerRef:
    def __init__(self, streams, max_tracks=128, high_threshold=0.5, low_threshold=0.1, new_threshold=0.6, match_iou=(0.2, 0.5, 0.3),
                 max_age=30, class_agnostic=False, box_format="center"):
        self.B, self.M = streams, max_tracks
        self.high, self.low, self.new = float(high_threshold), float(low_threshold), float(new_threshold)
        self.match_iou = tuple(float(m) for m in match_iou)
        self.max_age, self.agnostic, self.center = int(max_age), bool(class_agnostic), box_format == "center"
        B, M = streams, max_tracks
        self.frame, self.next_id, self.overflow = np.zeros(B, np.int32), np.ones(B, np.int32), np.zeros(B, np.int32)
        self.state, self.id, self.lost = np.zeros((B, M), np.int32), np.zeros((B, M), np.int32), np.zeros((B, M), np.int32)
        self.cls, self.score = np.zeros((B, M), F32), np.zeros((B, M), F32)
        self.mean, self.cov = np.zeros((B, M, 8), F32), np.zeros((B, M, 12), F32)

    def reset(self, streams=None):
        for s in (range(self.B) if streams is None else streams):
            self.frame[s], self.next_id[s], self.overflow[s] = 0, 1, 0
            for a in (self.state, self.id, self.lost, self.cls, self.score, self.mean, self.cov):
                a[s] = 0

    def slots(self):
        return dict(frame=self.frame.copy(), next_id=self.next_id.copy(), overflow=self.overflow.copy(), state=self.state.copy(),
                    id=self.id.copy(), cls=self.cls.copy(), score=self.score.copy(), lost_frames=self.lost.copy(),
                    mean=self.mean.copy(), cov=self.cov.copy())

    def _free(self, s, k):
        for a in (self.state, self.id, self.lost, self.cls, self.score, self.mean, self.cov):
            a[s, k] = 0

    def _match(self, s, slots, dets, rows, thr, slot_det, det_slot):
        if len(slots) == 0 or len(dets) == 0:
            return
        iou = iou_matrix(self.mean[s, slots], rows[dets], self.center)
        elig = iou > F32(thr)
        if not self.agnostic:
            elig &= self.cls[s, slots][:, None] == rows[dets, 5][None]
        for a, b in greedy_match(iou, elig):
            slot_det[slots[a]], det_slot[dets[b]] = dets[b], slots[a]

    def update(self, boxes, keep=None, count=None):
        """boxes (B, N, 6); keep (B, N) int and count (B) int as in the contract. Returns out_boxes (B, M, 6), out_ids (B, M),
        out_count (B), det_ids (B, N)."""
        boxes = np.ascontiguousarray(boxes, F32)
        B, N, _ = boxes.shape
        assert B == self.B and (keep is None or count is not None)
        M = self.M
        out_boxes, out_ids = np.zeros((B, M, 6), F32), np.zeros((B, M), np.int32)
        out_count, det_ids = np.zeros(B, np.int32), np.zeros((B, N), np.int32)
        for s in range(B):
            cnt = N if count is None else int(min(max(int(count[s]), 0), N))
            rowidx = np.arange(cnt) if keep is None else np.asarray(keep[s, :cnt]).astype(np.int64)
            valid = (rowidx >= 0) & (rowidx < N)
            rows = boxes[s, np.where(valid, rowidx, 0)] if cnt else np.zeros((0, 6), F32)
            obj = rows[:, 4].astype(np.float64)
            high = valid & (obj > self.high)
            low = valid & (obj > self.low) & (obj <= self.high)
            z = rows[:, :4].copy()
            if not self.center:
                z[:, 0] = rows[:, 0] + rows[:, 2] / F32(2)
                z[:, 1] = rows[:, 1] + rows[:, 3] / F32(2)
            # 1. predict
            st0 = self.state[s].copy()
            live = st0 != FREE
            m, c = kf_predict(self.mean[s], self.cov[s], st0 == LOST)
            self.mean[s], self.cov[s] = np.where(live[:, None], m, self.mean[s]), np.where(live[:, None], c, self.cov[s])
            # 2. - 4. the matchings
            slot_det, det_slot = np.full(M, -1), np.full(cnt, -1)
            self._match(s, np.nonzero((st0 == TRACKED) | (st0 == LOST))[0], np.nonzero(high)[0], rows, self.match_iou[0], slot_det, det_slot)
            self._match(s, np.nonzero((st0 == TRACKED) & (slot_det < 0))[0], np.nonzero(low)[0], rows, self.match_iou[1], slot_det, det_slot)
            self._match(s, np.nonzero(st0 == TENTATIVE)[0], np.nonzero(high & (det_slot < 0))[0], rows, self.match_iou[2], slot_det, det_slot)
            # 4. - 6. the slots
            listed = np.zeros(M, bool)
            for k in np.nonzero(live)[0]:
                d = slot_det[k]
                if d >= 0:
                    self.mean[s, k], self.cov[s, k] = kf_update(self.mean[s, k], self.cov[s, k], z[d])
                    self.state[s, k], self.score[s, k], self.lost[s, k] = TRACKED, rows[d, 4], 0
                    listed[k] = True
                elif st0[k] == TENTATIVE:
                    self._free(s, k)
                else:
                    self.state[s, k] = LOST
                    self.lost[s, k] += 1
                    if self.lost[s, k] > self.max_age:
                        self._free(s, k)
            # 7. founding
            for j in np.nonzero(high & (det_slot < 0) & (obj > self.new))[0]:
                free = np.nonzero(self.state[s] == FREE)[0]
                if len(free) == 0:
                    self.overflow[s] += 1
                    continue
                k = free[0]
                self.mean[s, k], self.cov[s, k] = kf_found(z[j])
                self.id[s, k], self.cls[s, k], self.score[s, k], self.lost[s, k] = self.next_id[s], rows[j, 5], rows[j, 4], 0
                self.next_id[s] += 1
                self.state[s, k] = TRACKED if self.frame[s] == 0 else TENTATIVE
                listed[k] = self.state[s, k] == TRACKED
                det_slot[j] = k
            self.frame[s] += 1
            # outputs
            ks = np.nonzero(listed)[0]
            ks = ks[np.argsort(self.id[s, ks], kind="stable")]
            out_count[s] = len(ks)
            for r, k in enumerate(ks):
                mu = self.mean[s, k]
                x = mu[0] if self.center else mu[0] - mu[2] / F32(2)
                y = mu[1] if self.center else mu[1] - mu[3] / F32(2)
                out_boxes[s, r] = (x, y, mu[2], mu[3], self.score[s, k], self.cls[s, k])
                out_ids[s, r] = self.id[s, k]
            for j in np.nonzero(det_slot >= 0)[0]:
                k = det_slot[j]
                det_ids[s, rowidx[j]] = -self.id[s, k] if self.state[s, k] == TENTATIVE else self.id[s, k]
        return out_boxes, out_ids, out_count, det_ids


# ------------------------------------------------------------------------------------------ scenes
def scene_frame(rng, pos, size, cls, score, pos_noise=0.002, size_noise=0.02):
    """Box rows (len(pos), 6) in centre format: positions with Gaussian noise `pos_noise`, sizes with relative noise `size_noise`."""
    k = len(pos)
    rows = np.zeros((k, 6))
    rows[:, :2] = pos + rng.normal(0, pos_noise, (k, 2))
    rows[:, 2:4] = size * (1 + rng.normal(0, size_noise, (k, 2)))
    rows[:, 4], rows[:, 5] = score, cls
    return rows.astype(F32)


def linear_scene(rng, objects=6, frames=120, classes=2):
    """`objects` boxes moving linearly inside the unit square: returns a list of `frames` arrays (objects, 6), row i = object i."""
    start = rng.uniform(0.15, 0.45, (objects, 2)) + np.arange(objects)[:, None] * np.array([0.07, 0.03])
    vel = rng.uniform(-0.002, 0.002, (objects, 2))
    size = rng.uniform(0.05, 0.09, (objects, 2))
    cls = np.arange(objects) % classes
    score = rng.uniform(0.7, 0.95, objects)
    return [scene_frame(rng, start + vel * t, size, cls, score) for t in range(frames)]


def crowd(rng, n_objects, n_rows, frame, spread=1.0, classes=3, dropout=0.15, low_share=0.2):
    """A frame of a synthetic crowd for the geometry tests: object o sits at a seeded position, drifts with the frame, and is
    reported with probability 1 - dropout, a `low_share` of them with a score between the default low and high thresholds.
    Returns (n_rows, 6) rows in centre format, shuffled, zero rows behind the reported objects; more objects than rows are cut."""
    base = np.random.default_rng(1234)
    pos = base.uniform(0.05, 0.95, (n_objects, 2)) * spread
    vel = base.uniform(-0.004, 0.004, (n_objects, 2))
    size = base.uniform(0.03, 0.08, (n_objects, 2))
    cls = base.integers(0, classes, n_objects)
    seen = rng.uniform(size=n_objects) > dropout
    score = np.where(rng.uniform(size=n_objects) < low_share, rng.uniform(0.15, 0.45, n_objects), rng.uniform(0.55, 0.99, n_objects))
    rows = scene_frame(rng, pos + vel * frame, size, cls, score)[seen]
    rows = rows[rng.permutation(len(rows))][:n_rows]
    out = np.zeros((n_rows, 6), F32)
    out[:len(rows)] = rows
    return out, len(rows)


def to_corner(rows):
    rows = np.array(rows, F32)
    rows[..., 0] = rows[..., 0] - rows[..., 2] / F32(2)
    rows[..., 1] = rows[..., 1] - rows[..., 3] / F32(2)
    return rows
