// metrics.hip — mean average precision on the device (the validation step the reference names as its
// bottleneck, README.md:32; next to the hot path: it consumes the kept boxes of NMS).
//
// Replaces calc_mAP (reference: code/utils.py:193-274), an O(D*G) Python loop that builds two fresh tensors per
// (detection, ground truth) pair. Same semantics:
//   per class with >= 1 ground truth: detections in descending-objectness order (stable); each detection looks at
//   the ground truths of ITS image and class in list order, takes the FIRST one with the largest IoU (> 0), and is a
//   true positive iff that IoU > threshold and the ground truth is still unassigned; precision/recall from fp32
//   cumulative sums, the point (recall 0, precision 1) prepended, trapezoid area; mAP = mean over those classes.
// Ordering (two stable sorts of 64-bit keys) is done by the caller; this file does the sequential-per-class matching
// (one wave per class: lanes evaluate the IoUs of one detection in parallel, a wave-wide first-argmax picks the
// ground truth) and the AP integration. IoU is calc_iou's arithmetic (utils.py:38-84), fp32, no FMA contraction
// (this file is built with -ffp-contract=off like the post-processing units).
// yolo_eval_detections does the same at up to 16 thresholds in one pass, without the sequential walk (further down).
#include "common.h"

namespace yolo {

__device__ __forceinline__ float iou_boxes(const float* a, const float* b, int center) {
    float ax = a[0], ay = a[1], bx = b[0], by = b[1];
    const float aw = a[2], ah = a[3], bw = b[2], bh = b[3];
    if (center) { ax = ax - aw / 2; ay = ay - ah / 2; bx = bx - bw / 2; by = by - bh / 2; }
    const float xa = fmaxf(ax, bx), ya = fmaxf(ay, by);
    const float xb = fminf(ax + aw, bx + bw), yb = fminf(ay + ah, by + bh);
    float iw = xb - xa, ih = yb - ya;
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = iw * ih;
    const float uni = (aw * ah + bw * bh) - inter;
    return inter / (uni + 1e-6f);
}

// dets / gts: rows [img, x, y, w, h, obj, cls] already ordered (dets: class asc, objectness desc, stable;
// gts: class asc, image asc, stable). det_off / gt_off: [nc + 1] class boundaries. One 64-lane block per class.
__global__ __launch_bounds__(64) void map_match_kernel(const float* __restrict__ dets, const int* __restrict__ det_off,
                                                       const float* __restrict__ gts, const int* __restrict__ gt_off,
                                                       int* __restrict__ assigned, float* __restrict__ tp, float iou_thr, int center) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int d0 = det_off[c], d1 = det_off[c + 1], g0 = gt_off[c], g1 = gt_off[c + 1];
    if (g1 == g0) return;                                  // class without ground truth: skipped by the reference
    for (int d = d0; d < d1; ++d) {
        const float* det = dets + (size_t)d * 7;
        const float img = det[0];
        // ground truths of this image inside the class range (sorted by image): lower / upper bound
        int lo = g0, hi = g1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (gts[(size_t)mid * 7] < img) lo = mid + 1; else hi = mid; }
        const int s = lo;
        hi = g1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (gts[(size_t)mid * 7] <= img) lo = mid + 1; else hi = mid; }
        const int e = lo;
        float best = 0.f;                                  // `best_iou = 0`, updated on strict `>`
        int best_idx = 0;
        for (int base = s; base < e; base += 64) {
            const int gi = base + lane;
            float v = -1.f;
            if (gi < e) v = iou_boxes(det + 1, gts + (size_t)gi * 7 + 1, center);
            // wave max, then the lowest index holding it (first maximum)
            float m = v;
            for (int sft = 32; sft > 0; sft >>= 1) m = fmaxf(m, __shfl_xor(m, sft));
            if (m > best) {
                const unsigned long long who = __ballot(v == m);
                best = m;
                best_idx = base - s + (__ffsll((long long)who) - 1);
            }
        }
        if (lane == 0) {
            float flag = 0.f;
            if (best > iou_thr) {
                if (assigned[s + best_idx] == 0) { flag = 1.f; assigned[s + best_idx] = 1; }
            }
            tp[d] = flag;
        }
        __syncthreads();                                   // the next detection must see the assignment
    }
}

// one block per class: AP = trapz(precisions, recalls) with (0, 1) prepended; ap[c] = -1 for classes without GT
__global__ __launch_bounds__(256) void map_ap_kernel(const float* __restrict__ tp, const int* __restrict__ det_off,
                                                     const int* __restrict__ gt_off, float* __restrict__ ap) {
    __shared__ float s_tp[256];
    __shared__ double s_area[256];
    __shared__ float carry_tp;
    __shared__ float prev_p, prev_r;
    const int c = blockIdx.x, t = threadIdx.x;
    const int d0 = det_off[c], d1 = det_off[c + 1];
    const int ng = gt_off[c + 1] - gt_off[c];
    if (ng == 0) { if (t == 0) ap[c] = -1.f; return; }
    if (t == 0) { carry_tp = 0.f; prev_p = 1.f; prev_r = 0.f; }
    double area = 0.0;
    __syncthreads();
    for (int base = d0; base < d1; base += 256) {
        const int d = base + t;
        s_tp[t] = d < d1 ? tp[d] : 0.f;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {          // inclusive scan (exact: small integers in fp32)
            const float v = t >= off ? s_tp[t - off] : 0.f;
            __syncthreads();
            s_tp[t] += v;
            __syncthreads();
        }
        const float ctp = carry_tp + s_tp[t];
        const float n_seen = (float)(d - d0 + 1);          // cum_TP + cum_FP
        const float p = ctp / n_seen, r = ctp / (float)ng;
        // trapezoid with the previous point
        float pp, pr;
        if (t == 0) { pp = prev_p; pr = prev_r; }
        else {
            const float ctp_prev = carry_tp + s_tp[t - 1];
            pp = ctp_prev / (n_seen - 1.f);
            pr = ctp_prev / (float)ng;
        }
        s_area[t] = d < d1 ? (double)((r - pr) * (p + pp)) : 0.0;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) s_area[t] += s_area[t + s];
            __syncthreads();
        }
        if (t == 0) area += s_area[0];
        __syncthreads();
        if (t == 255 || d == d1 - 1) {
            if (d < d1) { prev_p = p; prev_r = r; }
        }
        __syncthreads();
        if (t == 0) carry_tp += s_tp[255];
        __syncthreads();
    }
    if (t == 0) ap[c] = (float)(area / 2.0);
}

// ---- evaluation at several IoU thresholds in one pass (yolo_eval_detections) --------------------------------------
// The ground truth a detection looks at in the walk above does not depend on the threshold, and neither does its IoU; only
// `assigned` does, and at threshold t a ground truth is taken by the first detection (in the class's order) that looks at it
// with an IoU > t. So: best ground truth per detection (parallel), an integer atomicMin of the detection's row per
// (threshold, ground truth), and d is a true positive at t iff its IoU passes and it is that minimum.
constexpr int kEvalMaxThr = 16;
// Lanes per detection in eval_best_kernel. The ground truths of one (image, class) are what the group walks: a handful
// (~4 in a two-class set with 8 objects per image, below 1 with 80 classes), so 8 lanes finish in one step and a wave holds
// 8 detections; a crowded image costs ceil(n / 8) steps.
constexpr int kEvalGroup = 8;
struct EvalThr { float v[kEvalMaxThr]; };

// best_iou[d] / best_gt[d]: the first maximum IoU (> 0) over the ground truths of d's image and class, as a row of gts, or 0 / -1
__global__ __launch_bounds__(256) void eval_best_kernel(const float* __restrict__ dets, int n_det, const float* __restrict__ gts,
                                                        const int* __restrict__ gt_off, int nc, int center,
                                                        float* __restrict__ best_iou, int* __restrict__ best_gt) {
    const long long gid = (blockIdx.x * 256LL + threadIdx.x) / kEvalGroup;
    const int sub = threadIdx.x % kEvalGroup;
    const bool live = gid < n_det;
    float best = 0.f;                                      // `best_iou = 0`, updated on strict `>`: this lane's first maximum
    int best_idx = -1;
    if (live) {
        const float* det = dets + (size_t)gid * 7;
        const float img = det[0];
        const int c = (int)det[6];
        int s = 0, e = 0;
        if (c >= 0 && c < nc) {
            const int g0 = gt_off[c], g1 = gt_off[c + 1];
            int lo = g0, hi = g1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (gts[(size_t)mid * 7] < img) lo = mid + 1; else hi = mid; }
            s = lo;
            hi = g1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (gts[(size_t)mid * 7] <= img) lo = mid + 1; else hi = mid; }
            e = lo;
        }
        for (int gi = s + sub; gi < e; gi += kEvalGroup) {
            const float v = iou_boxes(det + 1, gts + (size_t)gi * 7 + 1, center);
            if (v > best) { best = v; best_idx = gi; }
        }
    }
    // across the group: the largest IoU, the lowest row among equals (every lane of the wave takes part in the exchange)
#pragma unroll
    for (int sft = kEvalGroup / 2; sft > 0; sft >>= 1) {
        const float ov = __shfl_xor(best, sft);
        const int oi = __shfl_xor(best_idx, sft);
        if (ov > best || (ov == best && oi >= 0 && oi < best_idx)) { best = ov; best_idx = oi; }
    }
    if (live && sub == 0) { best_iou[gid] = best; best_gt[gid] = best_idx; }
}

// first[t][g] = the lowest detection row that looks at ground truth g with an IoU > thr[t] (integer min: any arrival order)
__global__ __launch_bounds__(256) void eval_claim_kernel(const float* __restrict__ best_iou, const int* __restrict__ best_gt, int n_det,
                                                         int n_gt, int n_thr, EvalThr thr, unsigned* __restrict__ first) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)n_det * n_thr) return;
    const int t = (int)(i / n_det), d = (int)(i % n_det);
    const int g = best_gt[d];
    if (g >= 0 && g < n_gt && best_iou[d] > thr.v[t]) atomicMin(first + (size_t)t * n_gt + g, (unsigned)d);
}

// one block per (class, threshold): the flags of the class at that threshold, then map_ap_kernel's integration of them (the same
// fp32 quotients, the same fp64 sums in the same order, so the same bits), and the counts above the confidence threshold
__global__ __launch_bounds__(256) void eval_ap_kernel(const float* __restrict__ dets, const int* __restrict__ det_off,
                                                      const int* __restrict__ gt_off, const float* __restrict__ best_iou,
                                                      const int* __restrict__ best_gt, const unsigned* __restrict__ first, int n_det, int n_gt,
                                                      int nc, EvalThr thr, float conf_thr, unsigned char* __restrict__ tp,
                                                      float* __restrict__ ap, int* __restrict__ tp_at_conf, int* __restrict__ n_det_at_conf) {
    __shared__ int s_wave[4];
    __shared__ int s_cnt[2][4];
    __shared__ double s_area[256];
    const int c = blockIdx.x, ti = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int d0 = det_off[c], d1 = det_off[c + 1];
    const int ng = gt_off[c + 1] - gt_off[c];
    const float thr_t = thr.v[ti];
    int carry = 0, hit_conf = 0, det_conf = 0;
    double area = 0.0;
    for (int base = d0; base < d1; base += 256) {
        const int d = base + t;
        int flag = 0;
        if (d < d1) {
            const int g = best_gt[d];
            flag = g >= 0 && g < n_gt && best_iou[d] > thr_t && first[(size_t)ti * n_gt + g] == (unsigned)d;
            tp[(size_t)ti * n_det + d] = (unsigned char)flag;
            const int above = dets[(size_t)d * 7 + 5] > conf_thr;
            det_conf += above;
            hit_conf += flag & above;
        }
        int incl = flag;                                   // inclusive scan of the flags: inside the wave, then across the four
        for (int sft = 1; sft < 64; sft <<= 1) {
            const int v = __shfl_up(incl, sft);
            if (lane >= sft) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) { const int v = s_wave[w]; before += w < wave ? v : 0; total += v; }
        const int itp = carry + before + incl;
        // cum_TP is a small integer: exact in fp32, as map_ap_kernel's running fp32 sum is
        const float ctp = (float)itp, ctp_prev = (float)(itp - flag);
        const float n_seen = (float)(d - d0 + 1);          // cum_TP + cum_FP
        const float p = ctp / n_seen, r = ctp / (float)ng;
        const float pp = d == d0 ? 1.f : ctp_prev / (n_seen - 1.f);       // the point (recall 0, precision 1) in front
        const float pr = d == d0 ? 0.f : ctp_prev / (float)ng;
        s_area[t] = d < d1 ? (double)((r - pr) * (p + pp)) : 0.0;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) s_area[t] += s_area[t + s];
            __syncthreads();
        }
        if (t == 0) area += s_area[0];
        carry += total;                                    // (the barriers of the sum separate this round's s_wave from the next)
    }
    for (int sft = 32; sft > 0; sft >>= 1) { hit_conf += __shfl_xor(hit_conf, sft); det_conf += __shfl_xor(det_conf, sft); }
    if (lane == 0) { s_cnt[0][wave] = hit_conf; s_cnt[1][wave] = det_conf; }
    __syncthreads();
    if (t == 0) {
        ap[(size_t)ti * nc + c] = ng == 0 ? -1.f : (float)(area / 2.0);
        tp_at_conf[(size_t)ti * nc + c] = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
        if (ti == 0) n_det_at_conf[c] = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
    }
}

// check_model_accuracy (utils.py:334-381) for one scale of one batch: five integer counters, accumulated with integer
// atomics (order-independent, so still deterministic): [class correct, n_obj, obj correct, noobj correct, n_noobj].
__global__ __launch_bounds__(256) void accuracy_kernel(const float* __restrict__ pred, long long sb, long long sa, long long sy, long long sx,
                                                       long long sk, const float* __restrict__ tgt, long long cells, int gh, int gw,
                                                       int nc, float thr, unsigned long long* __restrict__ counts) {
    unsigned c_cls = 0, c_nobj = 0, c_obj = 0, c_noobj = 0, c_nnoobj = 0;
    for (long long cell = blockIdx.x * 256LL + threadIdx.x; cell < cells; cell += (long long)gridDim.x * 256) {
        const float t4 = tgt[cell * 6 + 4];
        if (t4 != 1.f && t4 != 0.f) continue;
        const int x = (int)(cell % gw);
        const long long r1 = cell / gw;
        const int y = (int)(r1 % gh);
        const long long r2 = r1 / gh;
        const float* q = pred + (r2 / 3) * sb + (r2 % 3) * sa + y * sy + x * sx;
        const bool obj_pred = 1.f / (1.f + expf(-q[4 * sk])) > thr;
        if (t4 == 1.f) {
            int best = 0;
            float bv = q[5 * sk];
            for (int k = 1; k < nc; ++k) {                   // first maximum; NaN counts as maximum (torch.argmax)
                const float v = q[(5 + k) * sk];
                if (v > bv || (v != v && bv == bv)) { bv = v; best = k; }
            }
            c_cls += (float)best == tgt[cell * 6 + 5];
            c_nobj += 1;
            c_obj += obj_pred;
        } else {
            c_noobj += !obj_pred;
            c_nnoobj += 1;
        }
    }
    unsigned v[5] = {c_cls, c_nobj, c_obj, c_noobj, c_nnoobj};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        unsigned s = v[k];
        for (int sft = 32; sft > 0; sft >>= 1) s += __shfl_xor(s, sft);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(counts + k, (unsigned long long)s);
    }
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_map_match(const float* dets_sorted, const int32_t* det_class_offsets, const float* gts_sorted, const int32_t* gt_class_offsets,
                   int num_classes, int n_gt, float iou_threshold, int center, int32_t* assigned, float* tp_flags, float* ap_per_class,
                   void* stream) {
    if (!det_class_offsets || !gt_class_offsets || !ap_per_class || num_classes <= 0) return fail(YOLO_ERR_ARG, "map: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (n_gt > 0) {
        if (!assigned || !gts_sorted) return fail(YOLO_ERR_ARG, "map: null pointer");
        if (hipMemsetAsync(assigned, 0, sizeof(int32_t) * (size_t)n_gt, s) != hipSuccess) return fail(YOLO_ERR_LAUNCH, "map: memset");
    }
    hipLaunchKernelGGL(map_match_kernel, dim3(num_classes), dim3(64), 0, s, dets_sorted, det_class_offsets, gts_sorted, gt_class_offsets,
                       assigned, tp_flags, iou_threshold, center);
    int rc = check_launch("map_match");
    if (rc) return rc;
    hipLaunchKernelGGL(map_ap_kernel, dim3(num_classes), dim3(256), 0, s, tp_flags, det_class_offsets, gt_class_offsets, ap_per_class);
    return check_launch("map_ap");
}

size_t yolo_eval_workspace_bytes(int n_det, int n_gt, int n_thr) {
    if (n_det < 0 || n_gt < 0 || n_thr < 1 || n_thr > kEvalMaxThr) return 0;
    return (((size_t)n_thr * (size_t)(n_gt > 0 ? n_gt : 1) * sizeof(uint32_t)) + 15) & ~(size_t)15;       // first[n_thr][n_gt]
}

int yolo_eval_detections(const float* dets_sorted, const int32_t* det_class_offsets, int n_det, const float* gts_sorted,
                         const int32_t* gt_class_offsets, int n_gt, int num_classes, const float* iou_thresholds, int n_thr,
                         float conf_threshold, int center, float* best_iou, int32_t* best_gt, unsigned char* tp, float* ap,
                         int32_t* tp_at_conf, int32_t* n_det_at_conf, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_det < 0 || n_gt < 0 || num_classes <= 0 || n_thr < 1 || n_thr > kEvalMaxThr || (center != 0 && center != 1) ||
        conf_threshold != conf_threshold)
        return fail(YOLO_ERR_ARG, "eval_detections: need n_det, n_gt >= 0, num_classes >= 1, 1 <= n_thr <= %d, center 0 or 1 and a confidence "
                    "threshold that is a number (n_det %d, n_gt %d, num_classes %d, n_thr %d, center %d)", kEvalMaxThr, n_det, n_gt, num_classes,
                    n_thr, center);
    if (!det_class_offsets || !gt_class_offsets || !iou_thresholds || !ap || !tp_at_conf || !n_det_at_conf ||
        (n_det > 0 && (!dets_sorted || !best_iou || !best_gt || !tp)) || (n_gt > 0 && !gts_sorted))
        return fail(YOLO_ERR_ARG, "eval_detections: null pointer");
    EvalThr thr = {};
    for (int t = 0; t < n_thr; ++t) {
        thr.v[t] = iou_thresholds[t];
        if (!(thr.v[t] >= 0.f && thr.v[t] < 1.f)) return fail(YOLO_ERR_ARG, "eval_detections: threshold %d is %g, outside [0, 1)", t, (double)thr.v[t]);
    }
    const size_t need = yolo_eval_workspace_bytes(n_det, n_gt, n_thr);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3))
        return fail(YOLO_ERR_WORKSPACE, "eval_detections: workspace of %zu bytes (4-byte aligned) needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    hipStream_t s = (hipStream_t)stream;
    unsigned* first = static_cast<unsigned*>(workspace);
    int rc;
    if (n_det > 0) {
        if (n_gt > 0 && hipMemsetAsync(first, 0xff, sizeof(uint32_t) * (size_t)n_thr * n_gt, s) != hipSuccess)
            return fail(YOLO_ERR_LAUNCH, "eval_detections: memset");
        const long long lanes = (long long)n_det * kEvalGroup, claims = (long long)n_det * n_thr;
        hipLaunchKernelGGL(eval_best_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, dets_sorted, n_det, gts_sorted, gt_class_offsets,
                           num_classes, center, best_iou, best_gt);
        if ((rc = check_launch("eval_best"))) return rc;
        hipLaunchKernelGGL(eval_claim_kernel, dim3((unsigned)((claims + 255) / 256)), dim3(256), 0, s, best_iou, best_gt, n_det, n_gt, n_thr, thr,
                           first);
        if ((rc = check_launch("eval_claim"))) return rc;
    }
    hipLaunchKernelGGL(eval_ap_kernel, dim3(num_classes, n_thr), dim3(256), 0, s, dets_sorted, det_class_offsets, gt_class_offsets, best_iou, best_gt,
                       first, n_det, n_gt, num_classes, thr, conf_threshold, tp, ap, tp_at_conf, n_det_at_conf);
    return check_launch("eval_ap");
}

int yolo_accuracy_counts(const float* pred, const int64_t* strides5, const float* target, int b, int g, int nc, float obj_threshold,
                         unsigned long long* counts5, void* stream) {
    return yolo_accuracy_counts_hw(pred, strides5, target, b, g, g, nc, obj_threshold, counts5, stream);
}

int yolo_accuracy_counts_hw(const float* pred, const int64_t* strides5, const float* target, int b, int gh, int gw, int nc,
                            float obj_threshold, unsigned long long* counts5, void* stream) {
    if (!pred || !strides5 || !target || !counts5 || b <= 0 || gh <= 0 || gw <= 0 || nc <= 0)
        return fail(YOLO_ERR_ARG, "accuracy: bad arguments");
    const long long cells = (long long)b * 3 * gh * gw;
    long long nb = (cells + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(accuracy_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, pred, (long long)strides5[0],
                       (long long)strides5[1], (long long)strides5[2], (long long)strides5[3], (long long)strides5[4], target, cells, gh, gw, nc,
                       obj_threshold, counts5);
    return check_launch("accuracy");
}

}  // extern "C"
