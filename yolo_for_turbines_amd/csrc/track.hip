// track.hip — multi-object tracking: per stream a table of Kalman-filtered tracks, associated with each frame's detections by IoU
// in three greedy matchings (ByteTrack's high / low / tentative passes).   BUILD WITH -ffp-contract=off.
//
// Nothing of the reference: the arithmetic and the order of a call are defined in include/yolo_mi355x.h (and DESIGN.md 7.23), fp32
// with one rounding per operation, and tests/track_ref.py restates them in numpy.
//
//   launch    ONE launch per call, one workgroup of TRK_THREADS per stream, nothing read back: the call can sit in a graph.
//   slots     thread k owns slot k: its 26 words are loaded into registers, predicted, updated or founded there and stored once.
//             What the other threads need of a slot (the predicted corners, area, class) is in LDS, compacted per matching.
//   matching  the greedy walk of the contract without a sort: repeat "take all mutually-best pairs among the unmatched" until no
//             eligible pair is left. The threads stride over the detections (global memory, L2-resident); each walks the records
//             of the matching's slots in LDS (every lane reads the same address: a broadcast), keeps its detection's best and offers
//             (orderable IoU << 32 | ~detection) to the slot's 64-bit LDS maximum. A pair is mutual when the slot's maximum names
//             the detection. Largest IoU first, ties to the lowest index on either side; the globally best pair is always mutual,
//             so a matching of S slots and D detections ends after at most min(S, D) + 1 rounds. The IEEE division is skipped
//             for a pair that does not intersect (IoU exactly 0 never passes a threshold >= 0). A round costs S x D box
//             intersections on one CU (about 63 us at 512 x 512), whatever the LDS reads do: reading the records eight at a
//             time ahead of their use measured the same (profiles/track/README.md).
//   founding  ordered without a serial walk: block prefix counts rank the free slots and the founding detections; founder r
//             takes the r-th free slot and id next_id + r.
//   outputs   rank by counting: a listed slot's row is the number of listed slots with a smaller id.
// Workspace, per stream: det_slot[n] (slot + 1 that detection index j updated or founded, 0 none) and det_best[n] (the position of the slot a
// detection prefers in the running round, -2 once it has no eligible slot left in the matching: the slots only get fewer); entry j is only ever touched by thread j % TRK_THREADS.
#include "nms.h"

namespace yolo {

constexpr int TRK_THREADS = 512;         // threads per stream = the most slots
constexpr int TRK_WAVES = TRK_THREADS / 64;
constexpr int TRK_MAX_B = 2047;
constexpr int TRK_MAX_N = 163456;        // the n up to which yolo_nms and yolo_fuse_boxes deliver detections
constexpr int TRK_HDR = 4;               // words per stream: frame, next_id, overflow, 0
constexpr int TRK_SLOT = 26;             // words per slot (the header has the layout)
enum { TRK_FREE = 0, TRK_TENTATIVE = 1, TRK_TRACKED = 2, TRK_LOST = 3 };
constexpr float TRK_WP = 0.05f, TRK_WV = 0.00625f;

__device__ __forceinline__ unsigned trk_orderable(float f) {      // ascending-orderable bits, -0 as +0
    const unsigned u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix count of `flag` over the workgroup in thread order; total = the count. Two barriers.
__device__ __forceinline__ int trk_scan(bool flag, int* wave_count, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    __syncthreads();                                              // wave_count is free again
    if (lane == 0) wave_count[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < TRK_WAVES; ++w) {
        const int c = wave_count[w];
        before += w < wave ? c : 0;
        total += c;
    }
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void track_reset_kernel(int* __restrict__ state, int m, const unsigned char* __restrict__ mask) {
    const int s = blockIdx.x;
    if (mask && !mask[s]) return;
    const int words = TRK_HDR + TRK_SLOT * m;
    int* w = state + (size_t)s * words;
    for (int i = threadIdx.x; i < words; i += 256) w[i] = i == 1 ? 1 : 0;
}

// grid (b), TRK_THREADS threads
__global__ __launch_bounds__(TRK_THREADS) void track_update_kernel(int* __restrict__ state, int m, const float* __restrict__ boxes, int n,
                                                                   const int* __restrict__ keep_idx, const int* __restrict__ keep_count,
                                                                   yolo_track_params p, float* __restrict__ out_boxes,
                                                                   int* __restrict__ out_ids, int* __restrict__ out_count,
                                                                   int* __restrict__ det_ids, int* __restrict__ ws) {
    __shared__ unsigned long long sBest[TRK_THREADS];             // a slot's best offer of the round
    __shared__ float4 cBox[TRK_THREADS];                          // the running matching's slots, compacted in slot order: corners,
    __shared__ float cArea[TRK_THREADS], cCls[TRK_THREADS];       // area and class (a matched one gets x2 = -inf: it intersects nothing)
    __shared__ int cSlot[TRK_THREADS];                            // ... and the slot each of them is
    __shared__ int sMatch[TRK_THREADS];                           // detection index + 1 the slot was matched with
    __shared__ int sFree[TRK_THREADS];                            // the free slots in ascending order
    __shared__ int sFound[TRK_THREADS], sFoundId[TRK_THREADS];    // detection index + 1 that founds a track in the slot, and its id
    __shared__ int sId[TRK_THREADS], sState[TRK_THREADS], sOut[TRK_THREADS];
    __shared__ int sWave[TRK_WAVES];
    __shared__ int sHdr[3];

    const int s = blockIdx.x, k = threadIdx.x;
    const bool mine = k < m;
    int* hdr = state + (size_t)s * (TRK_HDR + TRK_SLOT * m);
    int* slot = hdr + TRK_HDR + TRK_SLOT * (mine ? k : 0);
    const float* bx = boxes + (size_t)s * n * 6;
    const int* kp = keep_idx ? keep_idx + (size_t)s * n : nullptr;
    int cnt = keep_count ? keep_count[s] : n;
    cnt = cnt < 0 ? 0 : cnt > n ? n : cnt;
    int* det_slot = ws + (size_t)s * 2 * n;
    int* det_best = det_slot + n;
    int* dids = det_ids + (size_t)s * n;
    const int center = p.center, agnostic = p.class_agnostic;

    if (k < 3) sHdr[k] = hdr[k];
    for (int j = k; j < n; j += TRK_THREADS) dids[j] = 0;
    for (int j = k; j < cnt; j += TRK_THREADS) det_slot[j] = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the zeros of det_ids are in place before another thread's id can follow

    // ---- the thread's slot, predicted
    int st = TRK_FREE, id = 0, lost = 0;
    float cls = 0.f, score = 0.f, mu[8], P[12];
#pragma unroll
    for (int i = 0; i < 8; ++i) mu[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = 0.f;
    if (mine) {
        st = slot[0]; id = slot[1]; cls = __int_as_float(slot[2]); score = __int_as_float(slot[3]); lost = slot[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) mu[i] = __int_as_float(slot[5 + i]);
#pragma unroll
        for (int i = 0; i < 12; ++i) P[i] = __int_as_float(slot[13 + i]);
    }
    const int st0 = st;
    if (st != TRK_FREE) {
        if (st == TRK_LOST) { mu[6] = 0.f; mu[7] = 0.f; }
        const float sw = mu[2], sh = mu[3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float sc = (c & 1) ? sh : sw;
            const float a = TRK_WP * sc, qp = a * a, b = TRK_WV * sc, qv = b * b;
            const float P00 = P[3 * c], P01 = P[3 * c + 1], P11 = P[3 * c + 2];
            mu[c] = mu[c] + mu[4 + c];
            P[3 * c] = ((P00 + 2.0f * P01) + P11) + qp;
            P[3 * c + 1] = P01 + P11;
            P[3 * c + 2] = P11 + qv;
        }
    }
    const float px1 = mu[0] - mu[2] / 2.0f, py1 = mu[1] - mu[3] / 2.0f;      // the predicted box, the NMS's corners
    const float4 pbox = make_float4(px1, py1, px1 + mu[2], py1 + mu[3]);
    const float parea = mu[2] * mu[3];
    sMatch[k] = 0;

    // ---- the three matchings
    for (int stage = 0; stage < 3; ++stage) {
        const bool part = stage == 0 ? (st0 == TRK_TRACKED || st0 == TRK_LOST) : stage == 1 ? st0 == TRK_TRACKED : st0 == TRK_TENTATIVE;
        const float thr = (float)p.match_iou[stage];
        const bool want_low = stage == 1;
        __syncthreads();                                          // the matches of the stage before
        const bool act = mine && part && sMatch[k] == 0;
        int nact;
        const int pos = trk_scan(act, sWave, nact);
        if (nact == 0) continue;
        if (act) { cBox[pos] = pbox; cArea[pos] = parea; cCls[pos] = cls; cSlot[pos] = k; }
        for (int j = k; j < cnt; j += TRK_THREADS) det_best[j] = -1;
        for (int round = 0; round <= nact; ++round) {
            sBest[k] = 0ull;
            __syncthreads();
            bool any = false;
            for (int j = k; j < cnt; j += TRK_THREADS) {
                if (det_best[j] == -2) continue;                  // nothing for this detection in this matching any more
                int bs = -2;
                const int row = kp ? kp[j] : j;
                if (det_slot[j] == 0 && (unsigned)row < (unsigned)n) {
                    const float* r = bx + (size_t)row * 6;
                    const double obj = (double)r[4];
                    const bool high = obj > p.high_threshold, low = obj > p.low_threshold && obj <= p.high_threshold;
                    if (want_low ? low : high) {
                        const SBox d = make_sbox(r, center);
                        unsigned long long best = 0ull;           // (orderable IoU << 32) | ~position; 0 = no eligible slot
#pragma unroll 4
                        for (int t = 0; t < nact; ++t) {
                            const float4 sb = cBox[t];
                            const float xa = fmaxf(d.x1, sb.x), ya = fmaxf(d.y1, sb.y), xb = fminf(d.x2, sb.z), yb = fminf(d.y2, sb.w);
                            const float inter = fmaxf(xb - xa, 0.f) * fmaxf(yb - ya, 0.f);
                            if (inter > 0.f && (agnostic || cCls[t] == d.cls)) {
                                const float iou = inter / (((d.area + cArea[t]) - inter) + 1e-6f);
                                if (iou > thr) {
                                    const unsigned long long hi = (unsigned long long)trk_orderable(iou) << 32;
                                    const unsigned long long key = hi | (0xffffffffu - (unsigned)t);
                                    best = key > best ? key : best;
                                    atomicMax(&sBest[t], hi | (0xffffffffu - (unsigned)j));
                                }
                            }
                        }
                        if (best) bs = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
                    }
                }
                det_best[j] = bs;
                any = any || bs >= 0;
            }
            if (!__syncthreads_or(any)) break;
            for (int j = k; j < cnt; j += TRK_THREADS) {
                const int bs = det_best[j];
                if (bs >= 0 && (unsigned)(sBest[bs] & 0xffffffffull) == 0xffffffffu - (unsigned)j) {   // mutual
                    const int sl = cSlot[bs];
                    det_slot[j] = sl + 1;
                    sMatch[sl] = j + 1;
                    cBox[bs].z = -INFINITY;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- steps 4 to 6 on the thread's slot
    bool listed = false;
    auto release = [&]() {
        st = TRK_FREE; id = 0; lost = 0; cls = 0.f; score = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) mu[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) P[i] = 0.f;
    };
    if (mine && st0 != TRK_FREE) {
        const int md = sMatch[k];
        if (md) {
            const int row = kp ? kp[md - 1] : md - 1;
            const float* r = bx + (size_t)row * 6;
            float z[4] = {r[0], r[1], r[2], r[3]};
            if (!center) { z[0] = z[0] + z[2] / 2.0f; z[1] = z[1] + z[3] / 2.0f; }
            const float sw = mu[2], sh = mu[3];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float sc = (c & 1) ? sh : sw;
                const float a = TRK_WP * sc, rr = a * a;
                const float P00 = P[3 * c], P01 = P[3 * c + 1], P11 = P[3 * c + 2];
                const float S = P00 + rr, K0 = P00 / S, K1 = P01 / S, y = z[c] - mu[c];
                mu[c] = mu[c] + K0 * y;
                mu[4 + c] = mu[4 + c] + K1 * y;
                P[3 * c] = P00 - K0 * P00;
                P[3 * c + 1] = P01 - K0 * P01;
                P[3 * c + 2] = P11 - K1 * P01;
            }
            st = TRK_TRACKED; score = r[4]; lost = 0;
            listed = true;
        } else if (st0 == TRK_TENTATIVE) {
            release();
        } else {
            st = TRK_LOST;
            lost += 1;
            if (lost > p.max_age) release();
        }
    }

    // ---- step 7: founder r of the call takes the r-th free slot
    const int frame = sHdr[0], next_id = sHdr[1];
    const bool is_free = mine && st == TRK_FREE;
    int nfree;
    const int frank = trk_scan(is_free, sWave, nfree);
    if (is_free) sFree[frank] = k;
    sFound[k] = 0;
    __syncthreads();
    int founders = 0;
    for (int base = 0; base < cnt; base += TRK_THREADS) {
        const int j = base + k;
        bool founds = false;
        if (j < cnt && det_slot[j] == 0) {
            const int row = kp ? kp[j] : j;
            if ((unsigned)row < (unsigned)n) {
                const double obj = (double)bx[(size_t)row * 6 + 4];
                founds = obj > p.high_threshold && obj > p.new_threshold;
            }
        }
        int total;
        const int r = founders + trk_scan(founds, sWave, total);
        if (founds && r < nfree) {
            const int sl = sFree[r];
            sFound[sl] = j + 1;
            sFoundId[sl] = next_id + r;
            det_slot[j] = sl + 1;
        }
        founders += total;
    }
    __syncthreads();
    if (is_free && sFound[k]) {
        const int j = sFound[k] - 1;
        const int row = kp ? kp[j] : j;
        const float* r = bx + (size_t)row * 6;
        float z[4] = {r[0], r[1], r[2], r[3]};
        if (!center) { z[0] = z[0] + z[2] / 2.0f; z[1] = z[1] + z[3] / 2.0f; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float sc = (c & 1) ? z[3] : z[2];
            const float t = (2.0f * TRK_WP) * sc, u = (10.0f * TRK_WV) * sc;
            mu[c] = z[c];
            mu[4 + c] = 0.f;
            P[3 * c] = t * t;
            P[3 * c + 1] = 0.f;
            P[3 * c + 2] = u * u;
        }
        id = sFoundId[k]; cls = r[5]; score = r[4]; lost = 0;
        st = frame == 0 ? TRK_TRACKED : TRK_TENTATIVE;
        listed = st == TRK_TRACKED;
    }
    if (mine) {
        slot[0] = st; slot[1] = id; slot[2] = __float_as_int(cls); slot[3] = __float_as_int(score); slot[4] = lost;
#pragma unroll
        for (int i = 0; i < 8; ++i) slot[5 + i] = __float_as_int(mu[i]);
#pragma unroll
        for (int i = 0; i < 12; ++i) slot[13 + i] = __float_as_int(P[i]);
        slot[25] = 0;
    }
    if (k == 0) {
        const int took = founders < nfree ? founders : nfree;
        hdr[0] = frame + 1;
        hdr[1] = next_id + took;
        hdr[2] = sHdr[2] + (founders - took);
        hdr[3] = 0;
    }

    // ---- outputs
    sId[k] = id; sState[k] = st; sOut[k] = listed ? id : 0;
    __syncthreads();
    int rank = 0, nlisted = 0;
    for (int t = 0; t < m; ++t) {
        const int o = sOut[t];
        nlisted += o != 0;
        rank += o != 0 && o < id;
    }
    if (mine) {
        float* ob = out_boxes + (size_t)s * m * 6;
        int* oi = out_ids + (size_t)s * m;
        if (listed) {
            float* o = ob + (size_t)rank * 6;
            o[0] = center ? mu[0] : mu[0] - mu[2] / 2.0f;
            o[1] = center ? mu[1] : mu[1] - mu[3] / 2.0f;
            o[2] = mu[2]; o[3] = mu[3]; o[4] = score; o[5] = cls;
            oi[rank] = id;
        }
        if (k >= nlisted) {
            float* o = ob + (size_t)k * 6;
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] = 0.f;
            oi[k] = 0;
        }
    }
    if (k == 0) out_count[s] = nlisted;
    for (int j = k; j < cnt; j += TRK_THREADS) {
        const int sl = det_slot[j];
        if (sl) {
            const int row = kp ? kp[j] : j;                      // in [0, n): only such a detection is ever matched or founds
            dids[row] = sState[sl - 1] == TRK_TENTATIVE ? -sId[sl - 1] : sId[sl - 1];
        }
    }
}

static bool track_dims_ok(int b, int max_tracks) { return b >= 1 && b <= TRK_MAX_B && max_tracks >= 1 && max_tracks <= TRK_THREADS; }

}  // namespace yolo

using namespace yolo;

extern "C" {

size_t yolo_track_state_bytes(int b, int max_tracks) {
    if (!track_dims_ok(b, max_tracks)) return 0;
    return sizeof(int) * (size_t)b * (TRK_HDR + TRK_SLOT * (size_t)max_tracks);
}

size_t yolo_track_workspace_bytes(int b, int n, int max_tracks) {
    if (!track_dims_ok(b, max_tracks) || n < 0 || n > TRK_MAX_N) return 0;
    return sizeof(int) * 2 * (size_t)b * (size_t)n;
}

int yolo_track_reset(void* state, int b, int max_tracks, const uint8_t* stream_mask_dev, void* stream) {
    if (!track_dims_ok(b, max_tracks))
        return fail(YOLO_ERR_UNSUPPORTED, "track_reset: b = %d (1 .. %d) or max_tracks = %d (1 .. %d) outside the limits", b, TRK_MAX_B, max_tracks,
                    TRK_THREADS);
    if (!state || ((uintptr_t)state & 3)) return fail(YOLO_ERR_ARG, "track_reset: state missing or not 4-byte aligned");
    hipLaunchKernelGGL(track_reset_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, (int*)state, max_tracks, stream_mask_dev);
    return check_launch("track reset");
}

int yolo_track_update(void* state, int b, int max_tracks, const float* boxes, int n, const int32_t* keep_idx, const int32_t* keep_count,
                      const yolo_track_params* p, float* out_boxes, int32_t* out_ids, int32_t* out_count, int32_t* det_ids, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!track_dims_ok(b, max_tracks) || n < 0 || n > TRK_MAX_N)
        return fail(YOLO_ERR_UNSUPPORTED, "track_update: b = %d (1 .. %d), max_tracks = %d (1 .. %d) or n = %d (0 .. %d) outside the limits", b,
                    TRK_MAX_B, max_tracks, TRK_THREADS, n, TRK_MAX_N);
    if (!state || ((uintptr_t)state & 3) || !p || !out_boxes || !out_ids || !out_count || (n > 0 && (!boxes || !det_ids)))
        return fail(YOLO_ERR_ARG, "track_update: null pointer or a state that is not 4-byte aligned");
    if (keep_idx && !keep_count) return fail(YOLO_ERR_ARG, "track_update: keep_idx without keep_count");
    if (p->high_threshold != p->high_threshold || p->low_threshold != p->low_threshold || p->new_threshold != p->new_threshold)
        return fail(YOLO_ERR_ARG, "track_update: a NaN threshold");
    for (int i = 0; i < 3; ++i)
        if (!(p->match_iou[i] >= 0.0 && p->match_iou[i] <= 1.0)) return fail(YOLO_ERR_ARG, "track_update: match_iou[%d] outside [0, 1]", i);
    if (p->max_age < 0) return fail(YOLO_ERR_ARG, "track_update: max_age %d < 0", p->max_age);
    const size_t need = sizeof(int) * 2 * (size_t)b * (size_t)n;
    if (need && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < need))
        return fail(YOLO_ERR_WORKSPACE, "track_update: workspace missing, not 4-byte aligned or %zu < %zu bytes", workspace_bytes, need);
    hipLaunchKernelGGL(track_update_kernel, dim3(b), dim3(TRK_THREADS), 0, (hipStream_t)stream, (int*)state, max_tracks, boxes, n, keep_idx,
                       keep_count, *p, out_boxes, out_ids, out_count, det_ids, (int*)workspace);
    return check_launch("track update");
}

}  // extern "C"
