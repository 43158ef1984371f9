// nms_soft.hip — Soft-NMS (Bodla et al. 2017): the best box of a walk lowers the scores of the boxes it overlaps instead of removing
// them; hard removal, class-agnostic suppression, a cap on detections and a final score threshold ride on the same walk.
// BUILD WITH -ffp-contract=off.
//
// Nothing of the reference: the arithmetic is defined in include/yolo_mi355x.h (DESIGN.md 7.24 has it step by step), fp32 with one
// rounding per operation, and tests/soft_nms_ref.py restates it in numpy - the weight w(t) ~ exp(-t) of the Gaussian method included,
// which is a fixed sequence of fp32 operations and not the library's expf. Every pick changes the scores the next pick is made
// from, so the walk is sequential by definition and cannot go through the NMS mask / scan kernels.
//
//   order     nms_order_class_sorted (nms_order.hip): the candidates' score order (order 1) and the class-major rows (order 2) with
//             their records; nms_class_segments: the bounds of every class bucket's run
//   segments  scores only fall and rows of different classes never interact, so every run of one class bucket in order 2 is an
//             independent walk whose emissions come out in (score descending, row ascending) order; class-agnostic: one walk per
//             image over order 1. The lump bucket 4094 holds several classes: the walk compares the classes themselves.
//   walk      ONE WORKGROUP of SOFT_THREADS per segment. Position p of the segment belongs to thread p % SOFT_THREADS for the whole
//             walk; its corners, area, class and input row are written once, its current score is read and written by its owner
//             only. The first SOFT_ONCHIP positions live on chip: the record in LDS (28 bytes each: 112 KiB of a CU's 160, one
//             workgroup per CU - a walk is one serial chain, a second workgroup would not shorten it, and the segments of a
//             2-class dataset are few and long), the score in a register of the owner (eight rows per thread); the others in the
//             workspace, loaded four per thread at a time. One iteration: every thread brings the largest
//             (score, -row) key of its live rows - found while it decayed them - a wave maximum by DPP steps (no LDS round trip), one LDS slot
//             per wave, ONE barrier (the slots are double-buffered), every thread takes the maximum of the eight slots, reads the
//             winner's record (a broadcast read) and decays its own live rows. A row whose score no longer passes score_threshold
//             can never be emitted: it is dead (score -inf) and costs a compare. The IEEE division is skipped for a row the winner
//             does not intersect (its IoU is exactly 0 over a positive denominator).
//   merge     the emissions of an image by (score descending, row ascending): a counting rank over their unique 64-bit keys, which
//             IS the output position; the same launch applies max_det and writes keep_idx, scores, keep_count and rescore_rows.
// Everything is stream-ordered; the outputs are fully written by the call (memsets + scatters).
#include "nms.h"
#include <climits>
#include <cmath>

namespace yolo {

constexpr int SOFT_THREADS = 512;        // eight waves: two per SIMD
constexpr int SOFT_WAVES = SOFT_THREADS / 64;
constexpr int SOFT_SLOTS = 8;            // on-chip rows per thread: their current scores are in its registers
constexpr int SOFT_ONCHIP = SOFT_SLOTS * SOFT_THREADS;   // rows of one segment held on chip: 28 bytes of LDS each, 112 KiB of the 160 KiB of a CU
constexpr int SOFT_BATCH = 4;            // spilled rows a thread loads at once
constexpr int SOFT_BUCKETS = CLASS_BUCKETS;
constexpr int SOFT_WGS = 128;            // walk workgroups per image (class-aware): workgroup x takes buckets x, x + 128, ...
constexpr int SOFT_MAX_N = 163456;       // the n up to which yolo_nms orders class-sorted (nms_host.hip)
constexpr size_t SOFT_LDS = (size_t)SOFT_ONCHIP * 28 + sizeof(uint4) * 2 * SOFT_WAVES;
static_assert(SOFT_LDS <= 160 * 1024, "one workgroup's rows and exchange slots fit the LDS of a CU");
static_assert(SOFT_MAX_N <= SC * 80 && SOFT_MAX_N < (1 << 20), "the ordering's chunk count and the 20-bit index fields");

// bare v_max / v_min: fmaxf() makes the compiler canonicalise both operands first (nms_mask.hip)
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

__device__ __forceinline__ unsigned orderable(float f) {          // ascending-orderable bits, -0 as +0
    const unsigned u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// maximum over the 64 lanes (all active), result wave-uniform: four DPP steps inside the rows of 16, then the four rows (nms_scan.hip)
__device__ __forceinline__ unsigned wave_max32(unsigned v) {
    unsigned o;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true); v = o > v ? o : v;      // quad_perm [1,0,3,2]
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true); v = o > v ? o : v;      // quad_perm [2,3,0,1]
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true); v = o > v ? o : v;     // row_half_mirror
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true); v = o > v ? o : v;     // row_mirror: every lane holds its row's maximum
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// w(t) of the header, operation by operation: every product and sum below is rounded once (no contraction in this unit)
__device__ __forceinline__ float soft_w(float t) {
    if (t != t) return t;
    const float kf = rintf(t * 0x1.715476p+0f);                   // round half to even
    if (!(kf <= 125.0f)) return 0.0f;
    const float r = (t - kf * 0x1.63p-1f) - kf * -0x1.bd0106p-13f;
    float p = -0x1.a01a02p-13f;
    p = p * r + 0x1.6c16c2p-10f;
    p = p * r + -0x1.111112p-7f;
    p = p * r + 0x1.555556p-5f;
    p = p * r + -0x1.555556p-3f;
    p = p * r + 0x1p-1f;
    p = p * r + -0x1p+0f;
    p = p * r + 1.0f;
    return __uint_as_float(__float_as_uint(p) - ((unsigned)(int)kf << 23));
}

// the rows of one image in the workspace: the spill of the walk (position = segment start + p)
struct SoftSpill { float4* box; float4* meta; };                  // meta = {area, class, current score, input row as bits}

constexpr unsigned SOFT_DEAD = 0xff800000u;                      // -inf: a live score passes a finite threshold, so it is never this

// grid (SOFT_WGS or 1, B), SOFT_THREADS threads, SOFT_LDS bytes of dynamic LDS
__global__ __launch_bounds__(SOFT_THREADS) void soft_walk_kernel(const float* __restrict__ boxes, const unsigned long long* __restrict__ order,
                                                                 const SBox* __restrict__ sbox,
                                                                 const int* __restrict__ seg, int n, int center, int agnostic, int method, float thr,
                                                                 float sigma, double score_thr, int cap, SoftSpill sp,
                                                                 unsigned long long* __restrict__ em_key, float* __restrict__ em_score) {
    extern __shared__ __align__(16) unsigned char soft_lds[];
    float4* sBox = reinterpret_cast<float4*>(soft_lds);
    float2* sAC = reinterpret_cast<float2*>(sBox + SOFT_ONCHIP);                  // area, class
    int* sRow = reinterpret_cast<int*>(sAC + SOFT_ONCHIP);
    uint4* slots = reinterpret_cast<uint4*>(sRow + SOFT_ONCHIP);                   // [2][SOFT_WAVES]: key lo, key hi, position, score
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t img = (size_t)b * n;
    const float* bx = boxes + img * 6;
    const int nbuckets = agnostic ? 1 : SOFT_BUCKETS;
    const bool zero_removes = !(0.f < thr);                       // method 0: iou == +-0 for a row the winner does not intersect

    for (int mb = blockIdx.x; mb < nbuckets; mb += gridDim.x) {
        const int2 se = *reinterpret_cast<const int2*>(seg + ((size_t)b * SOFT_BUCKETS + mb) * 2);
        const int s0 = se.x, len = se.y - se.x;
        if (len <= 0) continue;                                   // uniform: every thread of the workgroup reads the same bounds
        const int lds_len = len < SOFT_ONCHIP ? len : SOFT_ONCHIP;
        float4* gBox = sp.box + img + s0;                         // position p >= SOFT_ONCHIP of this segment: index p (p < len)
        float4* gMeta = sp.meta + img + s0;
        __syncthreads();                                          // the walk before this one has left the LDS

        unsigned long long best = 0ull;                           // (orderable score << 32) | ~row of this thread's best live row; 0: none
        int bpos = 0;
        float bs = 0.f;
        int spill_live = 0;
        auto consider = [&](float s, int row, int p) {
            const unsigned long long key = ((unsigned long long)orderable(s) << 32) | (0xffffffffu - (unsigned)row);
            if (key > best) { best = key; bpos = p; bs = s; }
        };
        float sc[SOFT_SLOTS];                                     // current score of on-chip position tid + k * SOFT_THREADS (dead beyond the segment)
        auto fetch = [&](int p, SBox& sb, int& i) {              // the record and the starting score of position p
            const unsigned long long key = order[img + s0 + p];
            i = agnostic ? (int)(unsigned)(key & 0xffffffffull) : (int)(unsigned)(key & 0xfffffull);
            const float* row = bx + (size_t)i * 6;
            if (agnostic) sb = make_sbox(row, center);            // order 1 has no records; order 2's are the ordering stage's, the same bits
            else sb = sbox[img + s0 + p];
            const float s = row[4] + 0.0f;
            return (double)s > score_thr ? s : __uint_as_float(SOFT_DEAD);
        };
#pragma unroll
        for (int k = 0; k < SOFT_SLOTS; ++k) {
            const int p = tid + k * SOFT_THREADS;
            sc[k] = __uint_as_float(SOFT_DEAD);
            if (p < lds_len) {
                SBox sb;
                int i;
                sc[k] = fetch(p, sb, i);
                sBox[p] = make_float4(sb.x1, sb.y1, sb.x2, sb.y2);
                sAC[p] = make_float2(sb.area, sb.cls);
                sRow[p] = i;
                if (__float_as_uint(sc[k]) != SOFT_DEAD) consider(sc[k], i, p);
            }
        }
        for (int p = SOFT_ONCHIP + tid; p < len; p += SOFT_THREADS) {
            SBox sb;
            int i;
            const float s = fetch(p, sb, i);
            gBox[p] = make_float4(sb.x1, sb.y1, sb.x2, sb.y2);
            gMeta[p] = make_float4(sb.area, sb.cls, s, __int_as_float(i));
            if (__float_as_uint(s) != SOFT_DEAD) { ++spill_live; consider(s, i, p); }
        }
        __syncthreads();                                          // the records (LDS and spill) are visible to the workgroup

        int emitted = 0, par = 0;
        for (;;) {
            // wave maximum of the 64-bit keys in two 32-bit halves: the largest score, then the largest ~row among the lanes that hold it
            const unsigned hmax = wave_max32((unsigned)(best >> 32));
            const unsigned lmax = wave_max32((unsigned)(best >> 32) == hmax ? (unsigned)(best & 0xffffffffull) : 0u);
            const unsigned long long m = ((unsigned long long)hmax << 32) | lmax;
            const int src = __builtin_ctzll(__ballot(best == m));
            const int wp = __builtin_amdgcn_readlane(bpos, src);
            const unsigned wsb = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(bs), src);
            if (lane == 0) slots[par * SOFT_WAVES + wave] = make_uint4((unsigned)(m & 0xffffffffull), (unsigned)(m >> 32), (unsigned)wp, wsb);
            __syncthreads();                                      // the one barrier of an iteration
            unsigned long long M = 0ull;
            int P = 0;
            unsigned Sb = 0u;
#pragma unroll
            for (int w = 0; w < SOFT_WAVES; ++w) {
                const uint4 v = slots[par * SOFT_WAVES + w];
                const unsigned long long k = ((unsigned long long)v.y << 32) | v.x;
                if (k > M) { M = k; P = (int)v.z; Sb = v.w; }
            }
            par ^= 1;
            if (M == 0ull || emitted == cap) break;               // no live row is left, or max_det rows of this segment are out
            if (tid == 0) {
                const unsigned row = 0xffffffffu - (unsigned)(M & 0xffffffffull);
                em_key[img + s0 + emitted] = ((unsigned long long)(~(unsigned)(M >> 32)) << 32) | row;
                em_score[img + s0 + emitted] = __uint_as_float(Sb);
            }
            ++emitted;
            float4 wb;
            float wa, wc;
            if (P < SOFT_ONCHIP) {
                wb = sBox[P];
                const float2 ac = sAC[P];
                wa = ac.x; wc = ac.y;
            } else {
                wb = gBox[P];
                const float4 mt = gMeta[P];
                wa = mt.x; wc = mt.y;
            }

            // the winner's effect on one live row: its new score, SOFT_DEAD bits when it leaves the live set
            auto decay = [&](float s, const float4 bb, float a, float c) -> float {
                if (!(agnostic || c == wc)) return s;
                const float xa = vmax(wb.x, bb.x), ya = vmax(wb.y, bb.y), xb = vmin(wb.z, bb.z), yb = vmin(wb.w, bb.w);
                const float inter = vmax(xb - xa, 0.f) * vmax(yb - ya, 0.f);
                const float den = ((wa + a) - inter) + 1e-6f;
                if (inter == 0.f && den > 0.f)                    // iou = +-0 exactly: linear and Gaussian leave the score as it is
                    return (method == 0 && zero_removes) ? __uint_as_float(SOFT_DEAD) : s;
                const float iou = inter / den;
                if (method == 0) return !(iou < thr) ? __uint_as_float(SOFT_DEAD) : s;
                if (method == 1) { if (iou > thr) s = s * (1.0f - iou); }
                else s = s * soft_w((iou * iou) / sigma);
                return (double)s > score_thr ? s : __uint_as_float(SOFT_DEAD);
            };

            best = 0ull;
#pragma unroll
            for (int k = 0; k < SOFT_SLOTS; ++k) {
                const int p = tid + k * SOFT_THREADS;             // < SOFT_ONCHIP: the loads need no guard, so they are issued ahead of the branches
                const float2 ac = sAC[p];
                const float4 bb = sBox[p];
                const int rw = sRow[p];
                if (__float_as_uint(sc[k]) == SOFT_DEAD) continue;
                if (p == P) { sc[k] = __uint_as_float(SOFT_DEAD); continue; }
                sc[k] = decay(sc[k], bb, ac.x, ac.y);
                if (__float_as_uint(sc[k]) != SOFT_DEAD) consider(sc[k], rw, p);
            }
            // the spilled rows, SOFT_BATCH at a time: their loads are issued together, so a batch costs one trip to memory, not one per row
            for (int p0 = SOFT_ONCHIP + tid; spill_live > 0 && p0 < len; p0 += SOFT_BATCH * SOFT_THREADS) {
                float4 mt[SOFT_BATCH], bb[SOFT_BATCH];
#pragma unroll
                for (int u = 0; u < SOFT_BATCH; ++u) {
                    const int p = p0 + u * SOFT_THREADS;
                    const int pc = p < len ? p : p0;              // past the segment: this thread's first row again, unused
                    mt[u] = gMeta[pc];
                    bb[u] = gBox[pc];
                }
#pragma unroll
                for (int u = 0; u < SOFT_BATCH; ++u) {
                    const int p = p0 + u * SOFT_THREADS;
                    if (p >= len || __float_as_uint(mt[u].z) == SOFT_DEAD) continue;
                    float s2 = __uint_as_float(SOFT_DEAD);
                    if (p != P) s2 = decay(mt[u].z, bb[u], mt[u].x, mt[u].y);
                    if (__float_as_uint(s2) != __float_as_uint(mt[u].z)) gMeta[p].z = s2;
                    if (__float_as_uint(s2) != SOFT_DEAD) consider(s2, __float_as_int(mt[u].w), p);
                    else --spill_live;
                }
            }
        }
    }
}

// ---- output positions. grid (ceil(n / 256), B): position = number of the image's emission keys that are smaller (they are unique:
// the input row is part of the key). em_key is ~0 where nothing was emitted; tiles of it without an emission cost one load and a
// barrier. An emission at a position >= cap (max_det) is dropped.
__global__ __launch_bounds__(256) void soft_merge_kernel(const unsigned long long* __restrict__ em_key, const float* __restrict__ em_score, int n,
                                                         int cap, int* __restrict__ keep_idx, int* __restrict__ keep_count,
                                                         float* __restrict__ scores, float* rescore) {
    __shared__ unsigned long long keys[256];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const size_t img = (size_t)b * n;
    const unsigned long long mine = i < n ? em_key[img + i] : ~0ull;
    if (!__syncthreads_or(mine != ~0ull)) return;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        const unsigned long long kj = j < n ? em_key[img + j] : ~0ull;
        __syncthreads();
        keys[threadIdx.x] = kj;
        if (!__syncthreads_or(kj != ~0ull)) continue;
        for (int t = 0; t < 256; ++t) rank += keys[t] < mine;
    }
    const bool valid = mine != ~0ull && rank < cap;
    if (valid) {
        const int row = (int)(unsigned)(mine & 0xffffffffull);
        const float s = em_score[img + i];
        keep_idx[img + rank] = row;
        scores[img + rank] = s;
        if (rescore) rescore[(img + row) * 6 + 4] = s;
    }
    const unsigned long long bal = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(keep_count + b, __popcll(bal));
}

struct SoftWs { int* nvalid; unsigned long long* row_any; int* chunk_valid; unsigned long long* chunked; unsigned long long* sorted1;
                unsigned long long* sorted2; int* grank; SBox* sbox; int* blk_lo; int* blk_hi; int* seg; SoftSpill sp;
                unsigned long long* em_key; float* em_score; size_t total; };

static SoftWs soft_carve(void* base, int b, int n) {
    const int W = ceil_div(n > 0 ? n : 1, 64);
    const size_t bn = (size_t)b * (n > 0 ? n : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return (char*)base + o; };
    SoftWs w;
    w.nvalid = (int*)take(sizeof(int) * (size_t)b);
    w.row_any = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * W);
    w.chunk_valid = (int*)take(sizeof(int) * (size_t)b * SC_MAXCH);
    w.chunked = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * ceil_div(n > 0 ? n : 1, SC) * SC);
    w.sorted1 = (unsigned long long*)take(sizeof(unsigned long long) * bn);
    w.sorted2 = (unsigned long long*)take(sizeof(unsigned long long) * bn);
    w.grank = (int*)take(sizeof(int) * bn);
    w.sbox = (SBox*)take(sizeof(SBox) * bn);
    w.blk_lo = (int*)take(sizeof(int) * (size_t)b * W);
    w.blk_hi = (int*)take(sizeof(int) * (size_t)b * W);
    w.seg = (int*)take(sizeof(int) * (size_t)b * SOFT_BUCKETS * 2);
    w.sp.box = (float4*)take(sizeof(float4) * bn);
    w.sp.meta = (float4*)take(sizeof(float4) * bn);
    w.em_key = (unsigned long long*)take(sizeof(unsigned long long) * bn);
    w.em_score = (float*)take(sizeof(float) * bn);
    w.total = off;
    return w;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_soft_nms_onchip_rows(void) { return SOFT_ONCHIP; }

size_t yolo_soft_nms_workspace_bytes(int b, int n) {
    if (b <= 0 || n < 0 || b > 2047 || n > SOFT_MAX_N) return 0;
    return soft_carve(nullptr, b, n).total;
}

int yolo_soft_nms(const float* boxes, int b, int n, double iou_threshold, double obj_threshold, double score_threshold, int center, int method,
                  double sigma, int class_agnostic, int max_det, int32_t* keep_idx, int32_t* keep_count, float* scores, float* rescore_rows,
                  void* workspace, size_t workspace_bytes, void* stream) {
    // every argument is judged before the first call into the runtime: none of these needs a device
    if (b < 0 || n < 0) return fail(YOLO_ERR_ARG, "soft_nms: b = %d or n = %d is negative", b, n);
    if (method < 0 || method > 2) return fail(YOLO_ERR_ARG, "soft_nms: method %d is not 0 (hard), 1 (linear) or 2 (Gaussian)", method);
    if (max_det < 0) return fail(YOLO_ERR_ARG, "soft_nms: max_det = %d is negative", max_det);
    if (!std::isfinite(iou_threshold) || !(iou_threshold >= 0.0))
        return fail(YOLO_ERR_ARG, "soft_nms: iou_threshold %g is not a finite number >= 0", iou_threshold);
    if (!std::isfinite(obj_threshold) || !std::isfinite(score_threshold))
        return fail(YOLO_ERR_ARG, "soft_nms: obj_threshold %g or score_threshold %g is not finite", obj_threshold, score_threshold);
    if (score_threshold < obj_threshold)
        return fail(YOLO_ERR_ARG, "soft_nms: score_threshold %g is below obj_threshold %g", score_threshold, obj_threshold);
    if (method == 2 && (!std::isfinite(sigma) || !(sigma > 0.0) || !((float)sigma > 0.0f) || !std::isfinite((float)sigma)))
        return fail(YOLO_ERR_ARG, "soft_nms: sigma %g is not a finite number > 0 (as fp32)", sigma);
    if (!boxes || !keep_idx || !keep_count || !scores) return fail(YOLO_ERR_ARG, "soft_nms: null pointer");
    if (n > SOFT_MAX_N || b > 2047) return fail(YOLO_ERR_UNSUPPORTED, "soft_nms: n = %d (max %d) or b = %d (max 2047) too large", n, SOFT_MAX_N, b);
    const size_t bn = (size_t)b * n;
    if (rescore_rows && rescore_rows != boxes) {
        const uintptr_t p = (uintptr_t)boxes, q = (uintptr_t)rescore_rows, bytes = sizeof(float) * 6 * bn;
        if (p < q + bytes && q < p + bytes) return fail(YOLO_ERR_ARG, "soft_nms: rescore_rows overlaps boxes without being boxes");
    }
    if (b == 0) return YOLO_OK;
    SoftWs w{};
    if (n > 0) {
        if (!workspace || ((uintptr_t)workspace & 15)) return fail(YOLO_ERR_ARG, "soft_nms: workspace missing or not 16-byte aligned");
        w = soft_carve(workspace, b, n);
        if (workspace_bytes < w.total) return fail(YOLO_ERR_ARG, "soft_nms: workspace %zu < %zu bytes", workspace_bytes, w.total);
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(keep_count, 0, sizeof(int) * (size_t)b, st) != hipSuccess) return fail(YOLO_ERR_LAUNCH, "soft_nms: memset");
    if (n == 0) return YOLO_OK;
    const int W = ceil_div(n, 64), agnostic = class_agnostic ? 1 : 0, cap = max_det > 0 ? max_det : INT_MAX;
    bool ok = hipMemsetAsync(keep_idx, 0xff, sizeof(int) * bn, st) == hipSuccess;
    ok = ok && hipMemsetAsync(scores, 0, sizeof(float) * bn, st) == hipSuccess;
    ok = ok && hipMemsetAsync(w.seg, 0, sizeof(int) * (size_t)b * SOFT_BUCKETS * 2, st) == hipSuccess;
    ok = ok && hipMemsetAsync(w.em_key, 0xff, sizeof(unsigned long long) * bn, st) == hipSuccess;
    if (!ok) return fail(YOLO_ERR_LAUNCH, "soft_nms: memset");
    static LdsOnce lds_once;
    if (int rc = reserve_lds(lds_once, reinterpret_cast<const void*>(soft_walk_kernel), SOFT_LDS, "soft_nms walk")) return rc;
    if (int rc = nms_order_class_sorted(boxes, b, n, W, obj_threshold, center, w.chunked, w.chunk_valid, w.sorted1, w.sorted2, w.nvalid,
                                        w.row_any, w.grank, w.sbox, w.blk_lo, w.blk_hi, st))
        return rc;
    const unsigned long long* order = agnostic ? w.sorted1 : w.sorted2;
    const dim3 gn(ceil_div(n, 256), b);
    if (int rc = nms_class_segments(w.sorted2, w.nvalid, b, n, agnostic, w.seg, st)) return rc;
    hipLaunchKernelGGL(soft_walk_kernel, dim3(agnostic ? 1 : SOFT_WGS, b), dim3(SOFT_THREADS), SOFT_LDS, st, boxes, order, w.sbox, w.seg, n, center ? 1 : 0,
                       agnostic, method, (float)iou_threshold, (float)sigma, score_threshold, cap, w.sp, w.em_key, w.em_score);
    if (int rc = check_launch("soft_nms walk")) return rc;
    hipLaunchKernelGGL(soft_merge_kernel, gn, dim3(256), 0, st, w.em_key, w.em_score, n, cap, keep_idx, keep_count, scores, rescore_rows);
    return check_launch("soft_nms merge");
}

}  // extern "C"
