// nms_mask.hip — NMS stage 2: the suppression matrix in 64-bit words.   BUILD WITH -ffp-contract=off.
//
// Word (i, cb) of image b: bit jj set <=> box j = cb * 64 + jj comes after box i in the stage-1 order, has the same class and
// !(iou < thr) - "j is suppressed by i if i is kept" (calc_iou code/utils.py:38-84, the test of non_max_suppression :183-186).
// The result must equal the reference's for any fp32 input, which needs
//  (1) the reference's fp32 operation order for IoU with one rounding per op (no FMA contraction, IEEE division) - area and
//      corner sums are per-box values, so they are computed once per box (SBox);
//  (2) NaN-propagating max/min (torch.max/min propagate NaN, fmaxf/fminf do not);
//  (3) the IoU threshold compared in fp32.
// Two kernels over the same word routine: nms_mask_kernel (every 64x64 tile of the upper triangle) and nms_mask_sorted_kernel
// (class-major rows: only the column blocks whose class range overlaps the row block's). The bound is VALU pair work.
#include "nms.h"

namespace yolo {
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }

// One 64-bit suppression word: bit jj set <=> column col0 + jj comes after row i, has the same class and !(iou < thr)
// (utils.py:38-84 + 183-186). `cols` is the staged column block in LDS, `lim` its valid length.
// TAME: every coordinate and area of the 64 rows and the columns is below 1e18 in magnitude, so nothing before the
// division can be NaN or overflow and the NaN-propagating max / min / clamp reduce to plain v_max / v_min (the sign of a
// zero they may pick differently cannot reach the comparison: it only ever yields iou = +-0); and when no row of the
// wave has a same-class column with a non-zero intersection, iou is exactly +-0 over a positive denominator and the
// IEEE division is skipped. Same bits as the general path, about half the instructions per pair.
// bare v_max / v_min: fmaxf() makes the compiler canonicalise both operands first (3 instructions instead of 1)
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

__device__ __forceinline__ bool tame_box(const SBox& q) {
    const float lim = 1e18f;
    return fabsf(q.x1) < lim && fabsf(q.y1) < lim && fabsf(q.x2) < lim && fabsf(q.y2) < lim && fabsf(q.area) < lim;
}

// Per-row bounds of the fast path's candidate test (below): the column must reach x2 >= lo_x, x1 <= hi_x, y2 >= lo_y, y1 <= hi_y.
// The loose form is "the boxes overlap". The tight form uses what !(iou < thr) implies for thr > 0 with positive areas: from
// iou = fl(inter / den) >= thr and den = fl(fl(fl(a1 + a2) - inter) + 1e-6) follows inter >= 0.99 (thr / (1 + thr)) a1 (every
// rounding is a factor 1 +- 2^-24; a2 >= 0), and inter = fl(iw ih) with ih <= fl(y2 - y1) of the row itself, so the width of the
// intersection must be at least T = 0.98 (thr / (1 + thr)) a1 / fl(y2 - y1) - and its height U likewise. For equal-sized boxes at
// thr = 0.45 that halves the candidates the exact pass has to divide for, and it costs nothing per pair: the four compares
// stay, only their per-row constants move. The bounds are rounded outwards by a few ulps; a pair they admit wrongly is still
// decided by the exact pass, so the result cannot change - a pair they reject is one the exact formula cannot suppress.
struct RowBounds { float lo_x, hi_x, lo_y, hi_y; };
__device__ __forceinline__ RowBounds row_bounds(const SBox& me, float thr) {
    float T = 0.f, U = 0.f;
    const float ew = me.x2 - me.x1, eh = me.y2 - me.y1;
    if (thr > 1e-6f && thr < 1e3f && me.area > 1e-30f && ew > 1e-30f && eh > 1e-30f) {
        const float kf = 0.98f * (thr / (1.0f + thr)) * me.area;
        T = kf * __builtin_amdgcn_rcpf(eh);
        U = kf * __builtin_amdgcn_rcpf(ew);
    }
    RowBounds r;
    r.lo_x = me.x1 + T; r.hi_x = me.x2 - T; r.lo_y = me.y1 + U; r.hi_y = me.y2 - U;
    r.lo_x -= fabsf(r.lo_x) * 0x1p-21f; r.hi_x += fabsf(r.hi_x) * 0x1p-21f;       // outwards: the sums above were rounded
    r.lo_y -= fabsf(r.lo_y) * 0x1p-21f; r.hi_y += fabsf(r.hi_y) * 0x1p-21f;
    return r;
}

template <bool TAME>
__device__ __forceinline__ unsigned long long suppression_word(const SBox& me, bool active, int i, const SBox* cols, int lim, int col0,
                                                              float thr, const SBox* __restrict__ gcols, const RowBounds& rbnd) {
    unsigned long long word = 0;
    if (TAME) {
        // Two passes. (1) all 64 columns, ~10 instructions per pair: CANDIDATE = same class and the boxes overlap in x and in y
        // (strictly positive width and height of the intersection). Every other same-class pair has inter = +-0 exactly, and with
        // den = (a1 + a2) + 1e-6 > 0 (checked per pair) its iou is +-0: it suppresses iff !(0 < thr), decided once per word.
        // (2) the exact IoU with the IEEE division only for the candidates, each lane walking the set bits of ITS word: with
        // 2 classes and 10,000 boxes 3 % of the pairs are candidates (~2 per word, ~7 for the busiest lane of a wave), so
        // the division work drops ~8x; the old single pass divided whenever ANY of a wave's 256 pairs intersected - always.
        const bool zero_suppresses = !(0.f < thr);        // iou == +-0 for a pair that does not intersect
        unsigned clo = 0, chi = 0, slo = 0, shi = 0;      // candidate bits / same-class-and-zero-iou bits, low and high 32 columns
        auto half = [&](int j0, unsigned& cbits, unsigned& sbits) {
#pragma unroll 8
            for (int jj = 0; jj < 32; ++jj) {             // branch-free: bitwise & / | on the predicates, all six fields read up front
                const f32x4 c = *reinterpret_cast<const f32x4*>(&cols[j0 + jj].x1);    // entries at or beyond lim are masked out below
                const f32x2 ac = *reinterpret_cast<const f32x2*>(&cols[j0 + jj].area); // area, cls
                const bool same = ac[1] == me.cls;
                const float xa = vmax(me.x1, c[0]), ya = vmax(me.y1, c[1]);
                const float xb = vmin(me.x2, c[2]), yb = vmin(me.y2, c[3]);
                const bool den_bad = !((me.area + ac[0]) + 1e-6f > 0.f);               // ((a1 + a2) - 0) + 1e-6, the pair's denominator
                const bool cand = same & (((xb > xa) & (yb > ya)) | den_bad);
                const unsigned bit = 1u << jj;
                cbits |= cand ? bit : 0u;
                sbits |= same ? bit : 0u;
            }
        };
        // the common column block: every row and column of one class and every area positive (so the denominator of a
        // non-intersecting pair is positive) - 4 min/max + 2 compares per pair and nothing else
        auto half_uni = [&](int j0, unsigned& cbits) {
#pragma unroll 8
            for (int jj = 0; jj < 32; ++jj) {
                const f32x4 c = *reinterpret_cast<const f32x4*>(&cols[j0 + jj].x1);
                const float xa = vmax(me.x1, c[0]), ya = vmax(me.y1, c[1]);
                const float xb = vmin(me.x2, c[2]), yb = vmin(me.y2, c[3]);
                cbits |= ((xb > xa) & (yb > ya)) ? (1u << jj) : 0u;
            }
        };
        const int lane_c = (int)(threadIdx.x & 63);
        const bool odd = (active && !(me.area > 0.f)) || (lane_c < lim && !(cols[lane_c].area > 0.f)) ||
                         (active && cols[0].cls != me.cls) || (lane_c < lim && cols[lane_c].cls != cols[0].cls);
        // ... and when, on top of that, every box of the block has a positive width and height, "the intersection has a positive
        // width" is just o.x1 < me.x2 && me.x1 < o.x2 (min(a2, b2) > max(a1, b1) with a2 > a1, b2 > b1), likewise for y:
        // four compares whose lane masks are ANDed on the scalar unit, and the bit goes into the word as the carry-in of
        // w + w (v_addc_co_u32): 5 vector instructions per pair instead of 8. The column's four coordinates are uniform,
        // so they come from the scalar cache (s_load of the global array) as SGPR operands - no LDS read in this loop.
        // (The counters say the kernel is VALU-issue-bound: 109 M vector instructions = 203 us of issue in a 290 us launch.)
        const bool flat = (active && !(me.x2 > me.x1 && me.y2 > me.y1)) ||
                          (lane_c < lim && !(cols[lane_c].x2 > cols[lane_c].x1 && cols[lane_c].y2 > cols[lane_c].y1));
        if (gcols != nullptr && lim == 64 && __ballot(odd || flat) == 0ull) {   // full column blocks only: constant load offsets, no address arithmetic
            auto half_fast = [&](int j0, unsigned& cbits) {
                unsigned w = 0;
#pragma unroll
                for (int g8 = 24; g8 >= 0; g8 -= 8) {                            // 8 columns' coordinates requested before they are used
                    f32x4 c8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) c8[u] = *reinterpret_cast<const f32x4*>(&gcols[j0 + g8 + u].x1);
                    // four columns per statement, highest first. v_cmpx narrows EXEC, so four chained compares leave
                    // VCC = EXEC = the lanes where all four hold (the AND costs no instruction); EXEC is restored from a copy and
                    // the bit enters w as the carry-in of w + w: 5 vector + 1 scalar instruction per pair.
#define NMS_COL4(q) \
                    { unsigned long long sv; \
                      asm volatile("s_mov_b64 %[sv], exec\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[a3], %[mx2]\n\tv_cmpx_ge_f32_e32 vcc, %[c3], %[mx1]\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[b3], %[my2]\n\tv_cmpx_ge_f32_e32 vcc, %[d3], %[my1]\n\t" \
                                   "s_mov_b64 exec, %[sv]\n\tv_addc_co_u32_e32 %[w], vcc, %[w], %[w], vcc\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[a2], %[mx2]\n\tv_cmpx_ge_f32_e32 vcc, %[c2], %[mx1]\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[b2], %[my2]\n\tv_cmpx_ge_f32_e32 vcc, %[d2], %[my1]\n\t" \
                                   "s_mov_b64 exec, %[sv]\n\tv_addc_co_u32_e32 %[w], vcc, %[w], %[w], vcc\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[a1], %[mx2]\n\tv_cmpx_ge_f32_e32 vcc, %[c1], %[mx1]\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[b1], %[my2]\n\tv_cmpx_ge_f32_e32 vcc, %[d1], %[my1]\n\t" \
                                   "s_mov_b64 exec, %[sv]\n\tv_addc_co_u32_e32 %[w], vcc, %[w], %[w], vcc\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[a0], %[mx2]\n\tv_cmpx_ge_f32_e32 vcc, %[c0], %[mx1]\n\t" \
                                   "v_cmpx_le_f32_e32 vcc, %[b0], %[my2]\n\tv_cmpx_ge_f32_e32 vcc, %[d0], %[my1]\n\t" \
                                   "s_mov_b64 exec, %[sv]\n\tv_addc_co_u32_e32 %[w], vcc, %[w], %[w], vcc" \
                                   : [w] "+v"(w), [sv] "=&s"(sv) \
                                   : [a0] "s"(c8[q][0]), [b0] "s"(c8[q][1]), [c0] "s"(c8[q][2]), [d0] "s"(c8[q][3]), \
                                     [a1] "s"(c8[q + 1][0]), [b1] "s"(c8[q + 1][1]), [c1] "s"(c8[q + 1][2]), [d1] "s"(c8[q + 1][3]), \
                                     [a2] "s"(c8[q + 2][0]), [b2] "s"(c8[q + 2][1]), [c2] "s"(c8[q + 2][2]), [d2] "s"(c8[q + 2][3]), \
                                     [a3] "s"(c8[q + 3][0]), [b3] "s"(c8[q + 3][1]), [c3] "s"(c8[q + 3][2]), [d3] "s"(c8[q + 3][3]), \
                                     [mx1] "v"(rbnd.lo_x), [my1] "v"(rbnd.lo_y), [mx2] "v"(rbnd.hi_x), [my2] "v"(rbnd.hi_y) \
                                   : "vcc"); }
                    NMS_COL4(4)
                    NMS_COL4(0)
#undef NMS_COL4
                }
                cbits = w;
            };
            half_fast(0, clo);
            half_fast(32, chi);
            slo = shi = ~0u;
        } else if (__ballot(odd) == 0ull) {
            half_uni(0, clo);
            half_uni(32, chi);
            slo = shi = ~0u;
        } else {
            half(0, clo, slo);
            half(32, chi, shi);
        }
        const unsigned long long valid = lim >= 64 ? ~0ull : ((1ull << lim) - 1ull);
        unsigned long long cw = ((((unsigned long long)chi) << 32) | clo) & valid;
        const unsigned long long sw = ((((unsigned long long)shi) << 32) | slo) & valid;
        if (!active) cw = 0ull;
        word = (active && zero_suppresses) ? (sw & ~cw) : 0ull;
        while (__ballot(cw != 0ull)) {                    // wave-uniform trip count: the busiest lane's candidates
            if (cw) {
                const int jj = __builtin_ctzll(cw);
                cw &= cw - 1ull;
                const SBox o = cols[jj];
                const float xa = vmax(me.x1, o.x1), ya = vmax(me.y1, o.y1);
                const float xb = vmin(me.x2, o.x2), yb = vmin(me.y2, o.y2);
                const float iw = vmax(xb - xa, 0.f), ih = vmax(yb - ya, 0.f);
                const float inter = iw * ih;
                const float den = ((me.area + o.area) - inter) + 1e-6f;
                const float iou = inter / den;
                if (!(iou < thr)) word |= 1ull << jj;
            }
        }
        // only columns after row i
        const int first = i + 1 - col0;                   // first admissible bit
        if (first > 0) word &= first >= 64 ? 0ull : (~0ull << first);
        return word;
    }
    for (int jj = 0; jj < lim; ++jj) {
        const SBox o = cols[jj];
        // a box of another class never suppresses (kept if `cls != top.cls` OR iou < thr): skip the column when no row of
        // this wave shares its class
        if (__ballot(active && o.cls == me.cls) == 0ull) continue;
        const float xa = max_nan(me.x1, o.x1), ya = max_nan(me.y1, o.y1);
        const float xb = min_nan(me.x2, o.x2), yb = min_nan(me.y2, o.y2);
        float iw = xb - xa, ih = yb - ya;
        iw = iw < 0.f ? 0.f : iw;                       // torch.clamp(min=0): NaN stays NaN
        ih = ih < 0.f ? 0.f : ih;
        const float inter = iw * ih;
        const float uni = (me.area + o.area) - inter;
        const float iou = inter / (uni + 1e-6f);
        const bool survive = (o.cls != me.cls) || (iou < thr);
        if (active && !survive && col0 + jj > i) word |= 1ull << jj;
    }
    return word;
}

__device__ __forceinline__ unsigned long long suppression_word(const SBox& me, bool active, int i, const SBox* cols, int lim, int col0,
                                                              float thr, const SBox* __restrict__ gcols = nullptr,
                                                              const RowBounds& rbnd = RowBounds{0.f, 0.f, 0.f, 0.f}) {
    const bool wild = (active && !tame_box(me)) || ((int)(threadIdx.x & 63) < lim && !tame_box(cols[threadIdx.x & 63]));
    return __ballot(wild) == 0ull ? suppression_word<true>(me, active, i, cols, lim, col0, thr, gcols, rbnd)
                                  : suppression_word<false>(me, active, i, cols, lim, col0, thr, gcols, rbnd);
}

// ---- class-sorted variant (2,048 <= n <= 163,456) ---------------------------------------------------------------------
// A box only ever suppresses boxes of its own class (utils.py:183-186), so after a second STABLE sort by class the
// suppression matrix is block diagonal: the mask kernel visits only the column blocks whose class range overlaps the row
// block's (1/nc of the pairs for nc balanced classes) and the scan ORs only those. Greedy NMS per class in score order
// is exactly the reference's result; the scan then emits the kept set in the reference's (global score) order.

// grid (1, B, W), MS_WAVES waves: wave w takes row block rb against column blocks rb + w, + MS_WAVES, ... while the class ranges overlap
__global__ __launch_bounds__(64 * MS_WAVES) void nms_mask_sorted_kernel(const SBox* __restrict__ sbox, const int* __restrict__ nvalid,
                                                             const int* __restrict__ blk_lo, const int* __restrict__ blk_hi, int n,
                                                             int W, float thr, unsigned long long* __restrict__ mask,
                                                             unsigned long long* __restrict__ row_any, unsigned long long* __restrict__ near) {
    // row block slowest, image in the middle: the workgroups are dispatched in that order, and a row block's work shrinks
    // along its class range, so with the image slowest the last images' longest workgroups started late and ran alone at the end
    const int rb = blockIdx.z, b = blockIdx.y;
    const int nv = nvalid[b];
    if (rb * 64 >= nv) return;
    const int nblk = (nv + 63) / 64;
    // every wave works alone (its own staging buffer, its own trip count): no workgroup barrier below, only the wave's own
    // program order (LDS operations of one wave execute in order; the wave barrier keeps the compiler from moving them).
    // (Requesting the row's box, the class bounds and the first column block before nvalid is known was tried: the compiler
    // sinks the loads below the early exit again and parks the column block in LDS - 24 -> 48 us at 80 classes.)
    __shared__ SBox cols_all[MS_WAVES][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    SBox* cols = cols_all[wave];
    const SBox* sb = sbox + (size_t)b * n;
    const int i = rb * 64 + lane;
    const bool active = i < nv;
    const int hi_r = blk_hi[(size_t)b * W + rb];
    const int cb_first = rb + blockIdx.x * MS_WAVES + wave;
    // a wave whose first column block is already outside the row block's class range has nothing to do (with 80 classes
    // most of a workgroup's waves): it leaves before it asks for its rows' boxes
    if (cb_first >= nblk || blk_lo[(size_t)b * W + cb_first] > hi_r) return;
    const SBox me = sb[active ? i : nv - 1];
    const RowBounds rbnd = row_bounds(me, thr);
    for (int cb = cb_first; cb < nblk; cb += gridDim.x * MS_WAVES) {
        if (blk_lo[(size_t)b * W + cb] > hi_r) break;    // classes ascend: no later block can match either
        const int j = cb * 64 + lane;
        __builtin_amdgcn_wave_barrier();
        if (j < nv) cols[lane] = sb[j];
        __builtin_amdgcn_wave_barrier();
        const int lim = nv - cb * 64 < 64 ? nv - cb * 64 : 64;
        const unsigned long long word = suppression_word(me, active, i, cols, lim, cb * 64, thr, sb + cb * 64, rbnd);
        if (active) mask[((size_t)b * n + i) * W + cb] = word;
        if (active && cb - rb <= SCAN_NEAR) near[(((size_t)b * W + rb) * (SCAN_NEAR + 1) + (cb - rb)) * 64 + lane] = word;
        const unsigned long long bal = __ballot(active && word != 0ull);
        if (cb > rb && lane == 0 && bal) atomicOr(&row_any[(size_t)b * W + rb], bal);
    }
}

// grid (W, W, B), 64 threads. word (i, cb): bit jj set <=> j = cb*64+jj > i, same class, !(iou < thr)
__global__ __launch_bounds__(64) void nms_mask_kernel(const SBox* __restrict__ sbox, const int* __restrict__ nvalid, int n,
                                                      int W, float thr, unsigned long long* __restrict__ mask,
                                                      unsigned long long* __restrict__ row_any) {
    const int cb = blockIdx.x, rb = blockIdx.y, b = blockIdx.z;
    if (cb < rb) return;
    const int nv = nvalid[b];
    if (rb * 64 >= nv || cb * 64 >= nv) return;
    __shared__ SBox cols[64];
    const SBox* sb = sbox + (size_t)b * n;
    const int j = cb * 64 + threadIdx.x;
    if (j < nv) cols[threadIdx.x] = sb[j];
    __syncthreads();
    const int i = rb * 64 + threadIdx.x;
    const bool active = i < nv;
    const SBox me = sb[active ? i : nv - 1];
    const int lim = nv - cb * 64 < 64 ? nv - cb * 64 : 64;
    const unsigned long long word = suppression_word(me, active, i, cols, lim, cb * 64, thr);
    if (!active) return;
    mask[((size_t)b * n + i) * W + cb] = word;
    // row_any[b][rb] bit t: row rb*64+t has a suppression bit in some LATER column block (integer OR:
    // order-independent, so still deterministic)
    const unsigned long long bal = __ballot(word != 0ull);
    if (cb > rb && threadIdx.x == 0 && bal) atomicOr(&row_any[(size_t)b * W + rb], bal);
}

// ---- host side
int nms_mask_plain(const SBox* sbox, const int* nvalid, int b, int n, int W, float thr, unsigned long long* mask, unsigned long long* row_any,
                   hipStream_t st) {
    hipLaunchKernelGGL(nms_mask_kernel, dim3(W, W, b), dim3(64), 0, st, sbox, nvalid, n, W, thr, mask, row_any);
    return check_launch("nms_mask");
}

int nms_mask_class_sorted(const SBox* sbox, const int* nvalid, const int* blk_lo, const int* blk_hi, int b, int n, int W, float thr,
                          unsigned long long* mask, unsigned long long* row_any, unsigned long long* near, hipStream_t st) {
    // 4 column-block strides per row block (today the MS_WAVES waves of one workgroup): with many classes only the first 2-3
    // column blocks are in range and every further (empty) stride costs launch time (80 classes: 0.212 / 0.221 / 0.250 / 0.305 ms
    // for 3 / 4 / 8 / 16), with 2 classes more help a little (1.16 / 1.12 / 1.05 / 1.02 ms)
    hipLaunchKernelGGL(nms_mask_sorted_kernel, dim3(1, b, W), dim3(64 * MS_WAVES), 0, st, sbox, nvalid, blk_lo, blk_hi, n, W, thr, mask,
                       row_any, near);
    return check_launch("nms_mask_sorted");
}

}  // namespace yolo
