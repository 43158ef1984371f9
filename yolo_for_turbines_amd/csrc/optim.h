// optim.h — what the optimizer units share (optim.hip: SGD, the weight average, clipping; optim_adam.hip: Adam / AdamW):
// the row and state structs of the header, the chunk size and the walk over a chunk, and the arithmetic of the weight average.
#pragma once
#include "common.h"

namespace yolo {

struct SgdItem { float* p; const float* g; float* buf; long long n; };   // n < 0: the momentum buffer is new (first step): buf = g'
static_assert(sizeof(SgdItem) == 32, "matches yolo_sgd_item in the header");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int SGD_CHUNK = 4096;          // elements per block: 256 threads x 4 x float4

struct EmaState { int updates; float decay; int warmup; int reserved; };
static_assert(sizeof(EmaState) == 16, "matches yolo_ema_state in the header");

struct ClipState { float max_norm; float total_norm; float coef; int norm_type; };
static_assert(sizeof(ClipState) == 16, "matches yolo_clip_state in the header");

// A block's walk over its chunk ck = (item, first element) of a tensor of n elements: thread t takes the four elements at
// ck.y + r * 1024 + 4 t, r = 0 .. SGD_CHUNK / 1024 - 1, and calls f(i0, cnt, vec) for every such quad that begins inside the
// tensor. cnt: how many of the four exist; vec: all four do and every pointer is 16-byte aligned (one float4 each).
template <typename F>
__device__ __forceinline__ void for_each_quad(int2 ck, long long n, bool aligned, F&& f) {
#pragma unroll
    for (int r = 0; r < SGD_CHUNK / 1024; ++r) {
        const long long i0 = (long long)ck.y + r * 1024 + threadIdx.x * 4;
        if (i0 >= n) break;
        const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
        f(i0, cnt, aligned && cnt == 4);
    }
}

// The read-only pass over a chunk of gradients, as 32-bit words: take(bits) for every element of the walk above, in its order.
// A full chunk has its SGD_CHUNK / 1024 independent 16-byte loads in flight before the first word is looked at.
template <typename T>
__device__ __forceinline__ void scan_grad_chunk(const unsigned* __restrict__ g, int2 ck, long long n, T&& take) {
    const bool aligned = (((size_t)g) & 15) == 0;
    if (aligned && (long long)ck.y + SGD_CHUNK <= n) {
        const long long base = (long long)ck.y + threadIdx.x * 4;
        u32x4 v[SGD_CHUNK / 1024];
#pragma unroll
        for (int r = 0; r < SGD_CHUNK / 1024; ++r) v[r] = *reinterpret_cast<const u32x4*>(g + base + r * 1024);
#pragma unroll
        for (int r = 0; r < SGD_CHUNK / 1024; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) take(v[r][e]);
    } else {
        for_each_quad(ck, n, aligned, [&](long long i0, int cnt, bool vec) {
            if (vec) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(g + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) take(v[e]);
            } else {
                for (int e = 0; e < cnt; ++e) take(g[i0 + e]);
            }
        });
    }
}

// {d, 1 - d} of this update, from the state as it is when the block runs
__device__ __forceinline__ void ema_coeffs(const EmaState* __restrict__ st, float& d, float& omd) {
    const u32x4 s = *reinterpret_cast<const u32x4*>(st);
    const int t = (int)s[0];
    d = __uint_as_float(s[1]);
    if (s[2] != 0) {
        const float q = (float)(1 + t) / (float)(10 + t);
        if (q < d) d = q;
    }
    omd = 1.0f - d;
}

// e * d is an argument of the fused multiply-add, not a candidate for contraction: it is rounded on its own, like mul_
__device__ __forceinline__ float ema_one(float e, float p, float d, float omd) { return __builtin_fmaf(omd, p, e * d); }

}  // namespace yolo
