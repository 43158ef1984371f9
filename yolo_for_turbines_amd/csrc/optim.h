// optim.h — what the optimizer units share (optim.hip: SGD, the weight average, clipping; optim_adam.hip: Adam / AdamW):
// the row and state structs of the header, the chunk size, and the arithmetic of the weight average.
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
