// split3.h — the exact three-way bf16 split of an fp32 value, shared by the kernels that multiply fp32 operands on the bf16 matrix
// cores (conv_split3_f32.hip, and the Winograd F(4x4) planes of conv_wino4_f32.hip / conv_wino4s_f32.hip).
#pragma once
#include "common.h"

namespace yolo {

typedef __bf16 s3_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int s3_u32x4 __attribute__((ext_vector_type(4)));

// two floats' upper halves as one bf16 pair, `a` in the low half (the lower k)
__device__ __forceinline__ unsigned s3_pack(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

// v = hi + mid + lo exactly, each with 8 significand bits; chk turns NaN when v holds an Inf or a NaN
__device__ __forceinline__ void s3_split(const f32x4 v, u32x2& hi, u32x2& mid, u32x2& lo, f32x4& chk) {
    const s3_u32x4 vb = __builtin_bit_cast(s3_u32x4, v);
    const f32x4 h = __builtin_bit_cast(f32x4, vb & 0xffff0000u);
    const f32x4 r1 = v - h;
    const s3_u32x4 r1b = __builtin_bit_cast(s3_u32x4, r1);
    const f32x4 m = __builtin_bit_cast(f32x4, r1b & 0xffff0000u);
    const f32x4 r2 = r1 - m;
    const s3_u32x4 r2b = __builtin_bit_cast(s3_u32x4, r2);
    chk += r2 * 0.f;
    hi[0] = s3_pack(vb[0], vb[1]); hi[1] = s3_pack(vb[2], vb[3]);
    mid[0] = s3_pack(r1b[0], r1b[1]); mid[1] = s3_pack(r1b[2], r1b[3]);
    lo[0] = s3_pack(r2b[0], r2b[1]); lo[1] = s3_pack(r2b[2], r2b[3]);
}

}  // namespace yolo
