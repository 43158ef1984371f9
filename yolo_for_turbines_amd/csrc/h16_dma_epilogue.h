// h16_dma_epilogue.h — the register epilogues of the LDS-DMA kernels (conv3_dma_h16.hip, conv1_dma_h16.hip): inference
// (d_epilogue), train-mode forward with BatchNorm partial sums (d_epilogue_stats), input gradient with the BatchNorm-backward
// sums (d_epilogue_bstats) and the fused stride-2 input gradient (d_epilogue_s2g).
#pragma once
#include "h16.h"

namespace yolo {

struct DRes {                       // residual rows of the epilogue, requested from inside the last K steps (see d_kstep, e_step)
    const unsigned short* rptr[2];  // row of this lane's pixel in m-tile 0 / 1 (+ r_off), null-safe (pixel clamped)
    int ch0;                        // first of this lane's 8 channels (+ j * 64 + kp * 16)
    bool has_res;
};

// ---- epilogue of conv3_dma_h16 / conv1_dma_h16 (fp32 math, from registers)
// acc[i][j]: rows = the 32 channels of this wave's n-tile j, columns = the 32 pixels of m-tile i. A lane owns pixel
// (lane & 31) and channels 8g + 4h + {0..3} (g = 0..3, h = lane >> 5). Scale / shift / activation in that layout; then
// one v_permlane32_swap per register pair exchanges halves so that lanes 0-31 hold channels 8k .. 8k+7 and lanes 32-63
// channels 8k+8 .. 8k+15 of their pixel (k = 0, 2): 16 contiguous bytes of output per lane -> ONE 16-byte store (and one
// 16-byte residual row, requested inside the last chunk) per lane, pixel and 16 channels. No LDS round trip, no barrier
// (cdna_hip_programming.md T21). Phases: (A) arithmetic of all four tiles, (B) ALL residual adds, (C) per 16-byte group: NaN guard,
// one rounding, store - nothing that could wait on memory sits between two stores.
template <typename T, int BN, int ACT, bool RES>
__device__ __forceinline__ bool d_epilogue(const ConvHArgs& p, const f32x16 (&acc)[2][BN / 64], const u32x4 (&rr)[2][BN / 64][2],
                                           const float* sstab, const int (&mpix)[2], const size_t (&ooff)[2], int ch0, int wn, int fh) {
    constexpr int TN = BN / 64;
    float w[2][TN][2][8];           // w[i][j][kp][0..7] = this lane's 8 consecutive output channels (ch0 + j*64 + kp*16 ...) of pixel mpix[i]
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        // folded BatchNorm scale / shift of channels 8g + 4h + {0..3}: broadcast reads of the table the prologue staged
        f32x4 sc4[4], sh4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            sc4[g] = *reinterpret_cast<const f32x4*>(sstab + j * 64 + wn * 32 + 8 * g + 4 * fh);
            sh4[g] = *reinterpret_cast<const f32x4*>(sstab + BN + j * 64 + wn * 32 + 8 * g + 4 * fh);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = act_c<ACT>(acc[i][j][r] * sc4[r >> 2][r & 3] + sh4[r >> 2][r & 3]);
            // half exchange on the fp32 values (one rounding, after the residual add): group pairs (0,1) and (2,3)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[8 * kp + e]), __float_as_uint(v[8 * kp + 4 + e]), false, false);
                    w[i][j][kp][e] = __uint_as_float(sw[0]);          // lanes 0-31: own group 2kp | lanes 32-63: lower half's group 2kp+1
                    w[i][j][kp][4 + e] = __uint_as_float(sw[1]);      // lanes 0-31: upper half's group 2kp | lanes 32-63: own group 2kp+1
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);      // phases stay phases: overlapped by the scheduler they were all live at once (250 VGPRs)
    if (RES) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int kp = 0; kp < 2; ++kp)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        w[i][j][kp][2 * e] += HTraits<T>::to_f32((unsigned short)(rr[i][j][kp][e] & 0xffffu));
                        w[i][j][kp][2 * e + 1] += HTraits<T>::to_f32((unsigned short)(rr[i][j][kp][e] >> 16));
                    }
        __builtin_amdgcn_sched_barrier(0);
    }
    bool saw_nan = false;
    unsigned short* yo = reinterpret_cast<unsigned short*>(p.y);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = w[i][j][kp][2 * e], x1 = w[i][j][kp][2 * e + 1];
                    saw_nan |= __builtin_isunordered(x0, x1);          // one v_cmp_u_f32 per pair
                    o[e] = pack2<T>(x0, x1);
                }
                if (mpix[i] < 0 || ch0 + j * 64 + kp * 16 >= p.Cout) continue;
                unsigned short* d = yo + ooff[i] + j * 64 + kp * 16;
                *reinterpret_cast<u32x4*>(d) = o;
                if (p.out_mode != YOLO_OUT_NHWC) {
                    const size_t W2 = 2 * (size_t)p.Wo;
                    *reinterpret_cast<u32x4*>(d + p.y_ld) = o;
                    *reinterpret_cast<u32x4*>(d + W2 * p.y_ld) = o;
                    *reinterpret_cast<u32x4*>(d + (W2 + 1) * p.y_ld) = o;
                }
            }
    return saw_nan;
}


// ---- epilogue of the train-mode forward: raw convolution output z (no scale / shift / activation / residual) AND the
// BatchNorm partial sums of this wave's 64 pixels x 64 channels, so that the statistics pass over z (one full read of every
// conv output: 0.7 ms of the 17 ms bf16 step) disappears. Sums are taken of the ROUNDED values, i.e. of exactly what is
// stored and normalised later (the reference's batch_norm sees the 16-bit conv output too).
// After the half exchange of d_epilogue a lane holds 8 consecutive channels of ONE pixel per (n-tile j, channel pair kp) and
// m-tile i: 2 (sum, sum of squares) x 2 x 2 x 8 = 64 per-lane values, each to be added over the 32 pixels (lanes) of its half.
// A reduce-scatter butterfly does that in 31 + 31 adds instead of 64 x 5: every level pairs two registers and two lane groups,
// each group keeps one register of the pair and receives the partner group's copy of it:
//   level 16: v_permlane16_swap (odd rows of X <-> even rows of Y), pair = (sum, sum of squares)  -> bit 4 of the lane = quantity
//   level  8: DPP row_mirror (l <-> 15 - l),       pair = n-tile 0 / 1                           -> bit 3 = j
//   level  4: DPP row_half_mirror (l <-> 7 - l),   pair = channel pair kp 0 / 1                  -> bit 2 = kp
//   level  2: DPP quad_perm [2,3,0,1],             pair = channels e / e + 4                      -> bit 1
//   level  1: DPP quad_perm [1,0,3,2],             pair = channels e / e + 2                      -> bit 0
// leaving two values (channels c, c + 1) per lane: one 8-byte store into stats[row][quantity][channel].
template <int BN>
__device__ __forceinline__ void stats_reduce_store(const ConvHArgs& p, const float (&sq)[2][BN / 64][2][8], int ch0, int lane, int row) {
    constexpr int TN = BN / 64;
    // level 16
    float l8[TN][2][8];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int kp = 0; kp < 2; ++kp)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(sq[0][j][kp][e]), __float_as_uint(sq[1][j][kp][e]), false, false);
                l8[j][kp][e] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
            }
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
    float l4[2][8];
#pragma unroll
    for (int kp = 0; kp < 2; ++kp)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float t0 = l8[0][kp][e] + dpp_f<0x140>(l8[0][kp][e]);       // row_mirror
            const float t1 = l8[1][kp][e] + dpp_f<0x140>(l8[1][kp][e]);
            l4[kp][e] = b3 ? t1 : t0;
        }
    float l2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t0 = l4[0][e] + dpp_f<0x141>(l4[0][e]);                   // row_half_mirror
        const float t1 = l4[1][e] + dpp_f<0x141>(l4[1][e]);
        l2[e] = b2 ? t1 : t0;
    }
    float l1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t0 = l2[e] + dpp_f<0x4E>(l2[e]);                          // quad_perm [2,3,0,1]
        const float t1 = l2[e + 4] + dpp_f<0x4E>(l2[e + 4]);
        l1[e] = b1 ? t1 : t0;
    }
    float l0[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float t0 = l1[e] + dpp_f<0xB1>(l1[e]);                          // quad_perm [1,0,3,2]
        const float t1 = l1[e + 2] + dpp_f<0xB1>(l1[e + 2]);
        l0[e] = b0 ? t1 : t0;
    }
    const int qty = (lane >> 4) & 1;
    const int ch = ch0 + (b3 ? 64 : 0) + (b2 ? 16 : 0) + (b1 ? 4 : 0) + (b0 ? 2 : 0);
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 out = {l0[0], l0[1]};
    *reinterpret_cast<f32x2*>(p.stats + ((size_t)row * 2 + qty) * p.stats_ld + ch) = out;      // stats_ld covers the padded channel tiles
}

template <typename T, int BN>
__device__ __forceinline__ void d_epilogue_stats(const ConvHArgs& p, const f32x16 (&acc)[2][BN / 64], const int (&mpix)[2],
                                                 const size_t (&ooff)[2], int ch0, int lane, int row) {
    constexpr int TN = BN / 64;
    static_assert(TN == 2, "two n-tiles per wave");
    float sq[2][TN][2][8];                                  // [quantity][j][kp][e]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp)
#pragma unroll
                for (int e = 0; e < 8; ++e) sq[a][j][kp][e] = 0.f;
    unsigned short* yo = reinterpret_cast<unsigned short*>(p.y);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float live = mpix[i] < 0 ? 0.f : 1.f;        // tile padding: the lane computed a duplicate of pixel 0, counts for nothing
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                float w[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][j][8 * kp + e]), __float_as_uint(acc[i][j][8 * kp + 4 + e]), false, false);
                    w[e] = __uint_as_float(sw[0]);
                    w[4 + e] = __uint_as_float(sw[1]);
                }
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = pack2<T>(w[2 * e], w[2 * e + 1]);
                    const float r0 = HTraits<T>::to_f32((unsigned short)(o[e] & 0xffffu)) * live;
                    const float r1 = HTraits<T>::to_f32((unsigned short)(o[e] >> 16)) * live;
                    sq[0][j][kp][2 * e] += r0;
                    sq[0][j][kp][2 * e + 1] += r1;
                    sq[1][j][kp][2 * e] = __builtin_fmaf(r0, r0, sq[1][j][kp][2 * e]);
                    sq[1][j][kp][2 * e + 1] = __builtin_fmaf(r1, r1, sq[1][j][kp][2 * e + 1]);
                }
                if (mpix[i] >= 0 && ch0 + j * 64 + kp * 16 < p.Cout) *reinterpret_cast<u32x4*>(yo + ooff[i] + j * 64 + kp * 16) = o;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    stats_reduce_store<BN>(p, sq, ch0, lane, row);
}

// ---- epilogue of an input-gradient launch that ALSO takes the BatchNorm-backward sums of the block that produced this
// convolution's input (the block whose output gradient dx is): identity epilogue [+ the running gradient], rounded once, and
// of exactly those rounded values  sum(du)  and  sum(du * (z - mean))  with  du = dx * act'((z - mean) * scale + shift)  -
// the formula (and the fp32 operation order) of bn_bwd_partial, whose pass over dx and z this replaces. z is read here
// once (a 16-byte row per lane, pixel and 8 channels, like the residual). Same per-wave rows as d_epilogue_stats.
template <typename T, int BN, int ACT>
__device__ __forceinline__ void d_epilogue_bstats(const ConvHArgs& p, const f32x16 (&acc)[2][BN / 64], const u32x4 (&rr)[2][BN / 64][2],
                                                  bool has_res, const int (&mpix)[2], const size_t (&ooff)[2], int ch0, int lane, int row) {
    constexpr int TN = BN / 64;
    unsigned short* yo = reinterpret_cast<unsigned short*>(p.y);
    size_t zoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) zoff[i] = (size_t)(mpix[i] < 0 ? 0 : mpix[i]) * p.bz_ld + p.bz_off;
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
    float* srow = p.stats + ((size_t)row * 2 + ((lane >> 4) & 1)) * p.stats_ld + (b3 ? 4 : 0) + (b2 ? 2 : 0) + (b1 ? 1 : 0);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) {
            const int cb = ch0 + j * 64 + kp * 16;
            const bool chan_ok = cb < p.Cout;
            const int cbs = chan_ok ? cb : 0;
            f32x4 mu[2], sc[2], sh[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                mu[h] = *reinterpret_cast<const f32x4*>(p.bmean + cbs + 4 * h);
                sc[h] = *reinterpret_cast<const f32x4*>(p.bscale + cbs + 4 * h);
                sh[h] = *reinterpret_cast<const f32x4*>(p.bshift + cbs + 4 * h);
            }
            float sq[2][8];                                 // this group's 8 channels: sum(du), sum(du * (z - mean)) over the lane's two pixels
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const u32x4 zv = *reinterpret_cast<const u32x4*>(p.bz + zoff[i] + cbs);
                float w[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][j][8 * kp + e]), __float_as_uint(acc[i][j][8 * kp + 4 + e]), false, false);
                    w[e] = __uint_as_float(sw[0]);
                    w[4 + e] = __uint_as_float(sw[1]);
                }
                if (has_res) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        w[2 * e] += HTraits<T>::to_f32((unsigned short)(rr[i][j][kp][e] & 0xffffu));
                        w[2 * e + 1] += HTraits<T>::to_f32((unsigned short)(rr[i][j][kp][e] >> 16));
                    }
                }
                const float live = (mpix[i] >= 0 && chan_ok) ? 1.f : 0.f;
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = pack2<T>(w[2 * e], w[2 * e + 1]);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int c = 2 * e + h;
                        const float r = HTraits<T>::to_f32((unsigned short)(h ? o[e] >> 16 : o[e] & 0xffffu));
                        const float zc = HTraits<T>::to_f32((unsigned short)(h ? zv[e] >> 16 : zv[e] & 0xffffu)) - mu[c >> 2][c & 3];
                        const float du = r * act_grad_c<ACT>(zc * sc[c >> 2][c & 3] + sh[c >> 2][c & 3]) * live;
                        sq[0][c] = i == 0 ? du : sq[0][c] + du;
                        sq[1][c] = i == 0 ? du * zc : __builtin_fmaf(du, zc, sq[1][c]);
                    }
                }
                if (mpix[i] >= 0 && chan_ok) *reinterpret_cast<u32x4*>(yo + ooff[i] + j * 64 + kp * 16) = o;
            }
            // the 32 pixels of this half, per group (16 live values instead of 64 for all four groups at once - the kernel must
            // stay under 256 VGPRs): reduce-scatter as in stats_reduce_store, pairing (quantity), (c, c+4), (c, c+2), (c, c+1)
            float l8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(sq[0][e]), __float_as_uint(sq[1][e]), false, false);
                l8[e] = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
            }
            float l4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t0 = l8[e] + dpp_f<0x140>(l8[e]);
                const float t1 = l8[e + 4] + dpp_f<0x140>(l8[e + 4]);
                l4[e] = b3 ? t1 : t0;
            }
            float l2[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float t0 = l4[e] + dpp_f<0x141>(l4[e]);
                const float t1 = l4[e + 2] + dpp_f<0x141>(l4[e + 2]);
                l2[e] = b2 ? t1 : t0;
            }
            const float t0 = l2[0] + dpp_f<0x4E>(l2[0]);
            const float t1 = l2[1] + dpp_f<0x4E>(l2[1]);
            float l1 = b1 ? t1 : t0;
            l1 += dpp_f<0xB1>(l1);
            if (!(lane & 1)) srow[cb] = l1;                // stats_ld covers the padded channel tiles
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- epilogue of the FUSED stride-2 input gradient (conv1_dma_h16<GATH = 2>): the GEMM's output channel n = class * C + c
// (class = (ph, pw) parity of the dx pixel inside the 2 x 2 block of dz pixel m, C = p.H channels of dx), identity epilogue,
// optional accumulate into what is already there (p.res / r_ld / r_off address the same pixels of the running gradient).
// Each lane holds 8 consecutive n per (j, kp): one class, 8 consecutive channels -> a 16-byte store at pixel (2 row + ph, 2 col + pw).
template <typename T, int BN>
__device__ __forceinline__ void d_epilogue_s2g(const ConvHArgs& p, const f32x16 (&acc)[2][BN / 64], const int (&mpix)[2], int ch0) {
    constexpr int TN = BN / 64;
    const bool has_res = p.flags & YOLO_FLAG_RESIDUAL;
    unsigned short* yo = reinterpret_cast<unsigned short*>(p.y);
    const int W2 = 2 * p.Win;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = mpix[i] < 0 ? 0 : mpix[i];
        const int img = fdiv(m, p.mg_PC, p.PC), rem = m - img * p.PC;
        const int row = fdiv(rem, p.mg_TW, p.TW), col = rem - row * p.TW;
        const size_t blk = (size_t)(img * 2 * p.Hin + 2 * row) * W2 + 2 * col;          // dx pixel (2 row, 2 col)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                float w[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][j][8 * kp + e]), __float_as_uint(acc[i][j][8 * kp + 4 + e]), false, false);
                    w[e] = __uint_as_float(sw[0]);
                    w[4 + e] = __uint_as_float(sw[1]);
                }
                const int nb = ch0 + j * 64 + kp * 16;
                const int cls = fdiv(nb, p.mg_H, p.H), c = nb - cls * p.H;
                const size_t pix = blk + (size_t)(cls >> 1) * W2 + (cls & 1);
                if (mpix[i] < 0 || nb >= p.Cout) continue;
                if (has_res) {
                    const u32x4 r4 = *reinterpret_cast<const u32x4*>(p.res + pix * p.r_ld + p.r_off + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        w[2 * e] += HTraits<T>::to_f32((unsigned short)(r4[e] & 0xffffu));
                        w[2 * e + 1] += HTraits<T>::to_f32((unsigned short)(r4[e] >> 16));
                    }
                }
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = pack2<T>(w[2 * e], w[2 * e + 1]);
                *reinterpret_cast<u32x4*>(yo + pix * p.y_ld + p.y_off + c) = o;
            }
    }
}

}  // namespace yolo
