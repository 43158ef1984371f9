// wino4_epilogue.h — what a Winograd F(4x4) GEMM kernel does behind its K loop: the arguments, the tile table, the fold of one row
// of M into the output tiles and the epilogue. The C/D layout of v_mfma_f32_16x16x32_bf16 is that of v_mfma_f32_16x16x4_f32, so
// conv_wino4_f32.hip (the f32 GEMMs) and conv_wino4s_f32.hip (the GEMMs on bf16 planes) hand over the same registers: the one text
// of this code for both.
#pragma once
#include "wino_dma.h"

namespace yolo {

__device__ constexpr float W4_AT[4][6] = {
    {1.f, 1.f, 1.f, 1.f, 1.f, 0.f},
    {0.f, 1.f, -1.f, 2.f, -0.5f, 0.f},
    {0.f, 1.f, 1.f, 4.f, 0.25f, 0.f},
    {0.f, 1.f, -1.f, 8.f, -0.125f, 1.f},
};

struct Wino4Args {
    const float* V;
    const float* U;
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    int* nan_flag;
    int T, Tpad, C4p, Cout, CoutPad;
    int th, tw, H, W;
    int y_ld, y_off, r_ld, r_off;
    int flags;
    int n_mt, n_nt;
    int n_whole;             // tile blocks 0 .. n_whole - 1 run as one workgroup each, the rest as two workgroups of 32 tiles
};

constexpr int W4_TAB = 512;              // bytes behind the ring: the epilogue's tile table

// the epilogue's table: [64] first output pixel of the tile, [64] valid rows << 4 | columns (0: no such tile, or the other
// half's); visible to everybody after the first barrier of the K loop
__device__ __forceinline__ void wino4_tile_table(const Wino4Args& p, int* tab, int tid, int mt, bool cut, int half) {
    if (tid < 64) {
        const int t = mt * 64 + tid;
        const bool tv = t < p.T && (!cut || (tid >> 5) == half);
        const int tt = tv ? t : 0;
        const int per = p.th * p.tw;
        const int n = tt / per, rem = tt - n * per;
        const int ty = rem / p.tw, tx = rem - ty * p.tw;
        const int nr = p.H - 4 * ty < 4 ? p.H - 4 * ty : 4, nc = p.W - 4 * tx < 4 ? p.W - 4 * tx : 4;
        tab[tid] = (n * p.H + 4 * ty) * p.W + 4 * tx;
        tab[64 + tid] = tv ? (nr << 4 | nc) : 0;
    }
}

// row a of M into the output tiles: t[j] = sum_b M[a][b] A^T[j][b], Y[i][j] += A^T[i][a] t[j]
template <int a>
__device__ __forceinline__ void wino4_fold_row(const f32x4 (&acc)[6][2], f32x4 (&py)[2][4][4]) {
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
        f32x4 mb[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) mb[b] = acc[b][bb];
        f32x4 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < 6; ++b)
                if (W4_AT[j][b] != 0.f) t[j] += W4_AT[j][b] * mb[b];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (W4_AT[i][a] != 0.f)
#pragma unroll
                for (int j = 0; j < 4; ++j) py[bb][i][j] += W4_AT[i][a] * t[j];
    }
    // the partial tiles wait out the next pass in the AGPR half of the register file (the accumulators and everything else
    // of the K loop use the VGPR half: 2 waves per SIMD leave 256 registers per lane in all)
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(py[bb][i][j]));
}

// ------------------------------------------------------------------ epilogue through LDS, one output row i of the tiles at a time
// ([pixel j][tile][64 + 4] over the idle ring, 16 lanes per pixel row: stores and residual loads are 256-byte runs)
// py: [tile block bb][output row i][output column j] of the lane's tile 32 wm + 16 bb + l16, its channels 16 wn + 4 kq .. + 3
template <int ACT, bool RES>
__device__ __forceinline__ void wino4_epilogue(const Wino4Args& p, char* smem, const int* tab, const f32x4 (&py)[2][4][4], int tid, int nt,
                                               int wm, int wn, int l16, int kq, bool busy) {
    constexpr int OLD = 68;
    float* ost = reinterpret_cast<float*>(smem);
    // scale / shift of the 4 channels this thread STORES (4 (tid % 16) .. of the block); requested here, not at kernel start:
    // eight registers less through the K loops
    const int c16 = tid & 15;
    const int co_t = nt * 64 + 4 * c16;
    const bool cv = co_t < p.Cout;
    const f32x4 sc_t = *reinterpret_cast<const f32x4*>(p.scale + (cv ? co_t : 0));
    const f32x4 sh_t = *reinterpret_cast<const f32x4*>(p.shift + (cv ? co_t : 0));
    // this thread's 8 rows of staged row i: pixel j = it / 2 of tile (tid / 16) + 32 (it % 2), channels 4 (tid % 16) ..
    auto row_pixels = [&](int i, int (&pix)[8], bool (&pv)[8]) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int tl = (tid >> 4) + 32 * (it & 1), j = it >> 1;
            const int fl = tab[64 + tl];
            pv[it] = cv && j < (fl & 15) && i < (fl >> 4);
            pix[it] = pv[it] ? tab[tl] + i * p.W + j : 0;
        }
    };
    // (one 64-bit base per thread, so that an access costs one multiply-add of its pixel)
    float* const ybase = p.y + p.y_off + co_t;
    const float* const rbase = RES ? p.res + p.r_off + (cv ? co_t : 0) : nullptr;
    const size_t y_ld = (size_t)p.y_ld, r_ld = (size_t)p.r_ld;
    auto request_res = [&](const int (&pix)[8], f32x4 (&rr)[8]) {
#pragma unroll
        for (int it = 0; it < 8; ++it) rr[it] = *reinterpret_cast<const f32x4*>(rbase + (size_t)pix[it] * r_ld);
    };
    // the residual runs one output row ahead: row 0 is requested before the first staging barrier, row i + 1 once row i has taken
    // its residual and before it is stored (rr is free again there, so the look-ahead costs no registers; the loads are older
    // than the stores, so waiting for them does not wait for the stores)
    f32x4 rr[8];
    if (RES) {
        int pix[8];
        bool pv[8];
        row_pixels(0, pix, pv);
        request_res(pix, rr);
    }
    __builtin_amdgcn_sched_barrier(0);
    bool saw_nan = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i > 0) __syncthreads();                                  // the previous row's staging has been read back
        if (busy) {
            float* dst = ost + (32 * wm + l16) * OLD + 16 * wn + 4 * kq;
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(dst + (j * 64 + 16 * bb) * OLD) = py[bb][i][j];
        }
        __syncthreads();
        int pix[8];
        bool pv[8];
        row_pixels(i, pix, pv);
        f32x4 va[8];
#pragma unroll
        for (int it = 0; it < 8; ++it)
            va[it] = *reinterpret_cast<const f32x4*>(ost + ((it >> 1) * 64 + (tid >> 4) + 32 * (it & 1)) * OLD + 4 * c16);
        // all eight values first, then the eight predicated stores (inside a predicated block the compiler waits for
        // everything in flight)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
#pragma unroll
            for (int e = 0; e < 4; ++e) va[it][e] = act_c<ACT>(va[it][e] * sc_t[e] + sh_t[e]);
            if (RES) va[it] += rr[it];
            saw_nan |= pv[it] & ((va[it][0] != va[it][0]) | (va[it][1] != va[it][1]) | (va[it][2] != va[it][2]) | (va[it][3] != va[it][3]));
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) asm volatile("" : "+v"(va[it]));
        if (RES && i < 3) {
            int npix[8];
            bool npv[8];
            row_pixels(i + 1, npix, npv);
            request_res(npix, rr);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int it = 0; it < 8; ++it)
            if (pv[it]) *reinterpret_cast<f32x4*>(ybase + (size_t)pix[it] * y_ld) = va[it];
    }
    if ((p.flags & YOLO_FLAG_NANCHECK) && saw_nan) atomicOr(p.nan_flag, 2);
}

}  // namespace yolo
