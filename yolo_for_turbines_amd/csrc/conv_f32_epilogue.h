// conv_f32_epilogue.h — what the fp32 implicit-GEMM kernels of conv_f32.hip (exact f32 products) and conv_split3_f32.hip
// (three-way bf16 split products) share: the launch arguments and the epilogue (conv_splitk_f32.hip takes the arguments; its
// combine pass ends in the epilogue's per-pixel stores, conv_f32_store4 / conv_f32_store1). Both accumulate 32x32 MFMA tiles whose C/D
// layout is the same, so scale / shift / activation, the transpose through LDS, residual, 2x upsampling store, head layout and
// NaN flag are one piece of code.
#pragma once
#include "common.h"

namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
    const float* x;
    const float* w;
    const char* w_planes;    // conv_split3_f32 on prepared weights: the bf16 planes behind w (else null)
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    int* nan_flag;
    int N, H, W, Cin, Cout, Ho, Wo, M;
    int ks, stride, pad;
    int x_ld, x_off, y_ld, y_off, r_ld, r_off;
    int Kpad, KT;
    int act, out_mode, flags;
    int nc5;
    int tiles_n;
};

constexpr int BK = 32;       // one K step: 32 consecutive input channels of one filter tap

int conv_igemm_launch(const ConvArgs& a, int tile, hipStream_t s);   // conv_f32.hip: tile is one of kTileF32Reg*, anything else runs 64x64

// conv_split3_f32.hip (fp32 operands split into three bf16 each, six bf16 MFMAs per product; YOLO_FLAG_SPLIT_BF16)
bool split3_supported(const yolo_conv_desc* d);
bool split3_eligible(const yolo_conv_desc* d);
// a.w_planes set: a.w is the buffer split3_weights_launch made (YOLO_FLAG_SPLIT_WEIGHTS_READY), the planes in its tail (packed_f32)
int conv_split3_launch(const ConvArgs& a, int tile, hipStream_t s);
size_t split3_weight_bytes(const yolo_conv_desc* d);
int split3_weights_launch(const yolo_conv_desc* d, const void* w_packed, void* out, hipStream_t s);

// conv_splitk_f32.hip (exact f32 products, K cut into slices whose partial sums a second launch combines; YOLO_FLAG_SPLIT_K)
bool splitk_supported(const yolo_conv_desc* d);
bool splitk_eligible(const yolo_conv_desc* d);
int splitk_slices(const yolo_conv_desc* d, int* steps);          // S; *steps = K steps of 32 per slice
size_t splitk_workspace_bytes(const yolo_conv_desc* d);
int conv_splitk_launch(const ConvArgs& a, const yolo_conv_desc* d, void* ws, size_t ws_bytes, hipStream_t s);

// What follows scale / shift / activation for one output pixel m (shared by conv_f32_epilogue and splitk_combine_f32, so the store
// paths exist once): residual, NaN check, store. conv_f32_store4: channels n .. n + 3 as one 16-byte piece, YOLO_OUT_NHWC or
// YOLO_OUT_UPSAMPLE2X with y / residual views that are multiples of 4. conv_f32_store1: one channel, any output mode
// (head_a, head_k = n / nc5, n % nc5 for YOLO_OUT_HEAD).
__device__ __forceinline__ void conv_f32_store4(const ConvArgs& p, int m, int n, f32x4 v, int HoWo, bool has_res, bool nan_chk, bool& saw_nan) {
    if (has_res) v += *reinterpret_cast<const f32x4*>(p.res + (size_t)m * p.r_ld + p.r_off + n);
    if (nan_chk && (v[0] != v[0] || v[1] != v[1] || v[2] != v[2] || v[3] != v[3])) saw_nan = true;
    if (p.out_mode == YOLO_OUT_NHWC) {
        *reinterpret_cast<f32x4*>(p.y + (size_t)m * p.y_ld + p.y_off + n) = v;
    } else {                                        // YOLO_OUT_UPSAMPLE2X
        const int img = m / HoWo;
        const int rem = m - img * HoWo;
        const int ho = rem / p.Wo;
        const int wo = rem - ho * p.Wo;
        const int W2 = 2 * p.Wo;
        float* d = p.y + ((size_t)(img * 2 * p.Ho + 2 * ho) * W2 + 2 * wo) * p.y_ld + p.y_off + n;
        *reinterpret_cast<f32x4*>(d) = v;
        *reinterpret_cast<f32x4*>(d + p.y_ld) = v;
        *reinterpret_cast<f32x4*>(d + (size_t)W2 * p.y_ld) = v;
        *reinterpret_cast<f32x4*>(d + (size_t)(W2 + 1) * p.y_ld) = v;
    }
}

__device__ __forceinline__ void conv_f32_store1(const ConvArgs& p, int m, int n, float v, int HoWo, int head_a, int head_k, bool has_res,
                                                bool nan_chk, bool& saw_nan) {
    if (has_res) v += p.res[(size_t)m * p.r_ld + p.r_off + n];
    if (nan_chk && v != v) saw_nan = true;
    if (p.out_mode == YOLO_OUT_NHWC) {
        p.y[(size_t)m * p.y_ld + p.y_off + n] = v;
    } else {
        const int img = m / HoWo;
        const int rem = m - img * HoWo;
        const int ho = rem / p.Wo;
        const int wo = rem - ho * p.Wo;
        if (p.out_mode == YOLO_OUT_UPSAMPLE2X) {
            const int W2 = 2 * p.Wo;
            float* d = p.y + ((size_t)(img * 2 * p.Ho + 2 * ho) * W2 + 2 * wo) * p.y_ld + p.y_off + n;
            d[0] = v;
            d[p.y_ld] = v;
            d[(size_t)W2 * p.y_ld] = v;
            d[(size_t)(W2 + 1) * p.y_ld] = v;
        } else {  // YOLO_OUT_HEAD: (B,3,g,g,5+nc)
            p.y[((size_t)((img * 3 + head_a) * p.Ho + ho) * p.Wo + wo) * p.nc5 + head_k] = v;
        }
    }
}

// Epilogue of a BM x BN block of 256 threads = 2 x 2 waves with (BM/2) x (BN/2) wave tiles of 32x32 MFMA tiles.
// C/D map of the 32x32 tile: column (N = cout) = lane & 31, row (M = pixel) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
// `ost` is LDS of at least BM * (BN + 4) floats that every wave has finished reading (a barrier lies behind the last read).
template <int BM, int BN>
__device__ __forceinline__ void conv_f32_epilogue(const ConvArgs& p, f32x16 (&acc)[BM / 64][BN / 64], float* ost, int m0, int n0) {
    constexpr int WM = BM / 2, WN = BN / 2;
    constexpr int TM = WM / 32, TN = WN / 32;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int frow = lane & 31, fh = lane >> 5;
    const int HoWo = p.Ho * p.Wo;
    const bool has_res = p.flags & YOLO_FLAG_RESIDUAL;
    const bool nan_chk = p.flags & YOLO_FLAG_NANCHECK;
    bool saw_nan = false;
    // NHWC outputs with cout % 4 == 0 (every BN block): scale/shift/activation in registers, transpose the BM x BN tile
    // through the (now idle) operand LDS, and let every lane move 16 contiguous bytes of one pixel row. The direct stores
    // below are 4-byte pieces of different rows per lane; on the short 1x1 blocks they were most of the block's life.
    const bool aligned4 = ((p.y_ld | p.y_off) & 3) == 0 && (!has_res || ((p.r_ld | p.r_off) & 3) == 0);
    if (p.out_mode != YOLO_OUT_HEAD && (p.Cout & 3) == 0 && aligned4) {
        constexpr int OLD = BN + 4;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WN + j * 32 + frow;
            const bool nv = n < p.Cout;
            const float sc = nv ? p.scale[n] : 0.f;
            const float sh = nv ? p.shift[n] : 0.f;
            float* dst = ost + wn * WN + j * 32 + frow;
            YOLO_SWITCH_ACT(p.act,
                _Pragma("unroll") for (int i = 0; i < TM; ++i)
                    _Pragma("unroll") for (int r = 0; r < 16; ++r) {
                        const int row = wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                        dst[row * OLD] = act_c<ACT>(acc[i][j][r] * sc + sh);
                    })
        }
        __syncthreads();
        constexpr int C4 = BN / 4;
#pragma unroll 4
        for (int idx = tid; idx < BM * C4; idx += 256) {
            const int row = idx / C4, c4 = idx - row * C4;
            const int m = m0 + row, n = n0 + c4 * 4;
            if (m >= p.M || n >= p.Cout) continue;
            conv_f32_store4(p, m, n, *reinterpret_cast<const f32x4*>(ost + row * OLD + c4 * 4), HoWo, has_res, nan_chk, saw_nan);
        }
        if (nan_chk && saw_nan) atomicOr(p.nan_flag, 2);
        return;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WN + j * 32 + frow;
        const bool nv = n < p.Cout;
        const float sc = nv ? p.scale[n] : 0.f;
        const float sh = nv ? p.shift[n] : 0.f;
        int head_a = 0, head_k = 0;
        if (p.out_mode == YOLO_OUT_HEAD) {
            head_a = n / p.nc5;
            head_k = n - head_a * p.nc5;
        }
        YOLO_SWITCH_ACT(p.act,                          // activation chosen once, outside the element loops
            _Pragma("unroll") for (int i = 0; i < TM; ++i)
                _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[i][j][r] = act_c<ACT>(acc[i][j][r] * sc + sh);)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (m >= p.M || !nv) continue;
                conv_f32_store1(p, m, n, acc[i][j][r], HoWo, head_a, head_k, has_res, nan_chk, saw_nan);
            }
        }
    }
    if (nan_chk && saw_nan) atomicOr(p.nan_flag, 2);
}

}  // namespace yolo
