// conv_f32.hip — fp32 implicit-GEMM convolution on the gfx950 f32 matrix cores.
//
// Replaces (reference file:line): CNNBlock.forward  code/model.py:80-86  (Conv2d -> BN(eval) ->
// LeakyReLU/Mish, or bare Conv2d+bias), the residual add of ResidualBlock.forward :115-121, the
// nn.Upsample + torch.cat writer of YOLOv3.forward :189-191 and the head reshape/permute :145-148.
//
// GEMM view:  M = N*Ho*Wo output pixels, N = Cout, K = k*k*Cin with K index (kh, kw, ci).
// A (activations, NHWC) is gathered straight from HBM/L2 into LDS — no im2col buffer: one
// 32-wide K step lies inside a single filter tap because Cin % 32 == 0 for every layer but the
// first (Cin = 3 padded to 4, where each 16-byte chunk is one tap).  B is the packed weight
// matrix [Cout_pad][K_pad] (yolo_pack_weights).  Arithmetic: v_mfma_f32_32x32x2_f32, exact
// fp32 products and fp32 accumulation (bit-for-bit an fmaf chain), which is what lets the fp32
// path meet the 1e-3 parity bar with margin.
//
// Block = 256 threads = 4 waves (2 x 2), wave tile = (BM/2) x (BN/2) built from 32x32 MFMA
// tiles.  LDS rows are 32 floats padded to 36 so the ds_read_b128 fragment reads of 16 lanes
// (16 different rows, same column chunk) hit 16 different 16-byte slots.  Register-staged
// double buffering: global loads of step t+1 are issued before the MFMAs of step t and written
// to the other LDS buffer after them; one barrier per K step.
//
// Bits against conv_patch_f32 (conv_f32_v2.hip), which adds the same products in the same order where cin == 32 or ksize == 1:
// identical, except for Mish on the element-by-element path of conv_f32_epilogue (cout % 4 != 0, a y / residual view that is no
// multiple of 4, the head layout). There the activation runs on the accumulator registers and hipcc vectorises Mish's n = e (e + 2),
// n + 2 into v_pk_mul_f32 + v_add_f32 (two roundings); on the 16-byte path, and everywhere in conv_patch_f32, it runs on the way into
// the LDS transpose and n + 2 becomes one v_fma_f32 (one rounding). The results differ in their last bits, both within the fp64
// bound of tests/test_gpu_conv_f32_edges.py.
#include "conv_f32_epilogue.h"

namespace yolo {

constexpr int LDS_LD = 36;   // padded row length (floats)


template <int BM, int BN, bool SMALLC>
__global__ __launch_bounds__(256) void conv_igemm_f32(const ConvArgs p) {
    constexpr int WM = BM / 2, WN = BN / 2;      // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;    // 32x32 MFMA tiles per wave
    constexpr int RA = BM / 32, RB = BN / 32;    // rows staged per thread
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* As = reinterpret_cast<float*>(smem_raw);              // [2][BM][LDS_LD]
    float* Bs = As + 2 * BM * LDS_LD;                            // [2][BN][LDS_LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_n = blockIdx.x % p.tiles_n;
    const int tile_m = blockIdx.x / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---------------------------------------------------------------- staging geometry
    const int chunk = tid & 7;       // 16-byte chunk inside the 32-float K step
    const int lrow = tid >> 3;       // 0..31
    long long a_base[RA];
    unsigned a_mask[RA];
    const int HoWo = p.Ho * p.Wo;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + lrow + 32 * i;
        const bool mv = m < p.M;
        const int mm = mv ? m : 0;
        const int n = mm / HoWo;
        const int rem = mm - n * HoWo;
        const int ho = rem / p.Wo;
        const int wo = rem - ho * p.Wo;
        const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
        a_base[i] = ((long long)(n * p.H + hi0) * p.W + wi0) * p.x_ld + p.x_off;
        unsigned mk = 0;
        for (int kh = 0; kh < p.ks; ++kh)
            for (int kw = 0; kw < p.ks; ++kw)
                if (mv && (unsigned)(hi0 + kh) < (unsigned)p.H && (unsigned)(wi0 + kw) < (unsigned)p.W)
                    mk |= 1u << (kh * p.ks + kw);
        a_mask[i] = mk;
    }
    const float* wrow = p.w + (size_t)(n0 + lrow) * p.Kpad + chunk * 4;

    f32x4 ra[RA], rb[RB];
    auto load_global = [&](int kt) {
        int tap, coff;
        if (SMALLC) {
            tap = kt * 8 + chunk;
            coff = 0;
        } else {
            const int kg = kt * BK;
            tap = kg / p.Cin;
            coff = kg - tap * p.Cin + chunk * 4;
        }
        const int kh = tap / p.ks, kw = tap - kh * p.ks;
        const long long toff = (long long)(kh * p.W + kw) * p.x_ld + coff;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const bool v = (tap < 9) && ((a_mask[i] >> tap) & 1u);
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            ra[i] = v ? *reinterpret_cast<const f32x4*>(p.x + a_base[i] + toff) : z;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
            rb[i] = *reinterpret_cast<const f32x4*>(wrow + (size_t)(32 * i) * p.Kpad + kt * BK);
    };
    auto store_lds = [&](int buf) {
        float* a = As + buf * BM * LDS_LD + lrow * LDS_LD + chunk * 4;
        float* b = Bs + buf * BN * LDS_LD + lrow * LDS_LD + chunk * 4;
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(a + 32 * i * LDS_LD) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(b + 32 * i * LDS_LD) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read offsets: lane l -> row (l & 31), K chunk 4*(l >> 5) inside each 8-wide sub-step
    const int frow = lane & 31, fh = lane >> 5;
    const int a_frag = (wm * WM + frow) * LDS_LD + 4 * fh;
    const int b_frag = (wn * WN + frow) * LDS_LD + 4 * fh;

    load_global(0);
    store_lds(0);
    __syncthreads();

    for (int kt = 0; kt < p.KT; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < p.KT) load_global(kt + 1);
        const float* Ab = As + cur * BM * LDS_LD + a_frag;
        const float* Bb = Bs + cur * BN * LDS_LD + b_frag;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDS_LD + s * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDS_LD + s * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < p.KT) store_lds(cur ^ 1);
        __syncthreads();
    }

    // ---------------------------------------------------------------------- epilogue (conv_f32_epilogue.h)
    conv_f32_epilogue<BM, BN>(p, acc, As, m0, n0);   // As: [BM][BN + 4] floats <= 2 * (BM + BN) * LDS_LD, idle behind the last barrier
}

// ------------------------------------------------------------------------------ host side
static size_t lds_bytes(int bm, int bn) { return (size_t)2 * (bm + bn) * LDS_LD * sizeof(float); }

template <int BM, int BN>
static int launch_tile(const ConvArgs& a, bool smallc, hipStream_t s) {
    const int tiles_m = ceil_div(a.M, BM);
    ConvArgs p = a;
    p.tiles_n = ceil_div(a.Cout, BN);
    dim3 grid(tiles_m * p.tiles_n), block(256);
    const size_t lds = lds_bytes(BM, BN);
    if (smallc)
        hipLaunchKernelGGL((conv_igemm_f32<BM, BN, true>), grid, block, lds, s, p);
    else
        hipLaunchKernelGGL((conv_igemm_f32<BM, BN, false>), grid, block, lds, s, p);
    return check_launch("conv_igemm_f32");
}

int conv_igemm_launch(const ConvArgs& a, int tile, hipStream_t s) {
    const bool smallc = a.Cin == 4;       // the stem's 3 channels padded: each 16-byte chunk of a K step is one filter tap
    switch (tile) {
        case kTileF32Reg128x128: return launch_tile<128, 128>(a, smallc, s);
        case kTileF32Reg128x64: return launch_tile<128, 64>(a, smallc, s);
        case kTileF32Reg64x128: return launch_tile<64, 128>(a, smallc, s);
        default: return launch_tile<64, 64>(a, smallc, s);
    }
}

}  // namespace yolo
