// =====================================================================================================
// conv3_ws_h16 (round 3): the 3x3 layers with <= 64 input AND output channels (32 -> 64 at 208^2, its input gradient 64 -> 32,
// the stride-2 32 -> 64 at 416 -> 208^2), weights in REGISTERS.
// conv_patch_h16_n64 gives such a layer one 128-pixel tile per block: 36 MFMAs of matrix work per wave behind a prologue of index
// arithmetic, a register-staged patch and an LDS round trip - 173 us for a layer whose bytes take ~85 us (32 -> 64 with the
// residual) and whose matrix work takes ~25. These layers are a stream: the whole filter bank is 36 KB, so
//   * a wave keeps ALL weight fragments in registers (9 taps x Cin/16 k-steps x Cout/32 n-tiles x 4 VGPRs = 144) for the lifetime
//     of a PERSISTENT workgroup (2 per CU) and walks 8 x 16-pixel output tiles;
//   * the tile's input patch with halo ((8s+1... ) x (16s+...) pixels, s = stride) arrives by LDS-DMA into a double buffer while
//     the previous tile is multiplied: one wait + ONE barrier per tile, placed between the MFMA phase and the epilogue, so the
//     stores of tile t overlap the request and the matrix work of tile t + 1;
//   * patch rows are Cin x 2 bytes with the 16-byte chunks XOR-swizzled on the DMA's source side (by (p >> 2) & 3 for 64-byte
//     rows, (p >> 1) & 7 for 128-byte rows): 16 consecutive pixels cover all banks (stride 2: two-way);
//   * operand swap as in the other DMA kernels: weights = A, pixels = B, D = [channel][pixel]; one v_permlane32_swap per register
//     pair leaves a lane with 8 consecutive channels of its pixel: 16-byte stores / residual loads.
// Halo pixels outside the image read the zero page.
#include "h16.h"

namespace yolo {

constexpr int WS_TH = 8, WS_TW = 16;
struct ConvWsArgs {
    const unsigned short* x;
    const unsigned short* wf;
    const float* scale;
    const float* shift;
    const unsigned short* res;
    unsigned short* y;
    int* nan_flag;
    int N, Hin, Win, Ho, Wo;
    int x_ld, x_off, y_ld, y_off, r_ld, r_off;
    int Cout, KT, act, flags;
    int tiles_w, tiles_per_img, total_tiles;
    unsigned mg_tpi, mg_tw;
    float* stats;                         // STATS instances (train-mode forward): per-wave BatchNorm partial sums [row][2][stats_ld]
    int stats_ld;
};

// STATS = true (ACT none, no residual): raw z AND the BatchNorm partial sums of the rounded values (d_epilogue_stats). A wave
// keeps ONE running pair of sums per channel for all its tiles: per tile and 8-channel group the 32 pixel lanes of a half are
// folded by the reduce-scatter butterfly of d_epilogue_bstats (16 live values) and the result is added into the wave's private
// [2][32 NT] LDS accumulator with ds_add_f32 (one lane per address and tile: a fixed order); the accumulator is the wave's row.
template <typename T, int CIN, int NT, int STRIDE, int ACT, bool RES, bool STATS = false>
__global__ __launch_bounds__(256, 2) void conv3_ws_h16(const ConvWsArgs p) {
    typedef typename HTraits<T>::vec vec;
    constexpr int PR = STRIDE * (WS_TH - 1) + 3, PC = STRIDE * (WS_TW - 1) + 3, P = PR * PC;
    constexpr int RB = CIN * 2, CH = CIN / 8;                         // bytes and 16-byte chunks per patch pixel
    constexpr int KS16 = CIN / 16;                                     // k16 steps per tap
    constexpr int NCHUNK = P * CH, ROUNDS = (NCHUNK + 255) / 256;
    constexpr int BUF = ((P * RB + 255) / 256) * 256;
    extern __shared__ __attribute__((aligned(256))) char smem_raw[];   // [2][BUF] patches | [NT * 32] scale | [NT * 32] shift
    float* sstab = reinterpret_cast<float*>(smem_raw + 2 * BUF);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hl = lane >> 5, pl = lane & 31;
    float* wsum = sstab + 2 * NT * 32 + wave * (2 * NT * 32);          // STATS: this wave's [2][NT * 32] sums
    if (STATS) {
        for (int i = lane; i < 2 * NT * 32; i += 64) wsum[i] = 0.f;
    }

    // ---- the filter bank, once
    u32x4 wreg[NT][9 * KS16];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int cs = 0; cs < KS16; ++cs) {
                const int kt = (cs >> 1) * 9 + tap, sh = cs & 1;
                wreg[nt][tap * KS16 + cs] = *reinterpret_cast<const u32x4*>(p.wf + ((size_t)nt * p.KT + kt) * 1024 + sh * 512 + lane * 8);
            }
    if (!STATS && tid < NT * 32) {
        const int c = tid < p.Cout ? tid : p.Cout - 1;
        sstab[tid] = tid < p.Cout ? p.scale[c] : 0.f;
        sstab[NT * 32 + tid] = tid < p.Cout ? p.shift[c] : 0.f;
    }

    auto swz = [](int pp) { return CH == 4 ? (pp >> 2) & 3 : (pp >> 1) & 7; };
    // request the patch of tile t into buffer b: ROUNDS wave-instructions of 64 x 16 bytes, lane-linear in LDS
    // (__device__: a file-local __device__ variable named by an unmarked lambda counts as used by the host; hipcc then gives
    // it external linkage and addresses the zero page through the GOT)
    auto request = [&] __device__ (int t, char* dst) {
        const int img = fdiv(t, p.mg_tpi, p.tiles_per_img), rem = t - img * p.tiles_per_img;
        const int th = fdiv(rem, p.mg_tw, p.tiles_w), tw = rem - th * p.tiles_w;
        const int hi0 = th * WS_TH * STRIDE - 1, wi0 = tw * WS_TW * STRIDE - 1;
        const unsigned short* zp = reinterpret_cast<const unsigned short*>(g_zero_page) + (lane & 7) * 8;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int idx = r * 256 + tid;
            if (idx < NCHUNK) {
                const int pp = idx / CH, sl = idx - pp * CH;
                const int pr = pp / PC, pc = pp - pr * PC;
                const int hi = hi0 + pr, wi = wi0 + pc;
                const bool ok = (unsigned)hi < (unsigned)p.Hin && (unsigned)wi < (unsigned)p.Win;
                const unsigned short* src = p.x + ((size_t)(img * p.Hin + hi) * p.Win + wi) * p.x_ld + p.x_off + ((sl ^ swz(pp)) * 8);
                glds16(ok ? src : zp, dst + (r * 256 + wave * 64) * 16);
            }
        }
    };

    // this lane's output pixel inside a tile, and its patch pixel for tap (0, 0)
    const int r_o = 2 * wave + (pl >> 4), c_o = pl & 15;
    const int p0 = (r_o * STRIDE) * PC + c_o * STRIDE;
    const int stride_t = gridDim.x;
    int t = blockIdx.x;
    if (t >= p.total_tiles) return;
    request(t, smem_raw);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    bool saw_nan = false;
    for (int it = 0; t < p.total_tiles; t += stride_t, ++it) {
        char* cur = smem_raw + (it & 1) * BUF;
        if (t + stride_t < p.total_tiles) request(t + stride_t, smem_raw + ((it + 1) & 1) * BUF);
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int pp = p0 + (tap / 3) * PC + (tap % 3);
            const int f = swz(pp);
            const char* row = cur + pp * RB;
#pragma unroll
            for (int cs = 0; cs < KS16; ++cs) {
                const u32x4 a = *reinterpret_cast<const u32x4*>(row + (((cs * 2 + hl) ^ f) << 4));
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = HTraits<T>::mfma(__builtin_bit_cast(vec, wreg[nt][tap * KS16 + cs]), __builtin_bit_cast(vec, a), acc[nt]);
            }
        }
        // the next tile's patch has had the whole matrix phase to land; everybody is done reading `cur`
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // ---- epilogue (registers -> 16-byte stores), overlapping the next tile's request and matrix phase
        const int img = fdiv(t, p.mg_tpi, p.tiles_per_img), rem = t - img * p.tiles_per_img;
        const int th = fdiv(rem, p.mg_tw, p.tiles_w), tw = rem - th * p.tiles_w;
        const int ho = th * WS_TH + r_o, wo = tw * WS_TW + c_o;
        const bool live = ho < p.Ho && wo < p.Wo;
        const size_t m = ((size_t)img * p.Ho + (live ? ho : 0)) * p.Wo + (live ? wo : 0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float v[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 sc = *reinterpret_cast<const f32x4*>(sstab + nt * 32 + 8 * g + 4 * hl);
                const f32x4 sf = *reinterpret_cast<const f32x4*>(sstab + NT * 32 + nt * 32 + 8 * g + 4 * hl);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * g + e] = STATS ? acc[nt][4 * g + e] : act_c<ACT>(acc[nt][4 * g + e] * sc[e] + sf[e]);
            }
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                float w[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[8 * kp + e]), __float_as_uint(v[8 * kp + 4 + e]), false, false);
                    w[e] = __uint_as_float(sw[0]);
                    w[4 + e] = __uint_as_float(sw[1]);
                }
                const int ch = nt * 32 + kp * 16 + 8 * hl;
                const bool ok = live && ch < p.Cout;
                if (RES && ok) {
                    const u32x4 r4 = *reinterpret_cast<const u32x4*>(p.res + m * p.r_ld + p.r_off + ch);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        w[2 * e] += HTraits<T>::to_f32((unsigned short)(r4[e] & 0xffffu));
                        w[2 * e + 1] += HTraits<T>::to_f32((unsigned short)(r4[e] >> 16));
                    }
                }
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    saw_nan |= __builtin_isunordered(w[2 * e], w[2 * e + 1]);
                    o[e] = pack2<T>(w[2 * e], w[2 * e + 1]);
                }
                if (ok) *reinterpret_cast<u32x4*>(p.y + m * p.y_ld + p.y_off + ch) = o;
                if constexpr (STATS) {
                    const float lv = ok ? 1.f : 0.f;
                    float sq[2][8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float r0 = HTraits<T>::to_f32((unsigned short)(o[e] & 0xffffu)) * lv;
                        const float r1 = HTraits<T>::to_f32((unsigned short)(o[e] >> 16)) * lv;
                        sq[0][2 * e] = r0; sq[0][2 * e + 1] = r1;
                        sq[1][2 * e] = r0 * r0; sq[1][2 * e + 1] = r1 * r1;
                    }
                    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
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
                    const float u0 = l2[0] + dpp_f<0x4E>(l2[0]);
                    const float u1 = l2[1] + dpp_f<0x4E>(l2[1]);
                    float l1 = b1 ? u1 : u0;
                    l1 += dpp_f<0xB1>(l1);
                    // lane: quantity (lane >> 4) & 1, channel nt * 32 + kp * 16 + 8 hl + 4 b3 + 2 b2 + b1; the odd lane of a pair is a duplicate
                    if (!(lane & 1))
                        atomicAdd(wsum + ((lane >> 4) & 1) * (NT * 32) + nt * 32 + kp * 16 + 8 * hl + (b3 ? 4 : 0) + (b2 ? 2 : 0) + (b1 ? 1 : 0), l1);
                }
            }
        }
    }
    if ((p.flags & YOLO_FLAG_NANCHECK) && saw_nan) atomicOr(p.nan_flag, 2);
    if constexpr (STATS) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int row = blockIdx.x * 4 + wave;
        for (int i = lane; i < 2 * NT * 32; i += 64) {
            const int qty = i / (NT * 32), c = i - qty * (NT * 32);
            p.stats[((size_t)row * 2 + qty) * p.stats_ld + c] = wsum[i];
        }
    }
}

bool ws_eligible(const yolo_conv_desc* d, const void* residual) {
    if (d->tile != kTileH16Ws && (switches().no_conv3_ws || d->tile != 0)) return false;
    if (d->ksize != 3 || d->out_mode != YOLO_OUT_NHWC || d->dtype == YOLO_F32) return false;
    const bool shape = (d->stride == 1 && ((d->cin == 32 && d->cout > 32 && d->cout <= 64) || (d->cin == 64 && d->cout <= 32))) ||
                       (d->stride == 2 && d->cin == 32 && d->cout > 32 && d->cout <= 64);
    if (!shape || d->cout % 8) return false;
    if ((d->x_ld & 7) || (d->x_off & 7) || (d->y_ld & 7) || (d->y_off & 7)) return false;
    if (residual && ((d->r_ld & 7) || (d->r_off & 7))) return false;
    if (d->stride == 2 && ((d->h & 1) || (d->w & 1))) return false;
    return true;
}

static int ws_grid(int total_tiles) { return total_tiles < 512 ? total_tiles : 512; }   // two persistent workgroups per CU

// train-mode forward: one row of BatchNorm partial sums per wave
int ws_stats_rows(const yolo_conv_desc* d) {
    const int ho = (d->h + 2 - 3) / d->stride + 1, wo = (d->w + 2 - 3) / d->stride + 1;
    const long long total = (long long)ceil_div(wo, WS_TW) * ceil_div(ho, WS_TH) * d->n;
    return total <= 0x7fffffffLL ? 4 * ws_grid((int)total) : 0;
}

template <typename T, int CIN, int NT, int STRIDE>
static int launch_ws(ConvWsArgs& a, hipStream_t s) {
    constexpr int PR = STRIDE * (WS_TH - 1) + 3, PC = STRIDE * (WS_TW - 1) + 3;
    constexpr int BUF = ((PR * PC * CIN * 2 + 255) / 256) * 256;
    const size_t lds = 2 * (size_t)BUF + (2 + 8) * NT * 32 * sizeof(float);     // patches | scale, shift | 4 waves x [2][NT * 32] sums
    const int grid = ws_grid(a.total_tiles);
    const bool res = a.flags & YOLO_FLAG_RESIDUAL;
    auto go = [&](auto kern) -> int {
        static LdsOnce once;
        if (int rc = reserve_lds(once, reinterpret_cast<const void*>(kern), lds, "conv3_ws_h16")) return rc;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
        return check_launch("conv3_ws_h16");
    };
    if (a.stats) return go(&conv3_ws_h16<T, CIN, NT, STRIDE, YOLO_ACT_NONE, false, true>);
    YOLO_SWITCH_ACT(a.act, return res ? go(&conv3_ws_h16<T, CIN, NT, STRIDE, ACT, true>) : go(&conv3_ws_h16<T, CIN, NT, STRIDE, ACT, false>));
    return fail(YOLO_ERR_ARG, "conv3_ws_h16: activation");
}

int conv_ws_launch(const yolo_conv_desc* d, const void* x, const void* wf, const float* scale, const float* shift, const void* residual,
                   void* y, int32_t* nan_flag, hipStream_t s, float* stats, int stats_ld) {
    ConvWsArgs a;
    a.stats = stats; a.stats_ld = stats_ld;
    a.x = (const unsigned short*)x; a.wf = (const unsigned short*)wf; a.scale = scale; a.shift = shift;
    a.res = (const unsigned short*)residual; a.y = (unsigned short*)y; a.nan_flag = nan_flag;
    a.N = d->n; a.Hin = d->h; a.Win = d->w;
    a.Ho = (d->h + 2 - 3) / d->stride + 1; a.Wo = (d->w + 2 - 3) / d->stride + 1;
    a.x_ld = d->x_ld; a.x_off = d->x_off; a.y_ld = d->y_ld; a.y_off = d->y_off; a.r_ld = d->r_ld; a.r_off = d->r_off;
    a.Cout = d->cout; a.KT = (d->cin / 32) * 9; a.act = d->act; a.flags = d->flags;
    a.tiles_w = ceil_div(a.Wo, WS_TW);
    a.tiles_per_img = a.tiles_w * ceil_div(a.Ho, WS_TH);
    const long long total = (long long)a.tiles_per_img * d->n;
    if (total > 0x7fffffffLL || (long long)d->n * d->h * d->w > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "conv3_ws_h16: too many pixels");
    a.total_tiles = (int)total;
    a.mg_tpi = magic_of(a.tiles_per_img); a.mg_tw = magic_of(a.tiles_w);
    if ((a.flags & YOLO_FLAG_NANCHECK) && !nan_flag) return fail(YOLO_ERR_ARG, "conv3_ws_h16: nan_flag is NULL");
    YOLO_SWITCH_H16(d->dtype,
        if (d->stride == 2) return launch_ws<T, 32, 2, 2>(a, s);
        if (d->cin == 32) return launch_ws<T, 32, 2, 1>(a, s);
        return launch_ws<T, 64, 1, 1>(a, s));
}

}  // namespace yolo
