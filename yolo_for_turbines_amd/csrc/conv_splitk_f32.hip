// conv_splitk_f32.hip — fp32 implicit-GEMM convolution cut along K, for small batches (YOLO_FLAG_SPLIT_K).
//
// Replaces (reference file:line): what conv_f32.hip replaces - CNNBlock.forward  code/model.py:80-86, the residual add of
// ResidualBlock.forward :115-121, the nn.Upsample + torch.cat writer :189-191 and the head reshape/permute :145-148 - for the
// single-image forward of demo.py:41-42.
//
// At batch 1 a 13x13 layer is 169 pixels: 3 x 16 blocks of 64x64 on 256 CUs, each walking all of K (4,608 for 512 -> 1024 3x3) alone.
// The missing axis of parallelism is K. Two plain launches on the caller's stream, no atomics on floats, no waiting between
// workgroups:
//   conv_splitk_f32<64,64>  grid (tiles_m * tiles_n, S): conv_igemm_f32<64,64>'s block (same NHWC gather, same row-major weights,
//                           exact f32 products on v_mfma_f32_32x32x2_f32) over the K steps [s L, min((s + 1) L, KT)) of slice s; the
//                           raw 64x64 accumulators go to partial[s][m][n] in the caller's workspace ([S][M][cout_pad4] floats),
//                           transposed through the idle operand LDS so that every lane stores 16 contiguous bytes;
//   splitk_combine_f32      one lane per four channels of one output pixel: the S partials summed in ascending s, one fixed chain of
//                           adds, then conv_f32_epilogue's arithmetic and stores (scale / shift / activation, residual, NaN flag,
//                           NHWC / 2x upsampling / head layout, scalar path for cout % 4 != 0 or views that are not 16-byte aligned;
//                           the stores are conv_f32_epilogue.h's conv_f32_store4 / conv_f32_store1).
// S and L depend on the layer's shape per image only (splitk_slices): never on the batch, never on the device. An output value is
// therefore the same chain of operations whatever its image's neighbours are.
#include "conv_f32_epilogue.h"

namespace yolo {

constexpr int SK_LDS_LD = 36;          // padded LDS row (floats), as conv_igemm_f32
constexpr int SK_BM = 64, SK_BN = 64;
constexpr int SK_MAX_SLICES = 32;
constexpr int SK_MIN_STEPS = 4;        // K steps of 32 per slice, at least
constexpr int SK_TARGET_BLOCKS = 512;  // workgroups a batch-1 launch should reach: two per CU

struct SplitKArgs {
    ConvArgs p;
    float* partial;      // [S][M][ldp]
    int L;               // K steps per slice
    int S;
    int ldp;             // cout rounded up to 4
};

template <int BM, int BN>
__global__ __launch_bounds__(256) void conv_splitk_f32(const SplitKArgs q) {
    static_assert(BM == 64 && BN == 64, "one 32x32 MFMA tile per wave");
    const ConvArgs& p = q.p;
    constexpr int WM = BM / 2, WN = BN / 2;
    constexpr int RA = BM / 32, RB = BN / 32;    // rows staged per thread
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* As = reinterpret_cast<float*>(smem_raw);              // [2][BM][SK_LDS_LD]
    float* Bs = As + 2 * BM * SK_LDS_LD;                         // [2][BN][SK_LDS_LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_n = blockIdx.x % p.tiles_n;
    const int tile_m = blockIdx.x / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int slice = blockIdx.y;
    const int kt0 = slice * q.L;
    const int kt1 = min(kt0 + q.L, p.KT);

    // ---------------------------------------------------------------- staging geometry (conv_igemm_f32's)
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
    const float* wrow = p.w + (size_t)(n0 + lrow) * p.Kpad + chunk * 4;   // rows < cout_pad128: n0 + 63 < round_up(cout, 64)

    f32x4 ra[RA], rb[RB];
    auto load_global = [&](int kt) {
        const int kg = kt * BK;
        const int tap = kg / p.Cin;              // < ks * ks: Cin % 32 == 0, so Kpad = ks * ks * Cin and kt < KT
        const int coff = kg - tap * p.Cin + chunk * 4;
        const int kh = tap / p.ks, kw = tap - kh * p.ks;
        const long long toff = (long long)(kh * p.W + kw) * p.x_ld + coff;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const bool v = (a_mask[i] >> tap) & 1u;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            ra[i] = v ? *reinterpret_cast<const f32x4*>(p.x + a_base[i] + toff) : z;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
            rb[i] = *reinterpret_cast<const f32x4*>(wrow + (size_t)(32 * i) * p.Kpad + kt * BK);
    };
    auto store_lds = [&](int buf) {
        float* a = As + buf * BM * SK_LDS_LD + lrow * SK_LDS_LD + chunk * 4;
        float* b = Bs + buf * BN * SK_LDS_LD + lrow * SK_LDS_LD + chunk * 4;
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(a + 32 * i * SK_LDS_LD) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(b + 32 * i * SK_LDS_LD) = rb[i];
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // fragment read offsets: lane l -> row (l & 31), K chunk 4 * (l >> 5) inside each 8-wide sub-step
    const int frow = lane & 31, fh = lane >> 5;
    const int a_frag = (wm * WM + frow) * SK_LDS_LD + 4 * fh;
    const int b_frag = (wn * WN + frow) * SK_LDS_LD + 4 * fh;

    load_global(kt0);                            // (every slice has a step: S = ceil(KT / L))
    store_lds(0);
    __syncthreads();

    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = (kt - kt0) & 1;
        if (kt + 1 < kt1) load_global(kt + 1);
        const float* Ab = As + cur * BM * SK_LDS_LD + a_frag;
        const float* Bb = Bs + cur * BN * SK_LDS_LD + b_frag;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const f32x4 af = *reinterpret_cast<const f32x4*>(Ab + s * 8);
            const f32x4 bf = *reinterpret_cast<const f32x4*>(Bb + s * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], bf[e], acc, 0, 0, 0);
        }
        if (kt + 1 < kt1) store_lds(cur ^ 1);
        __syncthreads();
    }

    // ---------------------------------------------------------------------- raw accumulators -> partial[slice][m][n]
    // C/D map of the 32x32 tile: column (n) = lane & 31, row (m) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5). Through the operand
    // LDS (idle behind the loop's last barrier; BM * (BN + 4) floats <= 2 * (BM + BN) * SK_LDS_LD) into rows of 16-byte pieces.
    constexpr int OLD = BN + 4;
    float* ost = As;
    {
        float* dst = ost + wn * WN + frow;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * WM + (r & 3) + 8 * (r >> 2) + 4 * fh;
            dst[row * OLD] = acc[r];
        }
    }
    __syncthreads();
    constexpr int C4 = BN / 4;
    float* part = q.partial + (size_t)slice * (size_t)p.M * (size_t)q.ldp;
#pragma unroll 4
    for (int idx = tid; idx < BM * C4; idx += 256) {
        const int row = idx / C4, c4 = idx - row * C4;
        const int m = m0 + row, n = n0 + c4 * 4;
        if (m >= p.M || n >= q.ldp) continue;            // ldp % 4 == 0: a piece lies inside the row or outside it
        *reinterpret_cast<f32x4*>(part + (size_t)m * q.ldp + n) = *reinterpret_cast<const f32x4*>(ost + row * OLD + c4 * 4);
    }
}

// One lane per four channels of one output pixel. The sum over slices is one chain in ascending s; what follows is
// conv_f32_epilogue's arithmetic, in its order: act(scale * z + shift), then its per-pixel residual / NaN check / store helpers.
template <int ACT>
__global__ __launch_bounds__(256) void splitk_combine_f32(const SplitKArgs q) {
    const ConvArgs& p = q.p;
    const int c4n = q.ldp >> 2;
    const size_t total = (size_t)p.M * (size_t)c4n;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int m = (int)(idx / (size_t)c4n);
    const int n = (int)(idx - (size_t)m * (size_t)c4n) * 4;
    const size_t plane = (size_t)p.M * (size_t)q.ldp;
    const float* src = q.partial + (size_t)m * q.ldp + n;
    f32x4 z = *reinterpret_cast<const f32x4*>(src);
#pragma unroll 4
    for (int s = 1; s < q.S; ++s) z += *reinterpret_cast<const f32x4*>(src + (size_t)s * plane);

    const bool has_res = p.flags & YOLO_FLAG_RESIDUAL;
    const bool nan_chk = p.flags & YOLO_FLAG_NANCHECK;
    const int HoWo = p.Ho * p.Wo;
    bool saw_nan = false;
    const bool aligned4 = ((p.y_ld | p.y_off) & 3) == 0 && (!has_res || ((p.r_ld | p.r_off) & 3) == 0);
    if (p.out_mode != YOLO_OUT_HEAD && (p.Cout & 3) == 0 && aligned4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_c<ACT>(z[e] * p.scale[n + e] + p.shift[n + e]);
        conv_f32_store4(p, m, n, v, HoWo, has_res, nan_chk, saw_nan);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = n + e;
            if (c >= p.Cout) break;
            int head_a = 0, head_k = 0;
            if (p.out_mode == YOLO_OUT_HEAD) {
                head_a = c / p.nc5;
                head_k = c - head_a * p.nc5;
            }
            conv_f32_store1(p, m, c, act_c<ACT>(z[e] * p.scale[c] + p.shift[c]), HoWo, head_a, head_k, has_res, nan_chk, saw_nan);
        }
    }
    if (nan_chk && saw_nan) atomicOr(p.nan_flag, 2);
}

// ------------------------------------------------------------------------------ host side
bool splitk_supported(const yolo_conv_desc* d) {
    return d->dtype == YOLO_F32 && (d->ksize == 1 || d->ksize == 3) && (d->stride == 1 || d->stride == 2) && d->cin > 0 &&
           d->cin % 32 == 0 && d->cout > 0 && d->h > 0 && d->w > 0;
}

// Slices S and K steps per slice L: from the layer's shape PER IMAGE and the constants above, nothing else. The smallest S <= 32
// with which a batch-1 launch has at least SK_TARGET_BLOCKS workgroups, then L = max(SK_MIN_STEPS, ceil(KT / S)) and S = ceil(KT / L):
// every slice has a step, only the last may be short. KT <= 4 gives S = 1 (the pair then is conv_igemm_f32<64,64> in two launches).
int splitk_slices(const yolo_conv_desc* d, int* steps) {
    const int pad = d->ksize / 2;
    const int ho = (d->h + 2 * pad - d->ksize) / d->stride + 1, wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
    const long long tiles = (long long)ceil_div(ho * wo, SK_BM) * ceil_div(d->cout, SK_BN);
    const int KT = kpad_of(d->cin, d->ksize) / BK;
    long long want = (SK_TARGET_BLOCKS + tiles - 1) / tiles;
    if (want > SK_MAX_SLICES) want = SK_MAX_SLICES;
    int L = ceil_div(KT, (int)want);
    if (L < SK_MIN_STEPS) L = SK_MIN_STEPS;
    if (steps) *steps = L;
    return ceil_div(KT, L);
}

size_t splitk_workspace_bytes(const yolo_conv_desc* d) {
    const int pad = d->ksize / 2;
    const size_t ho = (d->h + 2 * pad - d->ksize) / d->stride + 1, wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
    return (size_t)splitk_slices(d, nullptr) * (size_t)d->n * ho * wo * (size_t)round_up(d->cout, 4) * sizeof(float);
}

// Measured on MI355X at batch 1 (tools/conv_bench.py --splitk, profiles/latency/conv_bench_splitk.txt): every fp32 conv
// shape of the 416 and 608 networks, the default plan's launch against the pair, 7 alternating rounds; "faster" = the slowest
// split-K round beats the fastest default round. The pair wins wherever the rule above cuts K at all (S >= 2: the 64x64 grid of one
// image has fewer than 512 workgroups), by 1.1x to 7x, with one exception: the 255-channel head at 76x76 (S = 2, 5,776 pixels
// through the combine's scalar stores: 24 against 23 us), while the heads up to 52x52 win. With S = 1 the pair is the
// 64x64 kernel in two launches and loses (1.2x to 1.8x slower from 104x104 1x1 / 152x152 up), except the 64 -> 128 3x3 at 152x152
// (49 against 52 us for Winograd F(4x4)), which is left to the default.
bool splitk_eligible(const yolo_conv_desc* d) {
    if (splitk_slices(d, nullptr) < 2) return false;
    const int pad = d->ksize / 2;
    const long long ho = (d->h + 2 * pad - d->ksize) / d->stride + 1, wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
    if ((d->cout & 3) && ho * wo > 4096) return false;       // scalar-store outputs: measured ahead at 2,704 pixels, behind at 5,776
    return true;
}

int conv_splitk_launch(const ConvArgs& a, const yolo_conv_desc* d, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!ws || ws_bytes < splitk_workspace_bytes(d)) return fail(YOLO_ERR_WORKSPACE, "conv: split-K workspace too small");   // (conv_fwd_impl checked)
    if ((uintptr_t)ws & 15) return fail(YOLO_ERR_ARG, "conv: the split-K workspace must be 16-byte aligned");
    SplitKArgs q;
    q.p = a;
    q.partial = (float*)ws;
    q.S = splitk_slices(d, &q.L);
    q.ldp = round_up(a.Cout, 4);
    q.p.tiles_n = ceil_div(a.Cout, SK_BN);
    const long long tiles = (long long)ceil_div(a.M, SK_BM) * q.p.tiles_n;
    const size_t lanes = (size_t)a.M * (size_t)(q.ldp / 4);
    const size_t cblocks = (lanes + 255) / 256;
    if (tiles > 0x7fffffffLL || cblocks > 0x7fffffffULL) return fail(YOLO_ERR_UNSUPPORTED, "conv: split-K grid exceeds int32");
    const size_t lds = (size_t)2 * (SK_BM + SK_BN) * SK_LDS_LD * sizeof(float);
    hipLaunchKernelGGL((conv_splitk_f32<SK_BM, SK_BN>), dim3((unsigned)tiles, (unsigned)q.S), dim3(256), lds, s, q);
    int rc = check_launch("conv_splitk_f32");
    if (rc) return rc;
    YOLO_SWITCH_ACT(a.act, hipLaunchKernelGGL((splitk_combine_f32<ACT>), dim3((unsigned)cblocks), dim3(256), 0, s, q));
    return check_launch("splitk_combine_f32");
}

}  // namespace yolo
