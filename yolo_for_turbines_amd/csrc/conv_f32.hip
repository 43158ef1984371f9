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

// Measured on MI355X (tools/conv_bench.py, batch 32). The register-staged kernel of this file is
// latency-bound, so among its tiles 64x64 (4+ resident blocks per CU) wins on every YOLOv3 shape;
// stride-1 layers with cin % 32 == 0 go to the patch/fragment-stream kernel (ids 5, 6).
static int pick_direct_tile(const yolo_conv_desc* d) {
    if (v2_eligible(d) && d->ksize == 3) {
        // Measured (tools/conv_bench.py --tile 5,6,7, batch 32): BN = 64 with ONE patch buffer (tile 7: 37 KB of LDS,
        // 148 registers -> 3 blocks per CU instead of 2, one extra barrier per 32-channel chunk) wins by 4-16 % at 208x208,
        // 104x104, 52x52 and 13x13 — three co-resident blocks cover each other's prologue/epilogue and 752 blocks fill
        // 768 slots in one round at 13x13. At 26x26 (K = 2304, 1440 such blocks) BN = 128 with two buffers stays 9 % ahead.
        const int ho = d->h;
        if (d->cout > 64 && ho <= 26 && ho > 13 && v2_blocks(d, 128) >= 640) return kTileF32V2Bn128;
        return kTileF32V2Single;
    }
    return kTileF32Reg64x64;       // 1x1 (few K steps, prologue-dominated) and stride-2 layers: 64x64 register-staged tile
}

// Which kernel family runs an fp32 descriptor: the one place that knows. `ws_avail` is the workspace the caller brings (0: none,
// SIZE_MAX: whatever yolo_conv_workspace_bytes asks for). A forced tile names its family whether or not the layer fits it - the
// launch then fails with that family's message; tile 0 is the heuristic, which looks at the layer's shape only, never at the batch
// (and, in wino4_eligible, at whether the caller brings finished filters: YOLO_FLAG_FILTERS_APPENDED).
enum class F32Family { Direct, Rs, Wino, Wino4 };

static F32Family f32_family(const yolo_conv_desc* d, const void* residual, size_t ws_avail) {
    const bool heuristic = d->tile == 0;
    // 1x1 with 256 / 384 / 512 input channels and a multiple of 128 output channels: weights stationary in registers
    if ((heuristic || d->tile == kTileF32Rs) && conv1_rs_eligible(d, residual)) return F32Family::Rs;
    // 3x3 stride 1 by Winograd F(4x4, 3x3), else by F(2x2, 3x3): the heuristic only with a large enough workspace (yolo_conv_fwd has
    // none: the library allocates nothing), so a workspace between the two sizes gets F(2x2)
    if (d->tile == kTileF32Wino4 || (heuristic && wino4_eligible(d) && ws_avail >= wino4_workspace_bytes(d))) return F32Family::Wino4;
    if (d->tile == kTileF32Wino || d->tile == kTileF32Wino2 || (heuristic && wino_eligible(d) && ws_avail >= wino_workspace_bytes(d)))
        return F32Family::Wino;
    return F32Family::Direct;       // tiles 1-7 (and tile 12 on a layer conv1_rs_f32 cannot run: an error)
}

// what the heuristic picks when the caller brings the workspace (yolo_conv_fwd_ws / the launch table). A layer of the F(2x2) family is
// reported as tile 13 also where conv_wino_launch then takes the two-pass kernel (tile 14), a conv1_rs_f32 layer as its direct tile
static int pick_tile(const yolo_conv_desc* d) {
    yolo_conv_desc h = *d;
    h.tile = 0;
    switch (f32_family(&h, nullptr, SIZE_MAX)) {
    case F32Family::Wino4: return kTileF32Wino4;
    case F32Family::Wino: return kTileF32Wino;
    default: return pick_direct_tile(d);
    }
}

// YOLO_FLAG_SPLIT_BF16 is honoured on fp32 descriptors of the Direct and Rs families that conv_split3_f32 can run
static bool split3_honoured(const yolo_conv_desc* d, const void* residual, size_t ws_avail) {
    if (!split3_supported(d)) return false;
    const F32Family f = f32_family(d, residual, ws_avail);
    return f == F32Family::Direct || f == F32Family::Rs;
}

static int validate(const yolo_conv_desc* d) {
    if (!d) return fail(YOLO_ERR_ARG, "conv: null descriptor");
    if (d->dtype < 0 || d->dtype > 2) return fail(YOLO_ERR_ARG, "conv: dtype %d", d->dtype);
    if (d->ksize != 1 && d->ksize != 3) return fail(YOLO_ERR_UNSUPPORTED, "conv: ksize %d", d->ksize);
    if (d->stride != 1 && d->stride != 2) return fail(YOLO_ERR_UNSUPPORTED, "conv: stride %d", d->stride);
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0) return fail(YOLO_ERR_ARG, "conv: bad shape");
    const int cp = cin_pad_of(d->cin);
    // (a forced tile 15 reaches conv_wino4_f32 or nothing: its transforms take any multiple of 4, wino4_supported checks that)
    const bool forced_wino4 = d->dtype == YOLO_F32 && d->tile == kTileF32Wino4 && d->ksize == 3 && d->stride == 1;
    if (cp != 4 && cp % 32 != 0 && !forced_wino4) return fail(YOLO_ERR_UNSUPPORTED, "conv: cin %d (need <= 4 or a multiple of 32)", d->cin);
    if (d->x_ld < cp + 0 || (d->x_ld & 3) || (d->x_off & 3)) return fail(YOLO_ERR_ARG, "conv: x_ld/x_off must be multiples of 4 and x_ld >= cin_pad");
    if (d->out_mode == YOLO_OUT_HEAD && d->cout % 3 != 0) return fail(YOLO_ERR_ARG, "conv: head cout %% 3 != 0");
    if (d->out_mode < 0 || d->out_mode > 2) return fail(YOLO_ERR_ARG, "conv: out_mode");
    if (d->tile < 0 || d->tile > kMaxTileId) return fail(YOLO_ERR_ARG, "conv: tile id");
    return YOLO_OK;
}

static int conv_fwd_impl(const yolo_conv_desc* d, const void* x, const void* w, const float* scale, const float* shift,
                         const void* residual, void* y, void* ws, size_t ws_bytes, int32_t* nan_flag, hipStream_t s) {
    int rc = validate(d);
    if (rc) return rc;
    if (!x || !w || !scale || !shift || !y) return fail(YOLO_ERR_ARG, "conv: null pointer");
    if ((d->flags & YOLO_FLAG_RESIDUAL) && !residual) return fail(YOLO_ERR_ARG, "conv: residual flag without pointer");
    if ((d->flags & YOLO_FLAG_NANCHECK) && !nan_flag) return fail(YOLO_ERR_ARG, "conv: nancheck flag without pointer");
    // the split-K pair runs whatever Winograd or the bf16 split would have chosen: it goes with none of their flags, with no forced tile
    const bool splitk = d->flags & YOLO_FLAG_SPLIT_K;
    if (splitk) {
        if (d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_FILTERS_APPENDED | YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY))
            return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_K goes with none of YOLO_FLAG_FILTERS_READY, YOLO_FLAG_FILTERS_APPENDED, "
                                              "YOLO_FLAG_SPLIT_BF16, YOLO_FLAG_SPLIT_WEIGHTS_READY");
        if (d->tile != 0 || !splitk_supported(d))
            return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_K needs an fp32 layer with ksize 1 or 3, stride 1 or 2, cin %% 32 == 0 and tile 0");
        if (!ws || ws_bytes < splitk_workspace_bytes(d))
            return fail(YOLO_ERR_WORKSPACE, "conv: YOLO_FLAG_SPLIT_K needs a workspace of %zu bytes (yolo_conv_workspace_bytes)",
                        splitk_workspace_bytes(d));
    }
    const bool filters_ready = d->flags & YOLO_FLAG_FILTERS_READY;
    if (filters_ready && (d->dtype != YOLO_F32 || f32_family(d, residual, ws ? ws_bytes : 0) != F32Family::Wino4))
        return fail(YOLO_ERR_ARG, "conv: YOLO_FLAG_FILTERS_READY on a layer that does not run as Winograd F(4x4) (tile 15 with its workspace)");
    // ... or the packed weights with U4 behind them: the same launch, and the only flag that wino4_eligible looks at
    const bool filters_appended = d->flags & YOLO_FLAG_FILTERS_APPENDED;
    if (filters_appended && (d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY)))
        return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_FILTERS_APPENDED goes with none of YOLO_FLAG_FILTERS_READY, YOLO_FLAG_SPLIT_BF16, "
                                          "YOLO_FLAG_SPLIT_WEIGHTS_READY, YOLO_FLAG_SPLIT_K");
    if (filters_appended && (d->dtype != YOLO_F32 || f32_family(d, residual, ws ? ws_bytes : 0) != F32Family::Wino4))
        return fail(YOLO_ERR_ARG, "conv: YOLO_FLAG_FILTERS_APPENDED on a layer that does not run as Winograd F(4x4) (tile 15 with its workspace)");
    // the three-way bf16 split runs what the direct kernels would run (conv_igemm_f32, conv_f32_v2, conv1_rs_f32) and nothing else
    const bool split3 = d->flags & YOLO_FLAG_SPLIT_BF16;
    if (split3 && !split3_honoured(d, residual, ws ? ws_bytes : 0))
        return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_BF16 needs an fp32 layer of the direct kernels (no Winograd workspace in play) with "
                                          "ksize 1 or 3, stride 1 or 2 and cin %% 32 == 0");
    if ((d->flags & YOLO_FLAG_SPLIT_WEIGHTS_READY) && !split3)
        return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_WEIGHTS_READY goes with YOLO_FLAG_SPLIT_BF16 only");
    if (d->dtype != YOLO_F32) return conv_h16_launch(d, x, w, scale, shift, residual, y, nan_flag, s);
    ConvArgs a;
    a.x = (const float*)x; a.w = (const float*)w; a.w_planes = nullptr; a.scale = scale; a.shift = shift;
    a.res = (const float*)residual; a.y = (float*)y; a.nan_flag = nan_flag;
    a.N = d->n; a.H = d->h; a.W = d->w; a.Cin = cin_pad_of(d->cin); a.Cout = d->cout;
    a.ks = d->ksize; a.stride = d->stride; a.pad = d->ksize / 2;
    a.Ho = (d->h + 2 * a.pad - d->ksize) / d->stride + 1;
    a.Wo = (d->w + 2 * a.pad - d->ksize) / d->stride + 1;
    const long long M = (long long)d->n * a.Ho * a.Wo;
    if (M > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "conv: N*Ho*Wo exceeds int32");
    a.M = (int)M;
    a.x_ld = d->x_ld; a.x_off = d->x_off; a.y_ld = d->y_ld; a.y_off = d->y_off; a.r_ld = d->r_ld; a.r_off = d->r_off;
    a.Kpad = kpad_of(d->cin, d->ksize);
    a.KT = a.Kpad / BK;
    a.act = d->act; a.out_mode = d->out_mode; a.flags = d->flags;
    a.nc5 = d->out_mode == YOLO_OUT_HEAD ? d->cout / 3 : 1;
    a.tiles_n = 0;
    const bool smallc = a.Cin == 4;
    if (splitk) return conv_splitk_launch(a, d, ws, ws_bytes, s);
    if (split3) {
        if (d->flags & YOLO_FLAG_SPLIT_WEIGHTS_READY) a.w_planes = (const char*)w + split3_planes_offset(d);
        return conv_split3_launch(a, d->tile == kTileF32Rs ? 0 : d->tile, s);
    }
    switch (f32_family(d, residual, ws ? ws_bytes : 0)) {
    case F32Family::Rs: return conv1_rs_launch(d, x, w, scale, shift, residual, y, nan_flag, s);
    case F32Family::Wino4: {        // the filters are transformed per launch from the row-major section, unless w is their transform
        if (!wino4_supported(d)) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile 15 needs fp32 3x3 stride 1 with NHWC output and channel counts %% 4 == 0");
        const float* U4 = filters_ready ? (const float*)w                                                      // ... or has it behind it
                        : filters_appended ? (const float*)((const char*)w + wino4_appended_offset(d)) : nullptr;
        return conv_wino4_launch(d, x, U4 ? nullptr : (const float*)w, U4, scale, shift, residual, y, ws, ws_bytes, nan_flag, s);
    }
    case F32Family::Wino: {
        if (!wino_supported(d)) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile 13 needs fp32 3x3 stride 1 with NHWC output and channel counts %% 4 == 0");
        const float* U = (const float*)w + v0_packed_elems(d->cout, d->cin, d->ksize) + v2_frag_elems(d->cout, d->cin, d->ksize);
        return conv_wino_launch(d, x, U, scale, shift, residual, y, ws, ws_bytes, nan_flag, s);
    }
    case F32Family::Direct: break;
    }
    if (d->tile == kTileF32Rs) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile 12 needs a 1x1 with 256 / 384 / 512 input channels and cout %% 128 == 0");
    const int t = d->tile ? d->tile : pick_direct_tile(d);
    if (t > kTileF32V2Single) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile ids from 8 up are 16-bit kernels (conv3_dma_h16)");
    if (t >= kTileF32V2Bn64) {
        if (!v2_eligible(d)) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile %d needs stride 1 and cin %% 32 == 0", t);
        const float* wf = (const float*)w + v0_packed_elems(d->cout, d->cin, d->ksize);
        return conv_v2_launch(d, x, wf, scale, shift, residual, y, nan_flag, t == kTileF32V2Bn128 ? 128 : 64, t == kTileF32V2Single, s);
    }
    switch (t) {
        case kTileF32Reg128x128: return launch_tile<128, 128>(a, smallc, s);
        case kTileF32Reg128x64: return launch_tile<128, 64>(a, smallc, s);
        case kTileF32Reg64x128: return launch_tile<64, 128>(a, smallc, s);
        default: return launch_tile<64, 64>(a, smallc, s);
    }
}

}  // namespace yolo

extern "C" {

int yolo_conv_num_tiles(void) { return yolo::kNumTiles; }

int yolo_conv_pick_tile(const yolo_conv_desc* d) {
    int rc = yolo::validate(d);
    if (rc) return rc;
    return yolo::pick_tile(d);
}

int yolo_conv_split3_supported(const yolo_conv_desc* d) {
    if (yolo::validate(d)) return 0;
    yolo_conv_desc h = *d;
    h.tile = 0;
    return yolo::split3_honoured(&h, nullptr, SIZE_MAX);
}

int yolo_conv_split3_eligible(const yolo_conv_desc* d) { return yolo_conv_split3_supported(d) && yolo::split3_eligible(d); }

int yolo_conv_splitk_supported(const yolo_conv_desc* d) { return !yolo::validate(d) && yolo::splitk_supported(d); }

int yolo_conv_splitk_eligible(const yolo_conv_desc* d) { return yolo_conv_splitk_supported(d) && yolo::splitk_eligible(d); }

int yolo_conv_splitk_slices(const yolo_conv_desc* d) { return yolo_conv_splitk_supported(d) ? yolo::splitk_slices(d, nullptr) : 0; }

size_t yolo_split3_weight_bytes(const yolo_conv_desc* d) { return d && yolo_conv_split3_supported(d) ? yolo::split3_weight_bytes(d) : 0; }

int yolo_split3_weights(const yolo_conv_desc* d, const void* w_packed, void* out, void* stream) {
    if (!d || !yolo_conv_split3_supported(d))
        return yolo::fail(YOLO_ERR_UNSUPPORTED, "yolo_split3_weights: the library does not honour YOLO_FLAG_SPLIT_BF16 on this layer");
    if (!w_packed || !out || ((uintptr_t)out & 15)) return yolo::fail(YOLO_ERR_ARG, "yolo_split3_weights: null or misaligned pointer");
    return yolo::split3_weights_launch(d, w_packed, out, (hipStream_t)stream);
}

int yolo_conv_fwd(const yolo_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                  const void* residual, void* y, int32_t* nan_flag, void* stream) {
    return yolo::conv_fwd_impl(d, x, w_packed, scale, shift, residual, y, nullptr, 0, nan_flag, (hipStream_t)stream);
}

size_t yolo_conv_workspace_bytes(const yolo_conv_desc* d) {
    if (yolo::validate(d)) return 0;
    if (d->flags & YOLO_FLAG_SPLIT_K)               // 0 wherever the launch refuses the flag: another kernel flag, a forced tile, the shape
        return !(d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_FILTERS_APPENDED | YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY)) && d->tile == 0 &&
                       yolo::splitk_supported(d)
                   ? yolo::splitk_workspace_bytes(d)
                   : 0;
    switch (yolo::f32_family(d, nullptr, SIZE_MAX)) {          // (the caller will bring what this asks for)
    case yolo::F32Family::Wino4: return yolo::wino4_workspace_bytes(d);
    case yolo::F32Family::Wino: return yolo::wino_workspace_bytes(d);
    default: return 0;
    }
}

int yolo_conv_fwd_ws(const yolo_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                     const void* residual, void* y, void* workspace, size_t workspace_bytes, int32_t* nan_flag, void* stream) {
    return yolo::conv_fwd_impl(d, x, w_packed, scale, shift, residual, y, workspace, workspace_bytes, nan_flag, (hipStream_t)stream);
}

int yolo_conv_fwd_batch(const yolo_conv_op* ops, int n_ops, int32_t* nan_flag, void* stream) {
    if (!ops && n_ops > 0) return yolo::fail(YOLO_ERR_ARG, "conv batch: null ops");
    for (int i = 0; i < n_ops; ++i) {
        const yolo_conv_op& o = ops[i];
        int rc = yolo::conv_fwd_impl(&o.d, (const void*)o.x, (const void*)o.w_packed, (const float*)o.scale,
                                     (const float*)o.shift, (const void*)o.residual, (void*)o.y, (void*)o.workspace,
                                     (size_t)o.workspace_bytes, nan_flag, (hipStream_t)stream);
        if (rc) return rc;
    }
    return YOLO_OK;
}

}  // extern "C"
