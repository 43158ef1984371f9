// conv_dispatch.hip — host side of yolo_conv_fwd, yolo_conv_fwd_ws, yolo_conv_fwd_batch and the queries next to them: which fp32 kernel
// a descriptor runs, which flags may stand on it, where in the packed buffer that kernel's weights begin. No kernel lives here: they
// are in conv_f32.hip, conv_f32_v2.hip, conv1_rs_f32.hip, conv_wino_f32.hip, conv_wino4_f32.hip, conv_wino4s_f32.hip, conv_split3_f32.hip, conv_splitk_f32.hip.
#include "conv_f32_epilogue.h"

namespace yolo {

// Measured on MI355X (tools/conv_bench.py, batch 32). The register-staged kernel of conv_f32.hip is
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

// Why a launch refuses YOLO_FLAG_SPLIT_K on d (null: it does not): the split-K pair runs whatever Winograd or the bf16 split would
// have chosen, so it goes with none of their flags and with no forced tile. yolo_conv_workspace_bytes reports 0 where this refuses.
static const char* splitk_refusal(const yolo_conv_desc* d) {
    if (d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_FILTERS_APPENDED | YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY))
        return "conv: YOLO_FLAG_SPLIT_K goes with none of YOLO_FLAG_FILTERS_READY, YOLO_FLAG_FILTERS_APPENDED, YOLO_FLAG_SPLIT_BF16, "
               "YOLO_FLAG_SPLIT_WEIGHTS_READY";
    if (d->tile != 0 || !splitk_supported(d))
        return "conv: YOLO_FLAG_SPLIT_K needs an fp32 layer with ksize 1 or 3, stride 1 or 2, cin % 32 == 0 and tile 0";
    return nullptr;
}

// Which kernel runs an fp32 descriptor, what it takes from the caller's workspace, where in w_packed its weights begin: the one place
// that knows, resolved once per call. Every valid descriptor has a route; check_flags says whether its flags may stand there.
enum class F32Kind { SplitK, Split3, Rs, Wino4, Wino, Direct };
struct F32Route {
    F32Kind kind;
    int direct_tile;            // Direct: the tile id (1 .. 7, or a forced id that no fp32 kernel has); Split3: the forced tile or 0
    size_t workspace_need;      // bytes of the caller's workspace the kernel uses
    size_t weights_offset;      // bytes from w_packed to what the kernel reads, where that is not the row-major section at 0
};
// `ws_avail` is the workspace the caller brings (0: none, SIZE_MAX: whatever yolo_conv_workspace_bytes asks for). A forced tile names
// its kernel whether or not the layer fits it - the launch then fails with that kernel's message; tile 0 is the heuristic, which
// looks at the layer's shape only, never at the batch (and, in wino4_eligible, at whether the caller brings finished filters:
// YOLO_FLAG_FILTERS_APPENDED). The two flags that name a kernel of their own come last: they replace what the rest chose.
static F32Route f32_route(const yolo_conv_desc* d, const void* residual, size_t ws_avail) {
    const bool heuristic = d->tile == 0;
    F32Route r{F32Kind::Direct, 0, 0, 0};       // tiles 1-7 (and tile 12 on a layer conv1_rs_f32 cannot run: an error)
    // 1x1 with 256 / 384 / 512 input channels and a multiple of 128 output channels: weights stationary in registers
    if ((heuristic || d->tile == kTileF32Rs) && conv1_rs_eligible(d, residual)) r.kind = F32Kind::Rs;
    // 3x3 stride 1 by Winograd F(4x4, 3x3), else by F(2x2, 3x3): the heuristic only with a large enough workspace (yolo_conv_fwd has
    // none: the library allocates nothing), so a workspace between the two sizes gets F(2x2)
    else if (d->tile == kTileF32Wino4 || (heuristic && wino4_eligible(d) && ws_avail >= wino4_workspace_bytes(d))) r.kind = F32Kind::Wino4;
    else if (d->tile == kTileF32Wino || d->tile == kTileF32Wino2 || (heuristic && wino_eligible(d) && ws_avail >= wino_workspace_bytes(d)))
        r.kind = F32Kind::Wino;
    // the split-K pair; the three-way bf16 split, which runs what conv_igemm_f32, conv_f32_v2 and conv1_rs_f32 would and nothing else
    if ((d->flags & YOLO_FLAG_SPLIT_K) && !splitk_refusal(d)) r.kind = F32Kind::SplitK;
    else if ((d->flags & YOLO_FLAG_SPLIT_BF16) && (r.kind == F32Kind::Direct || r.kind == F32Kind::Rs) && split3_supported(d)) r.kind = F32Kind::Split3;
    const auto sec = [d] { return packed_f32(d->cout, d->cin, d->ksize); };
    switch (r.kind) {
    case F32Kind::SplitK: r.workspace_need = splitk_workspace_bytes(d); break;
    case F32Kind::Split3:           // (prepared weights: the bf16 planes lie behind the packed ones)
        r.direct_tile = d->tile == kTileF32Rs ? 0 : d->tile;
        if (d->flags & YOLO_FLAG_SPLIT_WEIGHTS_READY) r.weights_offset = sec().tail_bytes;
        break;
    case F32Kind::Wino4:            // (appended filters: U4 lies behind the packed weights; YOLO_FLAG_FILTERS_READY: w_packed is U4 itself)
        // (YOLO_FLAG_WINO_SPLIT_BF16: the bf16 planes of V4 and U4 instead; check_flags says where the flag may stand)
        r.workspace_need = (d->flags & YOLO_FLAG_WINO_SPLIT_BF16) && wino4_split_supported(d) ? wino4_split_workspace_bytes(d) : wino4_workspace_bytes(d);
        if (d->flags & YOLO_FLAG_FILTERS_APPENDED) r.weights_offset = sec().tail_bytes;
        break;
    case F32Kind::Wino: r.workspace_need = wino_workspace_bytes(d); r.weights_offset = sec().wino * sizeof(float); break;
    case F32Kind::Direct:
        r.direct_tile = heuristic ? pick_direct_tile(d) : d->tile;
        if (r.direct_tile >= kTileF32V2Bn64) r.weights_offset = sec().frag * sizeof(float);
        break;
    case F32Kind::Rs: break;
    }
    return r;
}

// The route the queries ask about: the heuristic's, with the workspace it asks for, with `flags` for d's split-K / bf16-split flags
static F32Route heuristic_route(const yolo_conv_desc* d, int flags) {
    yolo_conv_desc h = *d;
    h.tile = 0;
    h.flags = (d->flags & ~(YOLO_FLAG_SPLIT_K | YOLO_FLAG_SPLIT_BF16)) | flags;
    return f32_route(&h, nullptr, SIZE_MAX);
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

// Whether the kernel flags on d may stand on route r, with the workspace the caller brought. The order of the checks is part of the
// ABI: a descriptor that breaks two rules is refused by the first.
static int check_flags(const yolo_conv_desc* d, const F32Route& r, const void* ws, size_t ws_bytes) {
    if (d->flags & YOLO_FLAG_SPLIT_K) {
        if (const char* why = splitk_refusal(d)) return fail(YOLO_ERR_UNSUPPORTED, "%s", why);
        if (!ws || ws_bytes < r.workspace_need)
            return fail(YOLO_ERR_WORKSPACE, "conv: YOLO_FLAG_SPLIT_K needs a workspace of %zu bytes (yolo_conv_workspace_bytes)", r.workspace_need);
    }
    const bool wino4 = d->dtype == YOLO_F32 && r.kind == F32Kind::Wino4;
    // finished filters: w_packed is U4 ...
    if ((d->flags & YOLO_FLAG_FILTERS_READY) && !wino4)
        return fail(YOLO_ERR_ARG, "conv: YOLO_FLAG_FILTERS_READY on a layer that does not run as Winograd F(4x4) (tile 15 with its workspace)");
    // ... or the packed weights with U4 behind them: the same launch, and the only flag that wino4_eligible looks at
    const bool filters_appended = d->flags & YOLO_FLAG_FILTERS_APPENDED;
    if (filters_appended && (d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY)))
        return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_FILTERS_APPENDED goes with none of YOLO_FLAG_FILTERS_READY, YOLO_FLAG_SPLIT_BF16, "
                                          "YOLO_FLAG_SPLIT_WEIGHTS_READY, YOLO_FLAG_SPLIT_K");
    if (filters_appended && !wino4)
        return fail(YOLO_ERR_ARG, "conv: YOLO_FLAG_FILTERS_APPENDED on a layer that does not run as Winograd F(4x4) (tile 15 with its workspace)");
    // ... with its bf16 planes behind it: describes the buffer of either filter flag, where the planes kernel could read it
    if ((d->flags & YOLO_FLAG_FILTER_PLANES) && !(wino4 && wino4_split_supported(d) && (d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_FILTERS_APPENDED))))
        return fail(YOLO_ERR_ARG, "conv: YOLO_FLAG_FILTER_PLANES goes with YOLO_FLAG_FILTERS_READY or YOLO_FLAG_FILTERS_APPENDED on a layer that runs as "
                                  "Winograd F(4x4) (tile 15 with its workspace) with cin %% 32 == 0");
    const bool split3 = d->flags & YOLO_FLAG_SPLIT_BF16;
    if (split3 && r.kind != F32Kind::Split3)
        return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_BF16 needs an fp32 layer of the direct kernels (no Winograd workspace in play) with "
                                          "ksize 1 or 3, stride 1 or 2 and cin %% 32 == 0");
    if ((d->flags & YOLO_FLAG_SPLIT_WEIGHTS_READY) && !split3)
        return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_WEIGHTS_READY goes with YOLO_FLAG_SPLIT_BF16 only");
    // the Winograd F(4x4) GEMMs on bf16 planes: a variant of the launch on finished filters, and of nothing else
    if (d->flags & YOLO_FLAG_WINO_SPLIT_BF16) {
        if (!wino4 || !wino4_split_supported(d))
            return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_WINO_SPLIT_BF16 needs an fp32 layer that runs as Winograd F(4x4) (tile 15 with its "
                                              "workspace) with cin %% 32 == 0");
        if (!(d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_FILTERS_APPENDED)))
            return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_WINO_SPLIT_BF16 goes with YOLO_FLAG_FILTERS_READY or YOLO_FLAG_FILTERS_APPENDED");
        if (d->flags & (YOLO_FLAG_SPLIT_K | YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY))
            return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_WINO_SPLIT_BF16 goes with none of YOLO_FLAG_SPLIT_K, YOLO_FLAG_SPLIT_BF16, "
                                              "YOLO_FLAG_SPLIT_WEIGHTS_READY");
    }
    return YOLO_OK;
}

static int conv_fwd_impl(const yolo_conv_desc* d, const void* x, const void* w, const float* scale, const float* shift,
                         const void* residual, void* y, void* ws, size_t ws_bytes, int32_t* nan_flag, hipStream_t s) {
    if (int rc = validate(d)) return rc;
    if (!x || !w || !scale || !shift || !y) return fail(YOLO_ERR_ARG, "conv: null pointer");
    if ((d->flags & YOLO_FLAG_RESIDUAL) && !residual) return fail(YOLO_ERR_ARG, "conv: residual flag without pointer");
    if ((d->flags & YOLO_FLAG_NANCHECK) && !nan_flag) return fail(YOLO_ERR_ARG, "conv: nancheck flag without pointer");
    const F32Route r = f32_route(d, residual, ws ? ws_bytes : 0);
    if (int rc = check_flags(d, r, ws, ws_bytes)) return rc;
    if (d->dtype != YOLO_F32) return conv_h16_launch(d, x, w, scale, shift, residual, y, nan_flag, s);
    const int pad = d->ksize / 2, Ho = (d->h + 2 * pad - d->ksize) / d->stride + 1, Wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
    const long long M = (long long)d->n * Ho * Wo;
    if (M > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "conv: N*Ho*Wo exceeds int32");
    const char* wr = (const char*)w + r.weights_offset;         // what the route's kernel reads
    const auto args = [&] {                                     // of the kernels that share conv_f32_epilogue.h
        ConvArgs a;
        a.x = (const float*)x; a.w = (const float*)w; a.scale = scale; a.shift = shift;
        a.w_planes = r.kind == F32Kind::Split3 && r.weights_offset ? wr : nullptr;         // (YOLO_FLAG_SPLIT_WEIGHTS_READY)
        a.res = (const float*)residual; a.y = (float*)y; a.nan_flag = nan_flag;
        a.N = d->n; a.H = d->h; a.W = d->w; a.Cin = cin_pad_of(d->cin); a.Cout = d->cout;
        a.ks = d->ksize; a.stride = d->stride; a.pad = pad;
        a.Ho = Ho; a.Wo = Wo; a.M = (int)M;
        a.x_ld = d->x_ld; a.x_off = d->x_off; a.y_ld = d->y_ld; a.y_off = d->y_off; a.r_ld = d->r_ld; a.r_off = d->r_off;
        a.Kpad = kpad_of(d->cin, d->ksize);
        a.KT = a.Kpad / BK;
        a.act = d->act; a.out_mode = d->out_mode; a.flags = d->flags;
        a.nc5 = d->out_mode == YOLO_OUT_HEAD ? d->cout / 3 : 1;
        a.tiles_n = 0;
        return a;
    };
    switch (r.kind) {
    case F32Kind::SplitK: return conv_splitk_launch(args(), d, ws, ws_bytes, s);
    case F32Kind::Split3: return conv_split3_launch(args(), r.direct_tile, s);
    case F32Kind::Rs: return conv1_rs_launch(d, x, w, scale, shift, residual, y, nan_flag, s);
    case F32Kind::Wino4: {          // the filters are transformed per launch from the row-major section, unless the caller brings U4
        if (!wino4_supported(d)) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile 15 needs fp32 3x3 stride 1 with NHWC output and channel counts %% 4 == 0");
        const float* U4 = d->flags & (YOLO_FLAG_FILTERS_READY | YOLO_FLAG_FILTERS_APPENDED) ? (const float*)wr : nullptr;
        if (d->flags & YOLO_FLAG_WINO_SPLIT_BF16) {         // (YOLO_FLAG_FILTER_PLANES: the planes of U4 lie directly behind it; ignored on the f32 GEMMs)
            const void* planes = d->flags & YOLO_FLAG_FILTER_PLANES ? wr + wino4_filter_bytes(d) : nullptr;
            return conv_wino4s_launch(d, x, U4, planes, scale, shift, residual, y, ws, ws_bytes, nan_flag, s);
        }
        return conv_wino4_launch(d, x, U4 ? nullptr : (const float*)w, U4, scale, shift, residual, y, ws, ws_bytes, nan_flag, s);
    }
    case F32Kind::Wino:
        if (!wino_supported(d)) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile 13 needs fp32 3x3 stride 1 with NHWC output and channel counts %% 4 == 0");
        return conv_wino_launch(d, x, (const float*)wr, scale, shift, residual, y, ws, ws_bytes, nan_flag, s);
    case F32Kind::Direct: break;
    }
    const int t = r.direct_tile;
    if (t == kTileF32Rs) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile 12 needs a 1x1 with 256 / 384 / 512 input channels and cout %% 128 == 0");
    if (t > kTileF32V2Single) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile ids from 8 up are 16-bit kernels (conv3_dma_h16)");
    if (t >= kTileF32V2Bn64) {
        if (!v2_eligible(d)) return fail(YOLO_ERR_UNSUPPORTED, "conv: tile %d needs stride 1 and cin %% 32 == 0", t);
        return conv_v2_launch(d, x, (const float*)wr, scale, shift, residual, y, nan_flag, t == kTileF32V2Bn128 ? 128 : 64, t == kTileF32V2Single, s);
    }
    return conv_igemm_launch(args(), t, s);
}

}  // namespace yolo

extern "C" {

int yolo_conv_num_tiles(void) { return yolo::kNumTiles; }

// what the heuristic picks when the caller brings the workspace (yolo_conv_fwd_ws / the launch table). A layer of the F(2x2) family is
// reported as tile 13 also where conv_wino_launch then takes the two-pass kernel (tile 14), a conv1_rs_f32 layer as its direct tile
int yolo_conv_pick_tile(const yolo_conv_desc* d) {
    if (int rc = yolo::validate(d)) return rc;
    const yolo::F32Kind k = yolo::heuristic_route(d, 0).kind;
    return k == yolo::F32Kind::Wino4 ? yolo::kTileF32Wino4 : k == yolo::F32Kind::Wino ? yolo::kTileF32Wino : yolo::pick_direct_tile(d);
}

// YOLO_FLAG_SPLIT_BF16 is honoured on fp32 descriptors that conv_split3_f32 can run and that the direct kernels or conv1_rs_f32 would run
int yolo_conv_split3_supported(const yolo_conv_desc* d) {
    return !yolo::validate(d) && yolo::heuristic_route(d, YOLO_FLAG_SPLIT_BF16).kind == yolo::F32Kind::Split3;
}

int yolo_conv_split3_eligible(const yolo_conv_desc* d) { return yolo_conv_split3_supported(d) && yolo::split3_eligible(d); }

// YOLO_FLAG_WINO_SPLIT_BF16 is honoured on the launches that run as tile 15 on finished filters (here: what the heuristic routes there
// with either filter flag) with cin % 32 == 0
int yolo_conv_wino4_split_supported(const yolo_conv_desc* d) {
    if (yolo::validate(d) || d->dtype != YOLO_F32 || !yolo::wino4_split_supported(d)) return 0;
    yolo_conv_desc h = *d;
    h.flags = 0;
    return yolo::heuristic_route(&h, 0).kind == yolo::F32Kind::Wino4 || yolo::heuristic_route(&h, YOLO_FLAG_FILTERS_APPENDED).kind == yolo::F32Kind::Wino4;
}

int yolo_conv_wino4_split_eligible(const yolo_conv_desc* d) { return yolo_conv_wino4_split_supported(d) && yolo::wino4_split_eligible(d); }

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

// (the caller will bring what this asks for) 0 wherever the launch refuses YOLO_FLAG_SPLIT_K; its other refusals are not applied here
size_t yolo_conv_workspace_bytes(const yolo_conv_desc* d) {
    if (yolo::validate(d)) return 0;
    if ((d->flags & YOLO_FLAG_SPLIT_K) && yolo::splitk_refusal(d)) return 0;
    return yolo::f32_route(d, nullptr, SIZE_MAX).workspace_need;
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
