// conv_h16.hip — host side of the bf16 / fp16 convolutions: checks a convolution (or a stride-2 input gradient), picks
// the kernel family that runs it, fills its ConvHArgs and calls that family's launcher. No kernel lives here; h16.h lists
// the units that hold them.
#include "h16.h"

namespace yolo {

// The GEMM view of ConvHArgs (conv1_dma_h16): one tile row of M pixels, `taps` K steps per 32-channel chunk. TW and PC are
// the divisors the gathering variants take a pixel index apart with, H the channels per class of the fused stride-2 gradient.
static void gemm_view(ConvHArgs& a, int M, int H, int TW, int PC, int taps) {
    a.H = H; a.W = M; a.rows_total = 1; a.TH = 1; a.TW = TW; a.PC = PC;
    a.nchunks = a.Cin / 32;
    a.KT = a.nchunks * taps;
    a.nc5 = 1;
    a.tiles_w = 1; a.first_wave = 0; a.stagger = 0; a.bufmask = 1; a.patch_cap = 128; a.mtab_off = 0;
}

// Fused statistics: report the number of partial rows and their channel stride. Returns 0 to go on to the launch, 1 when
// there is nothing to launch (dry run), or the error code of a statistics buffer that is too small.
static int stats_rows(int rows, int ld, int* rows_ld, bool dry, const size_t* bytes) {
    if (rows_ld) { rows_ld[0] = rows; rows_ld[1] = ld; }
    if (dry) return 1;
    if (bytes && *bytes < (size_t)rows * 2 * ld * sizeof(float)) return fail(YOLO_ERR_WORKSPACE, "conv statistics: buffer too small");
    return 0;
}

// dx (n, 2ho, 2wo, cin) [+ residual] from dz (n, ho, wo, cout), weights from h16_pack_dgrad_s2
int dgrad_s2_h16_launch(const void* dz, int dz_ld, int dz_off, const void* wf, const void* residual, int r_ld, int r_off, void* dx,
                        int dx_ld, int dx_off, int n, int ho, int wo, int cin, int cout, int dtype, hipStream_t s) {
    if (cout % 32) return fail(YOLO_ERR_UNSUPPORTED, "dgrad_s2 (16-bit): cout %d must be a multiple of 32", cout);
    if ((dz_ld & 7) || (dz_off & 7)) return fail(YOLO_ERR_ARG, "dgrad_s2 (16-bit): dz_ld/dz_off must be multiples of 8");
    ConvHArgs a;
    a.stats = nullptr; a.stats_ld = 0;
    a.x = (const unsigned short*)dz; a.scale = nullptr; a.shift = nullptr;
    a.res = (const unsigned short*)residual; a.y = dx; a.nan_flag = nullptr;
    a.Cin = cout; a.Cout = cin;
    a.x_ld = dz_ld; a.x_off = dz_off; a.y_ld = dx_ld; a.y_off = dx_off; a.r_ld = r_ld; a.r_off = r_off;
    a.Hin = ho; a.Win = wo; a.Ho = ho; a.Wo = wo;
    a.act = YOLO_ACT_NONE; a.out_mode = YOLO_OUT_NHWC; a.flags = residual ? YOLO_FLAG_RESIDUAL : 0;
    const long long M = (long long)n * ho * wo;
    if (M * 4 > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "dgrad_s2: too many pixels");
    if (s2g_ok(cout, cin) && !switches().no_dma && (dx_ld & 7) == 0 && (dx_off & 7) == 0 && (!residual || ((r_ld & 7) == 0 && (r_off & 7) == 0))) {
        size_t skip = 0;
        for (int cls = 0; cls < 4; ++cls) skip += cls_frag_elems(cin, cout, cls);
        a.wf = (const unsigned short*)wf + skip;
        a.scale = a.shift = reinterpret_cast<const float*>(a.wf);    // the kernel's prologue fetches a table it does not use here
        a.Cout = 4 * cin;
        gemm_view(a, (int)M, cin, wo, ho * wo, 4);          // K = 4 neighbours x cout
        a.cls_ph = a.cls_pw = 0;
        return launch_dma1(a, 2, dtype, s);
    }
    int prmax = 1;
    a.H = ho; a.W = wo; a.rows_total = n * ho;
    pick_tile_h(ho, ho, wo, 3, 1, &a.TH, &a.TW, &prmax);
    a.PC = a.TW + 2;
    a.patch_cap = round_up(prmax * a.PC, 8);               // see conv_h16_launch: keep two patch buffers under 40 KB when possible
    if (a.patch_cap < 224) a.patch_cap = 224;
    if (a.patch_cap > H_PATCH_CAP) return fail(YOLO_ERR_UNSUPPORTED, "dgrad_s2 (16-bit): patch too large");
    a.tiles_w = ceil_div(a.W, a.TW);
    a.nchunks = cout / 32;
    a.nc5 = 1;
    const int bn = (cin > 64 && ho <= 52) ? 128 : 64;
    return dgrad_s2_classes(a, (const unsigned short*)wf, cin, cout, bn, dtype, s);
}

int conv_h16_launch(const yolo_conv_desc* d, const void* x, const void* wf, const float* scale, const float* shift,
                    const void* residual, void* y, int32_t* nan_flag, hipStream_t s) {
    return conv_h16_launch_stats(d, x, wf, scale, shift, residual, y, nan_flag, nullptr, nullptr, nullptr, s, nullptr);
}

// stats != nullptr: the launch must be one of the DMA kernels (conv3_dma_h16 / conv1_dma_h16) with an identity epilogue; it
// also writes per-wave BatchNorm partial sums. dry (rows_ld != nullptr with x == nullptr): no launch, rows_ld[0..1] = the
// number of partial rows and their channel stride, or 0 rows when this convolution has no fused-statistics kernel.
int conv_h16_launch_stats(const yolo_conv_desc* d, const void* x, const void* wf, const float* scale, const float* shift,
                          const void* residual, void* y, int32_t* nan_flag, float* stats, int* rows_ld, const size_t* stats_bytes,
                          hipStream_t s, const ConvBStats* bs) {
    const bool dry = rows_ld != nullptr && x == nullptr;
    if (rows_ld) { rows_ld[0] = 0; rows_ld[1] = 0; }
    if (d->cin % 32) return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): cin %d must be a multiple of 32", d->cin);
    if (d->ksize == 1 && d->stride != 1) return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): strided 1x1");
    if ((d->x_ld & 7) || (d->x_off & 7)) return fail(YOLO_ERR_ARG, "conv (16-bit): x_ld/x_off must be multiples of 8");
    ConvHArgs a;
    a.x = (const unsigned short*)x; a.wf = (const unsigned short*)wf; a.scale = scale; a.shift = shift;
    a.res = (const unsigned short*)residual; a.y = y; a.nan_flag = nan_flag;
    a.stats = stats; a.stats_ld = round_up(d->cout, 128);
    const bool want_stats = stats != nullptr || dry;
    // the DMA kernels request their scale / shift table in the prologue whatever the epilogue does with it: in statistics mode
    // (identity epilogue, table unused) hand them readable memory - the statistics buffer itself (>= cout floats)
    if (stats != nullptr) { a.scale = stats; a.shift = stats; }
    if (want_stats && (d->act != YOLO_ACT_NONE || d->out_mode != YOLO_OUT_NHWC || (!bs && (d->flags & YOLO_FLAG_RESIDUAL))))
        return dry ? YOLO_OK : fail(YOLO_ERR_ARG, "conv (16-bit): statistics need the identity epilogue (raw convolution output)");
    if (bs) {                                               // backward statistics: sums over the gradient this launch writes
        if (!want_stats) return fail(YOLO_ERR_ARG, "conv (16-bit): backward statistics without a statistics buffer");
        if (d->stride != 1) return dry ? YOLO_OK : fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): backward statistics: stride-1 input gradients only");
        if (!dry) {
            if (!bs->z || !bs->mean || !bs->scale || !bs->shift) return fail(YOLO_ERR_ARG, "conv (16-bit): backward statistics: null pointer");
            if ((bs->z_ld & 7) || (bs->z_off & 7) || d->cout % 8) return fail(YOLO_ERR_ARG, "conv (16-bit): backward statistics: z_ld / z_off / channels must be multiples of 8");
            if (bs->act != YOLO_ACT_LEAKY && bs->act != YOLO_ACT_MISH) return fail(YOLO_ERR_ARG, "conv (16-bit): backward statistics: LeakyReLU or Mish block expected");
            a.bz = (const unsigned short*)bs->z; a.bz_ld = bs->z_ld; a.bz_off = bs->z_off;
            a.bmean = bs->mean; a.bscale = bs->scale; a.bshift = bs->shift; a.bact = bs->act;
        }
    }
    a.Cin = d->cin; a.Cout = d->cout;
    a.nchunks = d->cin / 32;
    a.act = d->act; a.out_mode = d->out_mode; a.flags = d->flags;
    a.x_ld = d->x_ld; a.x_off = d->x_off; a.y_ld = d->y_ld; a.y_off = d->y_off; a.r_ld = d->r_ld; a.r_off = d->r_off;
    const int pad = d->ksize / 2;
    a.Hin = d->h; a.Win = d->w;
    a.Ho = (d->h + 2 * pad - d->ksize) / d->stride + 1;
    a.Wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
    if (d->stride == 2 && ((d->h & 1) || (d->w & 1))) return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): stride 2 needs even H, W");
    const long long M = (long long)d->n * a.Ho * a.Wo;
    if (M > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "conv: N*H*W exceeds int32");
    int prmax = 1;
    // (tile ids of the 16-bit kernels: kTileH16* in common.h)
    const bool dma_ok = d->ksize == 3 && d->stride == 1 && d->cout > 64 && d->cin <= 2048 && d->cout % 8 == 0 && d->out_mode != YOLO_OUT_HEAD &&
                        (d->y_ld & 7) == 0 && (d->y_off & 7) == 0 && (!residual || ((d->r_ld & 7) == 0 && (d->r_off & 7) == 0));
    // 1x1 with >= 128 output channels and >= 4 K steps: conv1_dma_h16 (tile 8 / default); tiles 5, 6 keep conv_patch_h16
    const bool dma1_ok = d->ksize == 1 && d->stride == 1 && d->cout >= 128 && d->cin >= 128 && d->cout % 8 == 0 && d->out_mode != YOLO_OUT_HEAD &&
                         (d->y_ld & 7) == 0 && (d->y_off & 7) == 0 && (!residual || ((d->r_ld & 7) == 0 && (d->r_off & 7) == 0));
    if (d->tile == kTileH16Dma && !dma_ok && !dma1_ok)
        return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): tile 8 needs 3x3 stride 1 with more than 64 output channels, or 1x1 with >= 128 input and output channels");
    // (tile 10 is an A/B id of conv3_dma_h16 alone: on any other convolution it used to run conv_patch_h16 without a word)
    if (d->tile == kTileH16DmaIdentQuads && !dma_ok)
        return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): tile 10 needs 3x3 stride 1 with more than 64 output channels and 16-byte rows");
    const bool use_dma = dma_ok && (d->tile >= kTileH16Dma || (d->tile == 0 && !switches().no_dma));
    if (d->tile == kTileH16Ws && !ws_eligible(d, residual)) return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): tile 14 needs a 3x3 32 -> 64 (stride 1 / 2) or 64 -> 32 (stride 1) layer, NHWC");
    if (!want_stats && ws_eligible(d, residual)) return conv_ws_launch(d, x, wf, scale, shift, residual, y, nan_flag, s);
    if (want_stats && !bs && ws_eligible(d, residual)) {            // train-mode forward of the <= 64-channel 3x3 blocks: one row per wave
        if (const int rows = ws_stats_rows(d)) {
            if (const int r = stats_rows(rows, a.stats_ld, rows_ld, dry, stats_bytes)) return r < 0 ? r : YOLO_OK;
            return conv_ws_launch(d, x, wf, stats, stats, nullptr, y, nan_flag, s, stats, a.stats_ld);
        }
    }
    // lane quad -> pixel quad of a 32-pixel m-tile. Identity makes every patch ds_read_b128 2-way bank-conflicted with the 32x4
    // pixel tiles of 52x52 / 104x104 (its two 16-lane groups are quads {0,3,5,6} and {1,2,4,7}: 4 rows whose patch offsets collide
    // mod 16); sending even tile rows to one group and odd rows to the other removes that, and measured 1-4 % at every size
    // (profiles/r02/ab_quad_permutation.txt). Tile 10 keeps the identity map for A/B.
    a.qperm = d->tile == kTileH16DmaIdentQuads ? 0x76543210u : 0x76452310u;
    a.cls_ph = 0;                                           // (the MASK kernels' output parity: dgrad_s2_h16_launch)
    if (dma1_ok && (d->tile == kTileH16Dma || (d->tile == 0 && !switches().no_dma))) {
        gemm_view(a, (int)M, 1, 128, 128, 1);
        if (want_stats)
            if (const int r = stats_rows(2 * ceil_div(a.W, 128), a.stats_ld, rows_ld, dry, stats_bytes)) return r < 0 ? r : YOLO_OK;
        return launch_dma1(a, 0, d->dtype, s);
    }
    // 3x3 stride 2 with >= 128 output channels: conv1_dma_h16 as a GEMM with gathered rows (tile 0 / 13; tiles 5, 6 keep conv_patch_h16)
    const bool s2_ok = d->ksize == 3 && d->stride == 2 && d->cout >= 128 && d->cout % 8 == 0 && d->out_mode == YOLO_OUT_NHWC &&
                       (d->y_ld & 7) == 0 && (d->y_off & 7) == 0 && (!residual || ((d->r_ld & 7) == 0 && (d->r_off & 7) == 0)) &&
                       (long long)a.Ho * a.Wo < 0x7fffffffLL && d->cin * 9 / 32 >= 4;
    if (d->tile == kTileH16S2Gemm && !s2_ok) return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): tile 13 needs 3x3 stride 2 with >= 128 output channels");
    if (s2_ok && (d->tile == kTileH16S2Gemm || (d->tile == 0 && !switches().no_dma && !switches().no_s2_dma))) {
        gemm_view(a, (int)M, 1, a.Wo, a.Ho * a.Wo, 9);
        if (want_stats)
            if (const int r = stats_rows(2 * ceil_div(a.W, 128), a.stats_ld, rows_ld, dry, stats_bytes)) return r < 0 ? r : YOLO_OK;
        return launch_dma1(a, 1, d->dtype, s);
    }
    if (want_stats && !use_dma) return dry ? YOLO_OK : fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): no fused-statistics kernel for this convolution");
    if (d->ksize == 1) {
        a.H = 1; a.W = (int)M; a.rows_total = 1; a.TH = 1; a.TW = 128; a.PC = 128;
    } else {
        a.H = a.Ho; a.W = a.Wo; a.rows_total = d->n * a.Ho;
        pick_tile_h(d->h, a.Ho, a.Wo, 3, d->stride, &a.TH, &a.TW, &prmax, use_dma ? D_PATCH_PIX : H_PATCH_CAP);
        a.PC = d->stride * (a.TW - 1) + 3;
    }
    if (use_dma) {
        if (prmax * a.PC > D_PATCH_PIX) return fail(YOLO_ERR_UNSUPPORTED, "conv3_dma_h16: patch of %d pixels", prmax * a.PC);
        a.patch_cap = D_PATCH_PIX;
        a.tiles_w = ceil_div(a.W, a.TW);
        a.KT = a.nchunks * 9;
        a.nc5 = d->out_mode == YOLO_OUT_HEAD ? d->cout / 3 : 1;
        if (want_stats)
            if (const int r = stats_rows(2 * a.tiles_w * ceil_div(a.rows_total, a.TH), a.stats_ld, rows_ld, dry, stats_bytes)) return r < 0 ? r : YOLO_OK;
        return launch_dma(a, d->dtype, s);
    }
    // Not rounded up to the staging granularity of 64 pixels (the stores are guarded): measured with per-block stamps, a CU
    // never held more than TWO of the 64-wide 3x3 blocks although registers and the occupancy API allow three — their
    // 2 x 256 x 80 B = 41.5 KB of LDS did not pack three to a CU (consistent with allocations not straddling the two 80 KB
    // halves of the 160 KB LDS: 2 x 41.5 KB > 80 KB), while the 36.4 KB 1x1 blocks did run three deep.
    a.patch_cap = round_up(prmax * a.PC, 8);
    if (a.patch_cap < 224) a.patch_cap = 224;              // epilogue stages 128 x 68 fp32 in the patch region
    if (a.patch_cap > H_PATCH_CAP) return fail(YOLO_ERR_UNSUPPORTED, "conv (16-bit): patch too large");
    a.tiles_w = ceil_div(a.W, a.TW);
    a.KT = a.nchunks * d->ksize * d->ksize;
    a.nc5 = d->out_mode == YOLO_OUT_HEAD ? d->cout / 3 : 1;
    // measured (tools/conv_bench.py --dtype bf16 --tile 5,6, batch 32): 1x1 layers are latency/HBM-bound and want more,
    // smaller blocks (BN = 64); every 3x3 with more than 64 output channels gains from BN = 128 (64->128 @104: 81 vs 98 us,
    // 64->128 s2 @208: 119 vs 131 us, 13x13 .. 52x52: 15-20 %) - the earlier "only up to 52x52" rule predated the epilogue fixes
    const int auto_bn = (d->ksize == 3 && d->cout > 64) ? 128 : 64;   // same-box A/B of the whole forward: +0.7 % at 416x416, +3.8 % at 608x608
    const int bn = d->tile == kTileH16PatchBn64 ? 64 : (d->tile == kTileH16PatchBn128 ? 128 : auto_bn);
    return launch_h(a, d->ksize, d->stride, bn, d->dtype, s);
}

}  // namespace yolo
