/* yolo_mi355x.h — C ABI of libyolo_mi355x.so (MI355X / gfx950 YOLOv3 hot path).
 *
 * The reference (GabeTsai/YOLO-For-Turbines) has no FFI/plugin layer: its boundary is the
 * Python call surface of code/model.py and code/utils.py. Every entry point
 * below states which reference routine's arithmetic it replaces. The host-side mirror of the
 * reference interface (same class / function names) lives in yolo_for_turbines_amd/ and calls
 * these through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - all data pointers are DEVICE pointers (tensor.data_ptr()); the caller owns every buffer,
 *    including workspaces; the library allocates nothing and keeps no mutable global state
 *    except a thread-local error string;
 *  - `stream` is a hipStream_t passed as void*; every function only enqueues work on it and
 *    never synchronises the device;
 *  - return value 0 = ok, negative = error (message: yolo_last_error()).
 *  - activations are NHWC ("pixel-major"): element (n,h,w,c) of a tensor with channel stride
 *    `ld` and channel offset `off` lives at ((n*H + h)*W + w)*ld + off + c. A concat buffer is
 *    simply one allocation with a larger `ld` that several producers write slices of.
 */
#ifndef YOLO_MI355X_H
#define YOLO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YOLO_OK 0
#define YOLO_ERR_ARG (-1)
#define YOLO_ERR_UNSUPPORTED (-2)
#define YOLO_ERR_LAUNCH (-3)
#define YOLO_ERR_WORKSPACE (-4)

enum { YOLO_F32 = 0, YOLO_F16 = 1, YOLO_BF16 = 2 };
enum { YOLO_ACT_NONE = 0, YOLO_ACT_LEAKY = 1, YOLO_ACT_MISH = 2 };
/* where the epilogue writes: plain NHWC; NHWC with nearest 2x upsample (each value goes to its
 * 2x2 destination pixels, replaces nn.Upsample + the first half of torch.cat, model.py:189-191,
 * 222); or the detection-head layout (B,3,g,g,5+nc) contiguous (replaces the reshape + permute
 * of ScalePredictionBlock.forward, model.py:145-148; conv channel = a*(5+nc)+k). */
enum { YOLO_OUT_NHWC = 0, YOLO_OUT_UPSAMPLE2X = 1, YOLO_OUT_HEAD = 2 };
/* YOLO_FLAG_FILTERS_READY (layers of the Winograd F(4x4) family, tile 15, only): w_packed is not the packed weight buffer but the
 * transformed filters U4 that yolo_wino4_filters made of it.
 * YOLO_FLAG_FILTERS_APPENDED (the same layers): w_packed is the packed weight buffer, and U4 lies behind the packed weights in the
 * same buffer, at yolo_packed_weight_bytes(cout, cin, 3, YOLO_F32) rounded up to 16 (yolo_wino4_appended_bytes of room in all);
 * yolo_wino4_filters(d, w, (char*)w + that offset) made it in place. Same bits as the launch without the flag. It is also the one
 * flag the tile heuristic reads: a caller that brings finished filters gets tile 15 on the small maps that measured faster that
 * way (yolo_conv_pick_tile, yolo_conv_workspace_bytes and the launch agree; without the flag nothing changes). Accepted on fp32
 * descriptors that run as tile 15 with its workspace (a forced tile 15 honours it on any shape tile 15 supports), else an
 * argument error; together with YOLO_FLAG_FILTERS_READY, YOLO_FLAG_SPLIT_BF16, YOLO_FLAG_SPLIT_WEIGHTS_READY or YOLO_FLAG_SPLIT_K
 * it is refused with YOLO_ERR_UNSUPPORTED.
 * YOLO_FLAG_SPLIT_BF16 (fp32 layers of the direct kernels only: ksize 1 or 3, stride 1 or 2, cin a multiple of 32, no Winograd
 * workspace in play): the products run on the bf16 matrix cores. Each fp32 operand is split exactly into three bf16 values and six
 * of the nine partial products are accumulated in fp32, in one fixed order: the result has the accuracy of the fp32 kernel
 * (measured: DESIGN 4.13) but not its bits. Deterministic, and independent of the batch on finite data. A block of the output (up
 * to 128 pixels x 128 channels, possibly of two images) that reads an Inf or a NaN is computed with exact fp32 products, all of
 * it. tile: 0 = heuristic, 1 / 2 / 4 = 128x128 / 128x64 / 64x64 blocks. On any other descriptor the flag is refused with
 * YOLO_ERR_UNSUPPORTED. Without the flag nothing changes.
 * YOLO_FLAG_SPLIT_WEIGHTS_READY (together with YOLO_FLAG_SPLIT_BF16 only): w_packed is the buffer that yolo_split3_weights made, the
 * packed weights with their bf16 planes behind them, for weights that stay the same from call to call. Same bits as the launch
 * without it. Anywhere else the flag is refused with YOLO_ERR_UNSUPPORTED.
 * YOLO_FLAG_SPLIT_K (fp32 descriptors with ksize 1 or 3, stride 1 or 2, cin a multiple of 32 and tile 0; any act, out_mode, residual):
 * the launch for small batches. K is cut into S slices (yolo_conv_splitk_slices: a function of h, w, cin, cout, ksize, stride alone,
 * never of n or of the device); one launch writes the S partial sums of every output value into the caller's workspace, a second adds
 * them in ascending slice order and applies the epilogue. Exact fp32 products, no atomics on floats: deterministic, an image's bits
 * do not depend on its batch; fp32 accuracy, but not the bits of the launch without the flag (the sum is ordered differently). It
 * runs whatever Winograd or the bf16 split would have chosen, through yolo_conv_fwd_ws / yolo_conv_fwd_batch with the workspace
 * yolo_conv_workspace_bytes asks for (16-byte aligned), else YOLO_ERR_WORKSPACE (always from yolo_conv_fwd, which has none).
 * Together with YOLO_FLAG_FILTERS_READY, YOLO_FLAG_FILTERS_APPENDED, YOLO_FLAG_SPLIT_BF16 or YOLO_FLAG_SPLIT_WEIGHTS_READY, with a forced tile, on a 16-bit
 * descriptor or with cin of 3 or 4 the flag is refused with YOLO_ERR_UNSUPPORTED and nothing is launched. Without the flag nothing
 * changes.
 * YOLO_FLAG_WINO_SPLIT_BF16 (fp32 descriptors that run as tile 15 with its workspace, cin a multiple of 32, together with
 * YOLO_FLAG_FILTERS_READY or YOLO_FLAG_FILTERS_APPENDED): the 36 Winograd GEMMs run on the bf16 matrix cores. The transform pass
 * writes V4 as three bf16 planes per value (the exact split of YOLO_FLAG_SPLIT_BF16) and splits the caller's fp32 U4 the same way,
 * on every launch, into the workspace behind them; six of the nine partial products are accumulated in fp32 in one fixed order. fp32
 * accuracy (measured: DESIGN 4.15) but not the bits of the launch without the flag. Deterministic; an image's bits do not depend on
 * its batch on finite data. An Inf or a NaN in x or in the filters turns every output it reaches into NaN (YOLO_FLAG_NANCHECK sees
 * it). w_packed stays what the filter flag says; yolo_conv_workspace_bytes reports the planes, 36 * cin * (tiles_pad64 + cout_pad64)
 * * 6 bytes. Together with YOLO_FLAG_SPLIT_K, YOLO_FLAG_SPLIT_BF16 or YOLO_FLAG_SPLIT_WEIGHTS_READY, without a filter flag, or on any
 * other descriptor the flag is refused with YOLO_ERR_UNSUPPORTED. Without the flag nothing changes.
 * YOLO_FLAG_FILTER_PLANES (next to YOLO_FLAG_FILTERS_READY or YOLO_FLAG_FILTERS_APPENDED, on fp32 descriptors that run as tile 15 with
 * its workspace and cin a multiple of 32): directly behind the U4 this launch uses, at U4 + yolo_wino4_filter_bytes(d), lie its bf16
 * planes, yolo_wino4_filter_plane_bytes(d) of them, as yolo_wino4_filter_planes made them. It describes the buffer, as the two
 * filter flags do. With YOLO_FLAG_WINO_SPLIT_BF16 the transform pass then splits no filters (its trailing blocks only read the planes,
 * so that they come from the memory-side cache when the GEMMs ask for them), the GEMMs read the filter planes from there, and the
 * part of the workspace behind the V planes is not touched: the same bits as the launch without the flag.
 * Without YOLO_FLAG_WINO_SPLIT_BF16 it is accepted and ignored. yolo_conv_workspace_bytes does not change with it. Anywhere else
 * (without a filter flag, on a layer that does not run as tile 15, with cin not a multiple of 32) it is an argument error. */
enum { YOLO_FLAG_RESIDUAL = 1, YOLO_FLAG_NANCHECK = 2, YOLO_FLAG_FILTERS_READY = 4, YOLO_FLAG_SPLIT_BF16 = 8,
       YOLO_FLAG_SPLIT_WEIGHTS_READY = 16, YOLO_FLAG_SPLIT_K = 32, YOLO_FLAG_FILTERS_APPENDED = 64, YOLO_FLAG_WINO_SPLIT_BF16 = 128,
       YOLO_FLAG_FILTER_PLANES = 256 };

/* One fused block: y = [residual +] act(scale[c] * conv(x, w)[c] + shift[c]).
 * Replaces CNNBlock.forward (model.py:80-86: Conv2d -> BatchNorm2d(eval) -> LeakyReLU/Mish, or
 * bare Conv2d + bias) and the `x + layer(x)` of ResidualBlock.forward (model.py:115-121).
 * BN is folded by yolo_bn_fold(); a bare conv passes scale = 1, shift = bias. */
typedef struct yolo_conv_desc {
    int32_t n, h, w;        /* input batch, height, width                                  */
    int32_t cin, cout;      /* logical channel counts                                      */
    int32_t ksize, stride;  /* 1 or 3 (padding = ksize/2, model.py:201); 1 or 2            */
    int32_t x_ld, x_off;    /* input channel stride / offset (elements)                    */
    int32_t y_ld, y_off;    /* output  "   (ignored for YOLO_OUT_HEAD)                     */
    int32_t r_ld, r_off;    /* residual "  (YOLO_FLAG_RESIDUAL), same spatial size as y    */
                            /* YOLO_F16 / YOLO_BF16: x_ld and x_off must be multiples of 8 (16-byte input rows), else      */
                            /* YOLO_ERR_ARG. y_ld, y_off, r_ld and r_off may have any value: with all of them multiples    */
                            /* of 8 the stores move 8 channels at a time and the faster kernel families are open; any      */
                            /* other view is written element by element, same values. Base pointers: 16-byte aligned.      */
                            /* The same holds for dz (as x) and dx / residual (as y / r) of yolo_conv_dgrad_s2.            */
    int32_t act;            /* YOLO_ACT_*                                                  */
    int32_t out_mode;       /* YOLO_OUT_*                                                  */
    int32_t dtype;          /* YOLO_F32, YOLO_F16 or YOLO_BF16: activations (x, residual, y) and   */
                            /* packed weights; accumulation, scale/shift and heads stay fp32       */
    int32_t flags;          /* YOLO_FLAG_*                                                 */
    int32_t tile;           /* 0 = library heuristic; else forced tile id 1 .. 15 (tuning/tests) */
} yolo_conv_desc;

/* One queued launch for yolo_conv_fwd_batch (pointers as 64-bit integers so the table can be
 * built once per input shape on the host and replayed every forward). */
typedef struct yolo_conv_op {
    yolo_conv_desc d;
    uint64_t x, w_packed, scale, shift, residual, y;
    uint64_t workspace, workspace_bytes;   /* yolo_conv_workspace_bytes(&d); 0 / 0 = none (direct kernels only) */
} yolo_conv_op;

const char* yolo_last_error(void);
/* 101: the six SGD step entry points of 100 (by value, _hp, _amp, _hp_ema, _amp_ema, _clip) are one, yolo_sgd_step, with the
 * argument list the _clip one had and clip_state_dev optional like every other option.
 * 102: yolo_wgrad_plan; yolo_conv_wgrad refuses a channel slice that does not fit its buffer and, for 16-bit dtypes, operands or a
 * workspace that are not 16-byte aligned.
 * 104: yolo_conv_patch_plan; conv_patch_f32 (tiles 5 - 7) writes y / residual views that are not multiples of 4 element by element. */
int yolo_version(void);
/* The A/B environment switches (INTEGRATION.md has the table) are read once, when the library is loaded. This writes what was
 * read as "NAME=value\n" per switch, in the table's order (a boolean is 0 / 1 in the sense of its name: YOLO_NO_DMA=1 means the
 * DMA kernels are off), at most cap - 1 characters and a terminating 0; returns the length the whole text needs. */
int yolo_switches_describe(char* buf, size_t cap);

/* ---- weights (replaces nothing arithmetic: layout change of nn.Conv2d.weight, OIHW fp32,
 *      as filled by the Darknet loader model.py:293-305) ---------------------------------- */
/* elements of the packed buffer. It holds (1) the row-major matrix [cout_pad128][K_pad32],
 * K index = (kh*k + kw)*cin_pad + ci (channels innermost, matching NHWC gathers), used by the
 * register-staged kernel, and, when cin % 32 == 0, (2) a copy in MFMA-fragment order
 * [cout_pad128/32][cin/32][k*k][4][64 lanes][4] streamed straight into registers by the
 * stride-1 patch kernel, and, when ksize == 3 and cin % 4 == 0, (3) the Winograd-domain filters
 * G g G^T as [16][cin/4][cout_pad64][4] (yolo_conv_fwd_ws). */
size_t yolo_packed_weight_elems(int cout, int cin, int ksize);
/* bytes of the packed buffer for a dtype. YOLO_F16 / YOLO_BF16: fragment order for
 * v_mfma_f32_32x32x16_{f16,bf16}: [cout_pad128/32][cin/32][k*k][2][64 lanes][8 halfs] (cin % 32 == 0). */
size_t yolo_packed_weight_bytes(int cout, int cin, int ksize, int dtype);
int yolo_pack_weights(const float* w_oihw, void* w_packed, int cout, int cin, int ksize, int dtype, void* stream);
/* Many layers at once (every weight tensor changes at `optimizer.step()`, train.py:68): items is a HOST array. 16-bit dtypes:
 * one launch per 48 items. dgrad = 0: the layout of yolo_pack_weights; dgrad = 1: of yolo_pack_weights_dgrad(flip = 1)
 * (stride-1 layers only). fp32: the per-item functions are called in turn. */
typedef struct yolo_pack_item { const float* w_oihw; void* w_packed; int cout, cin, ksize, reserved; } yolo_pack_item;
int yolo_pack_weights_batch(const yolo_pack_item* items, int n, int dgrad, int dtype, void* stream);
/* inverse (for gradients / checkpoint export): packed -> OIHW */
int yolo_unpack_weights(const void* w_packed, float* w_oihw, int cout, int cin, int ksize, int dtype, void* stream);
/* scale = gamma / sqrt(var + eps), shift = beta - mean * scale (nn.BatchNorm2d eval,
 * model.py:61,84). gamma == NULL: scale = 1, shift = beta (bias of a bare conv, model.py:86). */
int yolo_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                 float* scale, float* shift, int c, void* stream);

/* ---- layout boundary ------------------------------------------------------------------- */
/* (N,C,H,W) fp32 -> NHWC with c_pad >= C channels (extra channels zero). Sets *nan_flag |= 1 if
 * any input element is NaN (the `assert torch.sum(torch.isnan(x)) == 0` of model.py:175). */
int yolo_nchw_to_nhwc(const float* x, void* y, int n, int c, int h, int w, int c_pad, int dtype,
                      int32_t* nan_flag, void* stream);
int yolo_nhwc_to_nchw(const void* x, float* y, int n, int c, int h, int w, int x_ld, int x_off, int dtype, void* stream);

/* ---- stem: layers[0] (3 -> 32, 3x3, stride 1) straight from the NCHW input ---------------- */
/* Replaces CNNBlock.forward for the first block (model.py:20-21,80-86) together with the
 * NCHW -> NHWC conversion and the NaN-input guard (model.py:175): x_nchw (N,3,H,W) fp32 ->
 * y NHWC in `dtype` (fp32, or fp16/bf16 for the 16-bit path; ld/off like yolo_conv_desc). Direct VALU
 * convolution in fp32: the layer is bound by its output
 * bytes, not by FLOPs. Weights as [27][cout] (yolo_stem_pack from OIHW). *nan_flag |= 1 for a NaN
 * input element, |= 2 for a NaN output. */
int yolo_stem_supported(int cin, int cout, int ksize, int stride);
int yolo_stem_pack(const float* w_oihw, float* w_k_major, int cout, void* stream);
int yolo_stem_fwd(const float* x_nchw, const float* w_k_major, const float* scale, const float* shift, void* y,
                  int n, int h, int w, int cout, int y_ld, int y_off, int act, int dtype, int32_t* nan_flag, void* stream);

/* ---- convolution blocks ---------------------------------------------------------------- */
/* nan_flag: *nan_flag |= 2 when YOLO_FLAG_NANCHECK is set and an output element is NaN
 * (the per-layer `raise ValueError("Nan in layer")` of model.py:183-184, checked once by host). */
int yolo_conv_fwd(const yolo_conv_desc* d, const void* x, const void* w_packed, const float* scale,
                  const float* shift, const void* residual, void* y, int32_t* nan_flag, void* stream);
int yolo_conv_fwd_batch(const yolo_conv_op* ops, int n_ops, int32_t* nan_flag, void* stream);
/* The same block with a caller-owned workspace. The fp32 3x3 stride-1 blocks with >= 64 input channels (the second convolution
 * of the residual units of model.py:115-121 at 104x104 ... 13x13, the 3x3 layers of the neck and of ScalePredictionBlock
 * model.py:140-143) then run as Winograd F(2x2, 3x3) - the algorithm PyTorch's backend itself picks for them: an input
 * transform pass into the workspace (16 planes of the 4x4 tiles, [xi][cin/4][tile][4]), 16 matrix products on the
 * transformed filters (third section of the packed fp32 buffer: [xi][cin/4][cout_pad64][4]) and the output transform in the
 * epilogue; 1 / 2.25 of the direct convolution's multiplications, same result within a few ulp of the transforms'
 * additions. yolo_conv_workspace_bytes: what descriptor d needs (0 = the launch takes no workspace); a NULL or smaller
 * workspace makes tile 0 fall back to the direct kernels of yolo_conv_fwd, tile 13 (= Winograd, forced) fail.
 * Streams that run concurrently need a workspace each.
 * With YOLO_FLAG_SPLIT_K set on d: the partial sums, S * n * Ho * Wo * cout_pad4 * 4 bytes, S = yolo_conv_splitk_slices(d), cout_pad4 =
 * cout rounded up to 4 (it grows linearly with the batch); 0 wherever a launch of d would refuse the flag (its shape or dtype, a forced
 * tile, one of the other kernel flags next to it). */
size_t yolo_conv_workspace_bytes(const yolo_conv_desc* d);
int yolo_conv_fwd_ws(const yolo_conv_desc* d, const void* x, const void* w_packed, const float* scale, const float* shift,
                     const void* residual, void* y, void* workspace, size_t workspace_bytes, int32_t* nan_flag, void* stream);
/* tile id the heuristic would pick (exposed for tests / tuning) and number of tile ids */
int yolo_conv_pick_tile(const yolo_conv_desc* d);
int yolo_conv_num_tiles(void);
/* YOLO_FLAG_SPLIT_BF16 for plans (flags and tile of d are not looked at; the layer's shape only, never the batch).
 * yolo_conv_split3_supported: 1 when the library honours the flag on a tile-0 launch of d that brings the workspace
 * yolo_conv_workspace_bytes asks for. yolo_conv_split3_eligible: 1 when, in addition, the shape measured faster that way than
 * on its exact kernel: what an inference plan should flag. */
int yolo_conv_split3_supported(const yolo_conv_desc* d);
int yolo_conv_split3_eligible(const yolo_conv_desc* d);
/* YOLO_FLAG_SPLIT_K for plans (n, flags and tile of d are not looked at). yolo_conv_splitk_supported: 1 when the library honours the
 * flag on d's shape and dtype. yolo_conv_splitk_eligible: 1 when, in addition, the shape measured faster that way at batch 1 than on
 * the kernel a default plan gives it: what a latency-mode plan should flag. yolo_conv_splitk_slices: the number of K slices S (1 ..
 * 32) such a launch uses, 0 where unsupported. */
int yolo_conv_splitk_supported(const yolo_conv_desc* d);
int yolo_conv_splitk_eligible(const yolo_conv_desc* d);
int yolo_conv_splitk_slices(const yolo_conv_desc* d);
/* YOLO_FLAG_SPLIT_BF16 with the weights split once instead of by every block of every launch (inference).
 * yolo_split3_weights reads the row-major fp32 section of w_packed (yolo_pack_weights, YOLO_F32) and writes the prepared buffer:
 *     [the packed weights, P = yolo_packed_weight_bytes(cout, cin, ksize, YOLO_F32) rounded up to 16 bytes]
 *     [K step = K_pad32 / 32][plane: hi, mid, lo][cout_pad128][64 bytes]
 *     [cout_pad128 / 32] 32-bit words
 * The planes hold the three bf16 parts of every weight (the truncation split of the kernel itself: w = hi + mid + lo exactly). A
 * 64-byte row holds the 32 k of the step as four 16-byte slots of 8 bf16 (k ascending), slot s of output channel n stored at slot
 * s ^ ((n >> 2) & 3): the kernel's LDS image, so the rows of one (K step, plane) that a block needs are contiguous and copied as
 * they are. Rows from cout up to cout_pad128 are zero. Word g of the table is 1 when a weight of output channels 32 g .. 32 g + 31
 * is an Inf or a NaN, else 0; a block whose channels have a word set is computed with exact fp32 products, as a launch on the
 * packed weights would, and reads the fp32 weights for that from the copy in front. out == w_packed prepares in place (the
 * packed buffer then needs yolo_split3_weight_bytes of room; one launch): the same pointer serves launches with and without the
 * flag. Otherwise the packed weights are copied to the front of out first; the two may not overlap. The planes add 6 bytes per
 * weight of the padded matrix:
 *     yolo_split3_weight_bytes = P + K_pad32 / 32 * 3 * cout_pad128 * 64 + cout_pad128 / 32 * 4,
 * or 0 where yolo_conv_split3_supported(d) is 0 (only the shape of d is looked at). out: 16-byte aligned. A descriptor with
 * YOLO_FLAG_SPLIT_BF16 | YOLO_FLAG_SPLIT_WEIGHTS_READY then takes that buffer as its w_packed. */
size_t yolo_split3_weight_bytes(const yolo_conv_desc* d);
int yolo_split3_weights(const yolo_conv_desc* d, const void* w_packed, void* out, void* stream);
/* Winograd F(4x4, 3x3) (tile 15) with the filters transformed once instead of on every launch, for weights that stay the same
 * from call to call (inference). yolo_wino4_filter_bytes: size of U4 = G g G^T, 36 * cin4_pad2 * cout_pad64 * 16 bytes (it
 * depends on cin and cout only; 0: the descriptor cannot run as tile 15). yolo_wino4_filters writes U4 (16-byte aligned) from
 * w_packed (yolo_pack_weights, or yolo_pack_weights_dgrad with flip = 1): the very values a launch without the flag leaves behind
 * V4 in its workspace. A descriptor with YOLO_FLAG_FILTERS_READY then takes that U4 as the w_packed of yolo_conv_fwd_ws /
 * yolo_conv_fwd_batch; the workspace size stays what yolo_conv_workspace_bytes reports, its U4 part is left alone. The flag
 * on a descriptor that does not run as tile 15 is an argument error.
 * yolo_wino4_filters works in place: it reads only the row-major section at the start of w_packed (cout rows of K_pad32 floats),
 * so U4 may lie anywhere behind that section in the same buffer, in particular behind the packed bytes rounded up to 16, where
 * YOLO_FLAG_FILTERS_APPENDED expects it; a U4 that overlaps the section itself is an argument error.
 * yolo_wino4_appended_bytes: the room such a buffer needs, packed bytes rounded up to 16 plus yolo_wino4_filter_bytes (0: the
 * descriptor cannot run as tile 15). yolo_wino4_appended_wanted: 1 when the heuristic admits some small map of a layer with
 * these channel counts once YOLO_FLAG_FILTERS_APPENDED is set (cin, cout, ksize, stride, dtype only: the layers worth the room).
 * A descriptor with tile forced to 15 may have any cin that is a multiple of 4 (the transforms pad an odd count of channel quads
 * with a zero plane); the heuristic and every other tile keep the rule of the direct kernels, cin <= 4 or a multiple of 32. */
size_t yolo_wino4_filter_bytes(const yolo_conv_desc* d);
int yolo_wino4_filters(const yolo_conv_desc* d, const void* w_packed, void* U4, void* stream);
size_t yolo_wino4_appended_bytes(const yolo_conv_desc* d);
int yolo_wino4_appended_wanted(const yolo_conv_desc* d);
/* How a tile-15 launch is cut on the current device: *whole tile blocks (64 tiles each) run as one workgroup per channel block;
 * *half tile blocks, those of a last round that would fill at most half the compute units, run as two workgroups of 32 tiles.
 * The result of a tile does not depend on the cut. */
int yolo_conv_wino4_blocks(const yolo_conv_desc* d, int* whole, int* half);
/* How a launch of d on the patch kernel conv_patch_f32 (tile 5, 6 or 7; nothing is launched, no device is needed) is cut, from the
 * code the launch itself runs: out = { TH, TW (output rows x columns of a block's spatial tile; rows are global rows n * h + row, so a
 * tile may straddle images; a 1x1 runs as one row of n * h * w pixels in tiles of 128), PC (patch columns: TW + 2, or 128), the bound on a
 * tile's patch rows that the LDS patch is sized for, patch pixels per LDS buffer (of 36 floats each), tiles across the width, tiles
 * down the rows, workgroups }. YOLO_ERR_ARG for a tile that is not 5, 6 or 7 or a bad shape, YOLO_ERR_UNSUPPORTED where the
 * kernel does not run d (stride 2, cin not a multiple of 32, a patch that does not fit). */
int yolo_conv_patch_plan(const yolo_conv_desc* d, int tile, int32_t out[8]);
/* YOLO_FLAG_WINO_SPLIT_BF16 for plans (flags and tile of d are not looked at; the layer's shape only, never the batch).
 * yolo_conv_wino4_split_supported: 1 when the library honours the flag on the layer once it runs as tile 15 on finished filters.
 * yolo_conv_wino4_split_eligible: 1 when, in addition, the shape measured faster that way at batch 32 (the eval plan's list). */
int yolo_conv_wino4_split_supported(const yolo_conv_desc* d);
int yolo_conv_wino4_split_eligible(const yolo_conv_desc* d);
/* The bf16 planes of U4 made once instead of on every YOLO_FLAG_WINO_SPLIT_BF16 launch, for weights that stay the same from call to
 * call. yolo_wino4_filter_plane_bytes: 36 * cin * cout_pad64 * 6 (cin and cout only), or 0 where tile 15 does not honour
 * YOLO_FLAG_WINO_SPLIT_BF16 on the layer (not fp32 3x3 stride 1 with NHWC output, or cin not a multiple of 32).
 * yolo_wino4_filter_planes reads the finished fp32 U4 (yolo_wino4_filters) and writes its planes (both 16-byte aligned, not
 * overlapping): the very bytes a YOLO_FLAG_WINO_SPLIT_BF16 launch leaves behind the V planes in its workspace. Written directly
 * behind U4, at U4 + yolo_wino4_filter_bytes(d), they are what YOLO_FLAG_FILTER_PLANES names. */
size_t yolo_wino4_filter_plane_bytes(const yolo_conv_desc* d);
int yolo_wino4_filter_planes(const yolo_conv_desc* d, const void* U4, void* planes, void* stream);

/* ---- training: batch-statistics BatchNorm, activation, and the conv gradients ------------- */
/* All of these replace pieces of `grad_scaler.scale(loss).backward()` / the train-mode forward of
 * train.py:53-67 for the blocks of model.py:47-121 (nn.Conv2d, nn.BatchNorm2d(train), LeakyReLU /
 * Mish, skip add, nn.Upsample). Reductions are deterministic (fixed order, fp64 across threads). */
size_t yolo_bn_workspace_bytes(int m, int c);
/* Activation / gradient tensors (z, y, residual, dy, dz, x, dx, dup) are NHWC in `dtype` (YOLO_F32, or
 * YOLO_BF16 / YOLO_F16 for the autocast training path of train.py:53: 16-bit storage, fp32 arithmetic,
 * one rounding at the store); statistics, parameters and parameter gradients are always fp32.
 *
 * z: raw conv output, m = N*H*W pixels, c channels (ld/off as usual). Batch mean / biased variance ->
 * mean, invstd = 1/sqrt(var+eps), scale = gamma*invstd, shift = beta (the train kernels evaluate
 * (z - mean)*scale + shift in that order, like PyTorch); running stats are updated in place like
 * nn.BatchNorm2d (momentum, unbiased variance) unless the pointers are NULL. */
int yolo_bn_stats(const void* z, int m, int c, int ld, int off, const float* gamma, const float* beta, float momentum,
                  float eps, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                  float* shift, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The statistics pass fused into the producing convolution (16-bit kernels on LDS-DMA: 3x3 stride 1 with > 64 output channels,
 * 1x1 with >= 128 input and output channels): yolo_conv_fwd_stats = the raw convolution (identity epilogue: act NONE, no
 * residual, YOLO_OUT_NHWC) that also writes per-wave partial sums of z and z^2 (of the ROUNDED values it stores) as
 * stats[row][2][ld] fp32; yolo_bn_stats_from_partials = the second half of yolo_bn_stats on those rows (same outputs, fp64
 * across rows in a fixed order). yolo_conv_stats_rows: rows (and *ld) for a descriptor, 0 = no fused kernel for it. */
int yolo_conv_stats_rows(const yolo_conv_desc* d, int* ld);
int yolo_conv_fwd_stats(const yolo_conv_desc* d, const void* x, const void* w_packed, void* z, float* stats, size_t stats_bytes,
                        void* stream);
int yolo_bn_stats_from_partials(const float* partial, int rows, int ld, int m, int c, const float* gamma, const float* beta,
                                float momentum, float eps, float* running_mean, float* running_var, float* mean, float* invstd,
                                float* scale, float* shift, void* stream);
/* The BACKWARD reduction pass fused the same way. The gradient dy of a block's output is written last by the input-gradient
 * convolution of the first layer that consumes it (a stride-1 convolution with the flipped weights, identity epilogue,
 * optionally accumulating onto the running gradient); yolo_conv_dgrad_bstats is that launch (d = the descriptor yolo_conv_fwd
 * would get, act NONE, YOLO_OUT_NHWC, [YOLO_FLAG_RESIDUAL]) and ALSO writes per-wave partial sums of du and du * (z - mean),
 * du = dy * act'((z - mean) * scale + shift), over the ROUNDED dy it stores, for the block that produced the gradient's
 * tensor (its raw conv output z, its batch mean / scale / shift, act = LeakyReLU or Mish). stats[row][2][ld] fp32 as above,
 * followed by 3 * c floats of scratch. yolo_bn_act_bwd_rows = yolo_bn_act_bwd without its reduction pass, from those rows:
 * same dgamma / dbeta / dz. yolo_conv_bstats_rows: rows (and *ld) for a descriptor, 0 = no fused kernel for it. */
int yolo_conv_bstats_rows(const yolo_conv_desc* d, int* ld);
int yolo_conv_dgrad_bstats(const yolo_conv_desc* d, const void* dz, const void* w_packed, const void* residual, void* dx, const void* z,
                           int z_ld, int z_off, const float* mean, const float* scale, const float* shift, int act, float* stats,
                           size_t stats_bytes, void* stream);
int yolo_bn_act_bwd_rows(const void* dy, int dy_ld, int dy_off, const void* z, int z_ld, int z_off, const float* gamma,
                         const float* mean, const float* invstd, const float* scale, const float* shift, int m, int c, int act,
                         float* dgamma, float* dbeta, void* dz, int dz_ld, int dz_off, int dtype, float* rows, int nrows, int rows_ld,
                         void* stream);
/* y = act((z - mean)*scale + shift) [+ residual] (mean may be NULL = 0); out_mode YOLO_OUT_NHWC or
 * YOLO_OUT_UPSAMPLE2X. */
int yolo_bn_act_fwd(const void* z, int z_ld, int z_off, const float* mean, const float* scale, const float* shift, const void* residual,
                    int r_ld, int r_off, void* y, int y_ld, int y_off, int n, int h, int w, int c, int act, int out_mode,
                    int dtype, int32_t* nan_flag, void* stream);
/* Backward of act(BN(z)): dy -> dgamma, dbeta, dz (gradient of the raw conv output). gamma == NULL:
 * bare conv (model.py:86) -> only dbeta (= bias gradient) is produced and dz is dy itself. */
int yolo_bn_act_bwd(const void* dy, int dy_ld, int dy_off, const void* z, int z_ld, int z_off, const float* gamma,
                    const float* mean, const float* invstd, const float* scale, const float* shift, int m, int c, int act,
                    float* dgamma, float* dbeta, void* dz, int dz_ld, int dz_off, int dtype, void* workspace, size_t workspace_bytes,
                    void* stream);
/* gradient of nn.Upsample(scale_factor=2): dx(n,h,w,c) = sum of the 2x2 destinations in dup(n,2h,2w,.) */
int yolo_upsample2x_bwd(const void* dup, int d_ld, int d_off, void* dx, int x_ld, int x_off, int n, int h, int w, int c,
                        int dtype, void* stream);
/* dW (OIHW fp32) = sum over pixels dz (x) x; n,h,w = INPUT dims of the conv; dz has the output dims.
 * dz: NHWC gradient of the raw conv output, channels [dz_off, dz_off + cout) of rows of dz_ld elements; x: NHWC conv input,
 * channels [x_off, x_off + cin) of rows of x_ld elements. Rules, checked before anything is launched (YOLO_ERR_ARG):
 *   - the four ld / off values are multiples of 4, and a slice lies inside its buffer: dz_off + cout <= dz_ld, x_off + cin <= x_ld;
 *   - the padding of a slice up to the next multiple of 4 channels (16-bit kernels: of 8) is read and must be zero; it must lie
 *     inside the row (x_ld >= cin rounded up to 4). Other neighbour channels are never read into a result;
 *   - 16-bit dtypes: dz, x and the workspace are 16-byte aligned.
 * A workspace smaller than yolo_wgrad_workspace_bytes is refused with YOLO_ERR_WORKSPACE. 16-bit operands whose four ld / off values
 * are multiples of 8 run on the bf16 / f16 matrix cores (three kernels, yolo_wgrad_plan says which), everything else on the f32
 * ones. Every kernel adds its K slices in a fixed order: two calls on the same operands give the same bits. */
size_t yolo_wgrad_workspace_bytes(int n, int h, int w, int cin, int cout, int ksize, int stride, int dtype);
int yolo_conv_wgrad(const void* dz, int dz_ld, int dz_off, const void* x, int x_ld, int x_off, float* dw_oihw, int n, int h,
                    int w, int cin, int cout, int ksize, int stride, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* What yolo_conv_wgrad will launch for these arguments and how the launch cuts the work (host only, nothing is launched; the same
 * decision function and launch plans as the call itself; YOLO_ERR_ARG where the call would refuse the shape or the ld / off values):
 *   out8[0] kernel, YOLO_WGRAD_KERNEL_*: F32 wgrad_f32_kernel (any dtype), PATCH wgrad_patch_h16, DMA wgrad3_dma_h16, STEM stem_wgrad_h16
 *   out8[1] dW tiles (STEM: 1)
 *   out8[2] K tiles: F32 steps of 32 pixels; PATCH / DMA tiles of 32 or 64 output pixels; STEM K steps of 16 pixels
 *   out8[3] K slices (STEM: workgroups)
 *   out8[4] K tiles per slice (STEM: K steps per wave)
 *   out8[5] fan-in of the reduce kernel: the G of wgrad_reduce<G> / wgrad_reduce_acc<G>; STEM: the strided parts of stem_wgrad_reduce
 *   out8[6] trailing slices (STEM: workgroups) that get no K tile and write zeros
 *   out8[7] DMA: the fragment look-ahead of the instantiation (3, or 5 under YOLO_WGRAD_LA=5); else 0 */
enum { YOLO_WGRAD_KERNEL_F32 = 0, YOLO_WGRAD_KERNEL_PATCH = 1, YOLO_WGRAD_KERNEL_DMA = 2, YOLO_WGRAD_KERNEL_STEM = 3 };
int yolo_wgrad_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int dtype, int dz_ld, int dz_off, int x_ld, int x_off,
                    int32_t* out8);
/* Test hook for the gfx950 transposing LDS read (ds_read_b64_tr_b16) the 16-bit wgrad kernel is built on:
 * in = [64][ld] 16-bit image; out[lane][8] = what lane receives as its 32x32x16 MFMA operand, i.e.
 * in[8*(lane/32) + e][lane%32]. */
int yolo_debug_tr_probe(const void* in, void* out, int ld, void* stream);
/* Weights of the input-gradient convolution, from the fp32 OIHW master weights. flip = 1: stride-1 convs —
 * the result is a packed buffer for yolo_conv_fwd (same dtype) with (cin' = cout rounded up to 32,
 * cout' = cin, same ksize, stride 1): dx = conv(dz, W'). flip = 0: operand of yolo_conv_dgrad_s2 in the same dtype
 * (fp32: row-major W'; 16-bit: four tap-subset fragment streams, one per output parity class). */
size_t yolo_packed_dgrad_bytes(int cout, int cin, int ksize, int flip, int dtype);
int yolo_pack_weights_dgrad(const float* w_oihw, void* w_packed, int cout, int cin, int ksize, int flip, int dtype, void* stream);
/* dx (n,2ho,2wo,cin) = transposed 3x3 stride-2 conv of dz (n,ho,wo,cout) [+ residual] */
int yolo_conv_dgrad_s2(const void* dz, int dz_ld, int dz_off, const void* w_packed, const void* residual, int r_ld, int r_off,
                       void* dx, int dx_ld, int dx_off, int n, int ho, int wo, int cin, int cout, int dtype, void* stream);
/* upstream gradient in the head layout (B,3,g,g,D) fp32, any strides -> NHWC (B,g,g,ld) in dtype, channel a*D+k, pads 0 */
int yolo_head_grad_to_nhwc(const float* dp, const int64_t* strides5, void* out, int b, int g, int d, int ld, int dtype, void* stream);
/* the same for a rectangular grid: (B,3,gh,gw,D) -> NHWC (B,gh,gw,ld); yolo_head_grad_to_nhwc is the gh = gw = g case */
int yolo_head_grad_to_nhwc_hw(const float* dp, const int64_t* strides5, void* out, int b, int gh, int gw, int d, int ld, int dtype,
                              void* stream);

/* ---- launch tables for the train-mode forward and the backward (train.py:41-82 run eagerly) -------------------------------- */
/* The reference's loop issues its step one Python statement at a time; here that is ~900 launches, and issued through an FFI
 * one by one the host is as slow as the GPU. A table of recorded calls is replayed by ONE call instead (the training
 * counterpart of yolo_conv_fwd_batch). yolo_call: fn = YOLO_FN_*, a[] = the arguments of that function in declaration order
 * WITHOUT the trailing stream: integers, size_t and pointers as 64-bit values, float arguments as the bits of a double.
 * Pointers inside a[] (descriptors, stride arrays, item tables) must stay valid while the table is in use.
 * yolo_reloc entries, sorted by call: at run time a[arg] of calls[call] is replaced by slots[slot] + offset - for the few pointers
 * that change from step to step (input batch, prediction tensors, upstream gradients). Stops at the first failing call. */
enum { YOLO_FN_FILL_ZERO = 1, YOLO_FN_COPY_D2D, YOLO_FN_NCHW_TO_NHWC, YOLO_FN_STEM_FWD, YOLO_FN_CONV_FWD, YOLO_FN_BN_STATS,
       YOLO_FN_BN_ACT_FWD, YOLO_FN_BN_ACT_BWD, YOLO_FN_UPSAMPLE2X_BWD, YOLO_FN_CONV_WGRAD, YOLO_FN_PACK_WEIGHTS_DGRAD,
       YOLO_FN_PACK_WEIGHTS_BATCH, YOLO_FN_CONV_DGRAD_S2, YOLO_FN_HEAD_GRAD_TO_NHWC, YOLO_FN_CONV_FWD_STATS,
       YOLO_FN_BN_STATS_FROM_PARTIALS, YOLO_FN_CONV_DGRAD_BSTATS, YOLO_FN_BN_ACT_BWD_ROWS, YOLO_FN_CONV_FWD_WS,
       YOLO_FN_HEAD_GRAD_TO_NHWC_HW };
#define YOLO_CALL_MAX_ARGS 24
typedef struct yolo_call { int32_t fn; int32_t reserved; uint64_t a[YOLO_CALL_MAX_ARGS]; } yolo_call;
typedef struct yolo_reloc { int32_t call, arg, slot, reserved; int64_t offset; } yolo_reloc;
int yolo_run_calls(const yolo_call* calls, int n_calls, const yolo_reloc* relocs, int n_relocs, const uint64_t* slots, int n_slots,
                   void* stream);
/* the two halves of a fine-tune step (train.py:54 forward in train mode, :67 backward): same table format */
int yolo_train_fwd_batch(const yolo_call* calls, int n_calls, const yolo_reloc* relocs, int n_relocs, const uint64_t* slots, int n_slots,
                         void* stream);
int yolo_train_bwd_batch(const yolo_call* calls, int n_calls, const yolo_reloc* relocs, int n_relocs, const uint64_t* slots, int n_slots,
                         void* stream);
/* stream-ordered memset(0) / device-to-device copy: the two non-kernel operations of the step, as table entries */
int yolo_fill_zero(void* p, size_t bytes, void* stream);
int yolo_copy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* ---- letterbox (config.py:101-113: LongestMaxSize -> centred PadIfNeeded(0) -> /255 -> CHW); parity with cv2 UNPINNED --- */
/* img: uint8 (h, w, 3) on the device; out: fp32 (3, size, size). new_hw / pad_tl (host pointers, may be NULL) receive the
 * resized size and the top / left padding, which un-letterboxing the boxes needs (utils.py:475-501). */
int yolo_letterbox(const unsigned char* img_hwc, int h, int w, int size, float* out_chw, int* new_hw, int* pad_tl, void* stream);
/* Canvas of a batch of n images (hw: host int32 [n][2] original sizes). rect = 0: (size, size). rect != 0: the smallest
 * multiples of 32 that hold every image resized so that its longer side is size (the resize rule of yolo_letterbox).
 * canvas_hw (host, out): [2]. */
int yolo_letterbox_canvas(const int32_t* hw, int n, int size, int rect, int32_t* canvas_hw);
/* yolo_letterbox onto a (canvas_h, canvas_w) canvas: same resize arithmetic, top / left padding = floor(diff / 2) per axis;
 * out: fp32 (3, canvas_h, canvas_w). yolo_letterbox is the canvas_h = canvas_w = size case. */
int yolo_letterbox_hw(const unsigned char* img_hwc, int h, int w, int size, int canvas_h, int canvas_w, float* out_chw, int* new_hw,
                      int* pad_tl, void* stream);

/* ---- ground-truth tensors (next to the hot path: dataset.py:119-161) ------------------------ */
/* boxes (B, max_boxes, 5) fp32 [x, y, w, h, class] normalised to [0,1), counts (B) valid boxes per image (list order
 * matters), anchors (9,2) normalised and scale-major (config.ANCHORS flattened). Writes the three target tensors
 * (B,3,g,g,6), g = S/32, S/16, S/8, rows [x_cell, y_cell, w_cells, h_cells, obj in {1,0,-1}, class] — zero-filled
 * here first. Same assignment rule and quirks as the reference loop (see csrc/targets.hip). */
int yolo_build_targets(const float* boxes, const int32_t* counts, int max_boxes, const float* anchors_9x2, int b, int image_size,
                       float ignore_iou, float* t0, float* t1, float* t2, void* stream);
/* The same for an (image_h, image_w) canvas (multiples of 32): target k is (B,3,gh_k,gw_k,6), per axis i = int(gh y),
 * j = int(gw x), rows [gw x - j, gh y - i, w gw, h gh, ...]; anchors are ranked by IoU of (w W/L, h H/L), L = max(H, W),
 * against the normalised anchors (the square canvas of side L with its padding cropped away). Square input: the same bits
 * as yolo_build_targets. */
int yolo_build_targets_hw(const float* boxes, const int32_t* counts, int max_boxes, const float* anchors_9x2, int b, int image_h,
                          int image_w, float ignore_iou, float* t0, float* t1, float* t2, void* stream);

/* ---- training augmentation (config.py:60-87 set_train_transforms, utils.py:503-662 mosaic_augmentation); parity with
 * cv2 / albumentations UNPINNED (see csrc/augment.hip) ------------------------------------------------------------------ */
/* Per-image parameter row, float64 (the draws of the transforms; the kernels hold no randomness). A switch is on when != 0.
 * mosaic: YOLO_AUG_MOSAIC + 2k, + 2k + 1 = (x, y) of cutout draw k, k < 10 (each in [0.2, 0.3]). */
#define YOLO_AUG_DO_HSV 0
#define YOLO_AUG_HUE 1
#define YOLO_AUG_SAT 2
#define YOLO_AUG_VAL 3
#define YOLO_AUG_DO_SSR 4
#define YOLO_AUG_SCALE 5
#define YOLO_AUG_DX 6
#define YOLO_AUG_DY 7
#define YOLO_AUG_DO_FLIP 8
#define YOLO_AUG_MOSAIC 9
#define YOLO_AUG_NPARAM 29
/* Tables. Host (read here, validated): hw [n_pool][2] source sizes, src [b][4] pool indices per output image: {i, -1, -1, -1}
 * = the standard transform of image i, four images = mosaic (square canvas only; all four must resize to the same size).
 * Device: the same hw / src (hw_dev, src_dev), params [b][YOLO_AUG_NPARAM], boxes [n_pool][max_in][5] yolo
 * (x, y, w, h, class) float64, nbox [n_pool] (-1 = no label file: letterbox only, count 0). Canvas (out_h, out_w):
 * multiples of 32; images are resized so that their longer side is max(out_h, out_w). */
size_t yolo_augment_workspace_bytes(int b, int out_h, int out_w);   /* the uint8 HWC staging canvas of yolo_augment_images */
/* out_boxes (B, max_out, 5) fp32 yolo, rows past counts[b] zeroed; counts (B) int32: the input of yolo_build_targets_hw.
 * max_out must be >= the sum of nbox over the row's images (extra boxes are not written). sel (B) int32 receives the
 * path each image takes and is read by yolo_augment_images: run this first, on the same stream. */
int yolo_augment_boxes(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, const int32_t* src_dev,
                       const int32_t* hw, int n_pool, const int32_t* src, const double* params, int b, int out_h, int out_w,
                       float* out_boxes, int32_t* counts, int max_out, int32_t* sel, void* stream);
/* pool: uint8 HWC images at byte offsets offsets (device, int64 [n_pool]); staging: yolo_augment_workspace_bytes;
 * out_chw: fp32 (B, 3, out_h, out_w) in [0, 1]. */
int yolo_augment_images(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, const int32_t* src_dev,
                        const int32_t* hw, int n_pool, const int32_t* src, const double* params, const int32_t* sel, int b, int out_h,
                        int out_w, void* staging, float* out_chw, void* stream);

/* ---- augmentation extras: rotation, vertical flip, MixUp, Cutout (csrc/augment.h; nothing of the reference, whose transform list
 * was chosen for ground-level photographs). A second per-row table, float64 [b][YOLO_AUGX_NPARAM], next to the YOLO_AUG_* one; both
 * users of augment.h take it: the *_ex entry points below and yolo_crop_*_ex. Parity with cv2 / albumentations UNPINNED, as for the
 * rest of the augmentation. This comment is the contract; the kernels and tests/augx_ref.py are both written from it. Box arithmetic
 * is fp64 with one rounding per operation (no fused multiply-add), rounded to fp32 at the store; pixel arithmetic is the fixed point
 * of the warp. Out of scope: the `ellipse` rotate method, shear, perspective.
 *
 * chain(r) is row r's output WITHOUT MixUp and Cutout: its own YOLO_AUG_* row, its own mosaic or crop window, and of its own extras
 * the rotation and the vertical flip. A row that takes no transform at all (an image without a label file in yolo_augment_*:
 * "letterbox only") takes no rotation and no vertical flip either; MixUp and Cutout work on outputs and apply to every row.
 *
 * ROTATION (ROT_COS, ROT_SIN: cos and sin of the angle, formed by the caller in fp64; the kernels evaluate neither). Part of
 * ShiftScaleRotate, behind its gate YOLO_AUG_DO_SSR. The matrix is getRotationMatrix2D((W/2, H/2), theta, scale):
 *   alpha = SCALE cos, beta = SCALE sin, cx = 0.5 W, cy = 0.5 H,
 *   m = [alpha, beta, (1 - alpha) cx - beta cy; -beta, alpha, beta cx + (1 - alpha) cy], then m02 += DX W, m12 += DY H.
 * With cos = 1, sin = 0 this is the matrix without the extras bit for bit. Pixels: the fixed-point warpAffine of that matrix,
 * constant border 0 per tap. Boxes (albumentations 1.x bbox_shift_scale_rotate, `largest_box`): the corners (b0, b1), (b2, b1),
 * (b0, b3), (b2, b3) in pixels (x W, y H) map to ((m00 px + m01 py + m02) / W, (m10 px + m11 py + m12) / H), sums taken left to
 * right; the box is their min / max envelope t; ta = (t2 W - t0 W)(t3 H - t1 H); c = t clipped to [0, 1], ca alike; kept iff
 * ca != 0 and ca / ta >= 0.4. A row with exactly cos = 1 and sin = 0 takes the two-corner expressions of the chain without extras.
 *
 * VERTICAL FLIP (DO_VFLIP != 0), after the horizontal flip: output row y reads warped row H - 1 - y; boxes y0, y1 = 1 - y1, 1 - y0.
 *
 * MIXUP. p = MIX_PARTNER if it is an integer value in [0, b_count) other than the row itself, else none (-1, a non-integer, NaN).
 * out[b] = chain(b) l + chain(p) m with l = (float) MIX_LAMBDA, m = 1.0f - l, per channel
 * ((float) pa * (1.0f / 255.0f)) * l + ((float) pb * (1.0f / 255.0f)) * m, every operation rounded once in fp32, no fused
 * multiply-add. Not transitive: the partner contributes chain(p), whatever its own MIX_PARTNER and rectangles say. Boxes: row b's
 * kept boxes in their order, then the partner's kept boxes in their order, each set by its own row's rules; kept rows beyond
 * max_out are not written. A partner without a label file contributes pixels and no boxes.
 *
 * CUTOUT, last, on the mixed output. Rectangle k < CUT_N (0 .. 4; values below 1 or NaN are 0, above 4 are 4) covers the pixels
 * X0 <= x < X1, Y0 <= y < Y1 with X0 = (int)(clip01(x0) W), Y0 = (int)(clip01(y0) H), X1, Y1 alike (clip01(NaN) = 0); these pixels
 * of the three planes become (float) CUT_FILL. Rectangles are in OUTPUT coordinates: no flip moves them. Boxes: with
 * R = (X0 / W, Y0 / H, X1 / W, Y1 / H) in fp64 and inter = max(0, min(b2, R2) - max(b0, R0)) max(0, min(b3, R3) - max(b1, R1)),
 * a box (own or the partner's, after every other step) is dropped iff inter > CUT_COVER ((b2 - b0)(b3 - b1)) for some k: strict,
 * each rectangle alone. An empty rectangle (X1 <= X0 or Y1 <= Y0) erases nothing and drops nothing. */
#define YOLO_AUGX_ROT_COS 0
#define YOLO_AUGX_ROT_SIN 1
#define YOLO_AUGX_DO_VFLIP 2
#define YOLO_AUGX_MIX_PARTNER 3
#define YOLO_AUGX_MIX_LAMBDA 4
#define YOLO_AUGX_CUT_N 5
#define YOLO_AUGX_CUT_COVER 6
#define YOLO_AUGX_CUT_FILL 7
#define YOLO_AUGX_CUT_RECT 8        /* + 4k .. + 4k + 3 = (x0, y0, x1, y1) of rectangle k < 4, normalised to the output canvas */
#define YOLO_AUGX_NPARAM 24
/* yolo_augment_boxes / yolo_augment_images with `extra` (device, [b][YOLO_AUGX_NPARAM]); NULL = exactly the calls above, which
 * forward here. With extra, max_out should hold a row's boxes plus its partner's. Still one launch over the output for the warp,
 * blend and erase, no atomics, nothing read back. */
int yolo_augment_boxes_ex(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, const int32_t* src_dev,
                          const int32_t* hw, int n_pool, const int32_t* src, const double* params, const double* extra, int b,
                          int out_h, int out_w, float* out_boxes, int32_t* counts, int max_out, int32_t* sel, void* stream);
int yolo_augment_images_ex(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, const int32_t* src_dev,
                           const int32_t* hw, int n_pool, const int32_t* src, const double* params, const double* extra,
                           const int32_t* sel, int b, int out_h, int out_w, void* staging, float* out_chw, void* stream);

/* ---- evaluation: average precision per class (utils.py:193-274) ----------------------------- */
/* rows are [image, x, y, w, h, objectness, class] fp32. dets_sorted: class ascending, objectness descending (stable);
 * gts_sorted: class ascending, image ascending (stable); *_class_offsets: [num_classes + 1] row ranges.
 * assigned: n_gt int32 scratch, tp_flags: one fp32 per detection (1 = true positive), ap_per_class: trapezoid area of the
 * precision/recall curve, -1 for classes without ground truth (the reference skips them). */
int yolo_map_match(const float* dets_sorted, const int32_t* det_class_offsets, const float* gts_sorted, const int32_t* gt_class_offsets,
                   int num_classes, int n_gt, float iou_threshold, int center, int32_t* assigned, float* tp_flags, float* ap_per_class,
                   void* stream);

/* The same matching at 1 .. 16 IoU thresholds in one pass (mAP@[.5:.95]), with the counts for precision / recall at a confidence
 * threshold. dets_sorted [n_det] / gts_sorted [n_gt] and the class offsets as for yolo_map_match. iou_thresholds: n_thr floats ON THE
 * HOST, each in [0, 1), any order, repeats allowed; every comparison with them is fp32.
 *
 * Per detection d (a row of dets_sorted): best_iou[d] = the first maximum IoU over the ground truths of its image and class in
 * list order under a strict `>` against a running best that starts at 0 (yolo_map_match's choice, which does not depend on the
 * threshold), best_gt[d] = that row of gts_sorted, or 0 and -1 when there is none. At threshold t, d is a true positive iff
 * best_iou[d] > t and d is the lowest row among the detections d' with best_gt[d'] == best_gt[d] and best_iou[d'] > t: exactly the
 * detections the sequential walk of yolo_map_match marks (the first one that reaches a ground truth with a passing IoU assigns it).
 *
 * Outputs (device): best_iou [n_det] fp32, best_gt [n_det] int32, tp [n_thr][n_det] bytes (1 = true positive), ap [n_thr][nc] fp32 =
 * yolo_map_match's ap_per_class at that threshold, bit for bit (-1 for a class without ground truth, 0 for one with ground truth
 * and no detection), tp_at_conf [n_thr][nc] int32 = the true positives among the detections with objectness > conf_threshold
 * (strict, fp32), n_det_at_conf [nc] int32 = those detections. Integer atomics only, so a call repeats bit for bit. A memset and
 * three launches (one launch for n_det == 0, which is legal, as is n_gt == 0); nothing is copied to the host and the call does not
 * wait. Limits: n_det, n_gt >= 0, num_classes >= 1, 1 <= n_thr <= 16, thresholds in [0, 1), conf_threshold not NaN, center 0 or 1,
 * no null pointer (dets_sorted / best_iou / best_gt / tp may be NULL for n_det == 0, gts_sorted for n_gt == 0): otherwise
 * YOLO_ERR_ARG. A workspace that is NULL, not 4-byte aligned or smaller than yolo_eval_workspace_bytes (0 for shapes outside the
 * limits): YOLO_ERR_WORKSPACE. Both are returned before any launch. */
size_t yolo_eval_workspace_bytes(int n_det, int n_gt, int n_thr);
int yolo_eval_detections(const float* dets_sorted, const int32_t* det_class_offsets, int n_det, const float* gts_sorted,
                         const int32_t* gt_class_offsets, int n_gt, int num_classes, const float* iou_thresholds, int n_thr,
                         float conf_threshold, int center, float* best_iou, int32_t* best_gt, unsigned char* tp, float* ap,
                         int32_t* tp_at_conf, int32_t* n_det_at_conf, void* workspace, size_t workspace_bytes, void* stream);

/* check_model_accuracy (utils.py:334-381) for one scale of one batch: counts5 += [class correct, n_obj, objectness correct
 * on object cells, objectness correct on no-object cells, n_noobj]; pred / target as for yolo_loss_fwd. */
int yolo_accuracy_counts(const float* pred, const int64_t* strides5, const float* target, int b, int g, int nc, float obj_threshold,
                         unsigned long long* counts5, void* stream);
/* rectangular grid (B,3,gh,gw,·); yolo_accuracy_counts is the gh = gw = g case */
int yolo_accuracy_counts_hw(const float* pred, const int64_t* strides5, const float* target, int b, int gh, int gw, int nc,
                            float obj_threshold, unsigned long long* counts5, void* stream);

/* ---- fused per-scale loss (optional replacement of YOLOLoss.forward, loss.py:29-81) -------- */
/* pred (B,3,g,g,5+nc) fp32 through element strides; target (B,3,g,g,6) fp32 contiguous
 * [x_cell,y_cell,w_cells,h_cells,obj in {1,0,-1},class]; anchors (3,2) in grid units.
 * losses4 = [5*box, 1*object, 0.5*noobj, 1*class] (each a mean over the selected cells of this call, as in
 * the reference), counts2 = [n_obj, n_noobj] for the backward. Deterministic (fixed-order fp64 sums), no host
 * dependence (graph-capturable), and — unlike the reference — no in-place mutation of pred / target. */
size_t yolo_loss_workspace_bytes(int b, int g);
int yolo_loss_fwd(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int g, int nc,
                  float* losses4, float* counts2, void* workspace, size_t workspace_bytes, void* stream);
/* dpred (B,3,g,g,5+nc) contiguous = sum_k grad_losses4[k] * d losses4[k] / d pred */
int yolo_loss_bwd(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int g, int nc,
                  const float* counts2, const float* grad_losses4, float* dpred, void* stream);
/* rectangular grid (B,3,gh,gw,·); the three functions above are the gh = gw = g case */
size_t yolo_loss_workspace_bytes_hw(int b, int gh, int gw);
int yolo_loss_fwd_hw(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int gh, int gw,
                     int nc, float* losses4, float* counts2, void* workspace, size_t workspace_bytes, void* stream);
int yolo_loss_bwd_hw(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int gh, int gw,
                     int nc, const float* counts2, const float* grad_losses4, float* dpred, void* stream);
/* The same three launches with other terms (NOT the reference's; csrc/loss_iou.hip). Decoded boxes in cell / grid
 * units: b = (sig(p0), sig(p1), exp(p2) aw, exp(p3) ah), g = t0..3; IoU as above (detached wherever it is a target).
 *   box_kind   MSE: the reference's term. GIOU / DIOU / CIOU: mean over the object cells of 1 - XIoU(b, g), gradient into p0..3
 *              (CIoU's alpha is a constant of the gradient)
 *   obj_kind   MSE: (p4 - IoU)^2. BCE: BCEWithLogits(p4, IoU)
 *   focal_gamma >= 0: no-object cells cost sig(p4)^gamma * softplus(p4); 0 is the reference's BCE
 *   label_smoothing in [0, 1): torch.nn.CrossEntropyLoss(label_smoothing=...)
 *   lambda_*   the weights of losses4 = [box, object, noobj, class] (the reference: 5, 1, 0.5, 1), finite
 * Anything else: YOLO_ERR_ARG before a launch. Workspace, counts2, determinism and graph capture as for yolo_loss_fwd_hw. */
enum { YOLO_LOSS_BOX_MSE = 0, YOLO_LOSS_BOX_GIOU = 1, YOLO_LOSS_BOX_DIOU = 2, YOLO_LOSS_BOX_CIOU = 3 };
enum { YOLO_LOSS_OBJ_MSE = 0, YOLO_LOSS_OBJ_BCE = 1 };
typedef struct yolo_loss_opts {
    int box_kind, obj_kind;
    float focal_gamma, label_smoothing;
    float lambda_box, lambda_obj, lambda_noobj, lambda_class;
} yolo_loss_opts;                                            /* 32 bytes */
int yolo_loss_fwd_opts(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int gh, int gw,
                       int nc, float* losses4, float* counts2, void* workspace, size_t workspace_bytes, const yolo_loss_opts* opts,
                       void* stream);
int yolo_loss_bwd_opts(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int gh, int gw,
                       int nc, const float* counts2, const float* grad_losses4, float* dpred, const yolo_loss_opts* opts, void* stream);

/* ---- optimizer step (code/train.py:171-172 torch.optim.SGD(model.parameters(), lr, momentum, weight_decay); :68 step) ---- */
/* One launch over every parameter tensor; the same bits as torch.optim.SGD's default implementation (each of its passes
 * rounds a + alpha * b once). items (device): n_items x yolo_sgd_item; an item with g == NULL is skipped; n < 0 marks a
 * momentum buffer that does not exist yet (first step: buf = g + wd * p). chunks (device): n_chunks x {item index, first
 * element}, one per yolo_sgd_chunk_elems() elements of every item.
 * yolo_sgd_step: one block per chunk does the whole update in registers (p, g, buf read once; p, buf written once; the gradient
 *   is never written). hyper4_dev: {lr, momentum, dampening, weight_decay} as a 16-byte aligned float[4] in DEVICE memory, read
 *   when the kernel runs: a launch captured in a HIP graph then follows the LR scheduler of train.py:71-74,187-189 (stepped after
 *   every batch) instead of replaying the capture-time values. nesterov needs momentum > 0 and dampening == 0 (the caller's
 *   responsibility: the values are not on the host). Every option is a pointer that may be NULL:
 *   grad_scale_dev (fp16 loss scaling without a host wait, torch.amp.GradScaler, train.py:39,67-69: g * (float)(1.0 /
 *   (double)*grad_scale_dev) first, a rounding of its own; NULL, or a scale of 1: no unscale), found_inf_dev (set: nothing is
 *   touched), written_dev ("first step" as a device fact: written_dev[i] == 0 means item i's momentum buffer was never written,
 *   buf = g + wd * p, and n of an item may then have either sign; a second small launch sets the word to 1 for every item with a
 *   gradient after a step that was applied; needs found_inf_dev; NULL: the sign of n says "first step"), clip_state_dev (g * coef
 *   after the unscale, a rounding of its own, applied also when coef == 1; the state is what yolo_clip_finalize left),
 *   shadows_dev + ema_state_dev (the weight average below of every item with a gradient moved in the same launch, towards the
 *   NEW parameter value; shadows_dev: n_items x float*, the average of each item's parameter, NULL entry: plain update; both or
 *   neither; `updates` is not advanced: the caller finishes the update with yolo_ema_update).
 * yolo_sgd_check_finite: one launch over the same tables; *found_inf_dev (float) becomes 1.0f when any gradient holds an inf
 *   or a NaN (exponent bits all ones). clear != 0: a one-thread launch sets the word to 0.0f first (stream-ordered,
 *   capturable); clear == 0 adds to what an earlier call (another parameter group) found. Nothing else is written. */
typedef struct yolo_sgd_item { float* p; const float* g; float* buf; long long n; } yolo_sgd_item;
int yolo_sgd_chunk_elems(void);
int yolo_sgd_step(const void* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, const float* hyper4_dev,
                  const void* clip_state_dev, const float* grad_scale_dev, const float* found_inf_dev, int32_t* written_dev,
                  const void* shadows_dev, const void* ema_state_dev, int nesterov, int maximize, void* stream);
int yolo_sgd_check_finite(const void* items_dev, const int32_t* chunks_dev, int n_chunks, float* found_inf_dev, int clear, void* stream);
/* Weight average (an exponential moving average of every parameter and BatchNorm statistic), fp32, bit for bit
 * e.mul_(d).add_(p, alpha = 1 - d) of PyTorch on the GPU:
 *   d = warmup ? min(decay, float(1 + updates) / float(10 + updates)) : decay;   e = fma(1 - d, p, e * d)
 * The yolo_ema_state lives in device memory, 16-byte aligned, and is read when a kernel runs, never passed by value: a launch captured in a HIP
 * graph follows the warm-up of the decay through its replays.
 * yolo_sgd_step with shadows_dev + ema_state_dev moves the average of what it updates in its own launch and leaves `updates` alone.
 * yolo_ema_update: one launch over n_chunks chunks of a table of yolo_ema_item rows (chunks as for the step); n > 0: n floats
 * are averaged, n < 0: -n 32-bit words are copied (integer entries). advance != 0: a one-thread launch then adds 1 to
 * `updates`. found_inf_dev (may be NULL) != 0: nothing is written and nothing is counted, like the skipped step. */
typedef struct yolo_ema_state { int32_t updates; float decay; int32_t warmup; int32_t reserved; } yolo_ema_state;
typedef struct yolo_ema_item { const void* src; void* dst; long long n; } yolo_ema_item;
int yolo_ema_update(const void* items_dev, const int32_t* chunks_dev, int n_chunks, void* ema_state_dev, const float* found_inf_dev,
                    int advance, void* stream);
/* Gradient clipping by global norm: torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, error_if_nonfinite=False)
 * between the unscale and the step, over the same tables as the step.
 *   total_norm = the norm of every gradient of every group (items with g != NULL), after the unscale g * (float)(1.0 /
 *                (double)*grad_scale_dev) (a rounding of its own; grad_scale_dev == NULL: none), before maximize / weight decay.
 *                YOLO_NORM_L2: squares summed in fp64 in a fixed order, square root, one rounding to fp32. YOLO_NORM_INF: the
 *                largest |g|, NaN-propagating.
 *   coef       = min(fl(fl(1 / fl(total_norm + 1e-6f)) * max_norm), 1) in fp32, the reciprocal correctly rounded: the bits of
 *                torch.clamp(max_norm / (total_norm + 1e-6), max=1.0).
 * The yolo_clip_state lives in device memory, 16-byte aligned. max_norm is the caller's to write and is read when the
 * finalize kernel runs, never passed by value: a launch captured in a HIP graph follows a changed value. The other three
 * words are written by yolo_clip_finalize.
 * yolo_clip_norm_partials: one block per chunk writes one double to partials_dev[chunk] (n_chunks slots, 8-byte aligned; a
 *   chunk of an item without a gradient writes 0). found_inf_dev != NULL: the same read of the gradients also does the check of
 *   yolo_sgd_check_finite into it (clear as there). No atomics: the same bits every run.
 * yolo_clip_finalize: one block reduces n_partials doubles (every group's, laid out one after the other) in a fixed order and
 *   writes total_norm, coef and norm_type. n_partials == 0: total_norm = 0.
 * yolo_sgd_step / yolo_adam_step with clip_state_dev: the update with g * coef in registers, as described there.
 * yolo_clip_scale_grads: g *= coef in place for every item with a gradient (p and buf of the items are not looked at). */
enum { YOLO_NORM_L2 = 0, YOLO_NORM_INF = 1 };
typedef struct yolo_clip_state { float max_norm; float total_norm; float coef; int32_t norm_type; } yolo_clip_state;
int yolo_clip_norm_partials(const void* items_dev, const int32_t* chunks_dev, int n_chunks, const float* grad_scale_dev, int norm_type,
                            double* partials_dev, float* found_inf_dev, int clear, void* stream);
int yolo_clip_finalize(const double* partials_dev, int n_partials, int norm_type, void* clip_state_dev, void* stream);
int yolo_clip_scale_grads(const void* items_dev, const int32_t* chunks_dev, int n_chunks, const void* clip_state_dev, void* stream);
/* Adam / AdamW (torch.optim.Adam / AdamW as PyTorch runs them by default on the GPU: foreach, not capturable, not fused), the
 * same bits; the rounding of every pass is listed in csrc/optim_adam.hip. Two launches per parameter group over the tables of
 * the SGD step. items (device): n_items x yolo_sgd_item {p, g, exp_avg, n}, FOLLOWED by n_items x float* (exp_avg_sq of each
 * item), so the clip entry points above read the same table; an item with g == NULL is skipped and its step count stays.
 * yolo_adam_prepare: one thread per item, in front of the step. *found_inf_dev (may be NULL) != 0: nothing moves. Otherwise, for
 *   every item with a gradient, steps_dev[i] += 1 (int32, t below) and words_dev[8 i .. 8 i + 7] (float, 16-byte aligned) become
 *   {float(1 - lr*wd), float(1 - beta1), float(beta2), float(1 - beta2), float(eps), float(sqrt(1 - beta2^t)),
 *   float((lr / (1 - beta1^t)) * -1), float(wd)}, every expression in fp64 with the roundings of the Python expression and one
 *   cast at the end. hyper5_dev: the group's {lr, beta1, beta2, eps, weight_decay} as doubles in DEVICE memory, read when the
 *   kernel runs: a launch captured in a HIP graph follows an LR scheduler, and the step count is a device fact that a skipped
 *   step does not move.
 * yolo_adam_step: one block per chunk reads the item's words and does the whole update in registers (p, g, exp_avg, exp_avg_sq
 *   read once; p, exp_avg, exp_avg_sq written once; the gradient is never written). Every option is a pointer that may be NULL:
 *   grad_scale_dev (g * (float)(1.0 / (double)*grad_scale_dev) first, a rounding of its own), found_inf_dev (set: nothing is
 *   touched), clip_state_dev (g * coef after the unscale, a rounding of its own, applied also when coef == 1; the state is what
 *   yolo_clip_finalize left), shadows_dev + ema_state_dev (the weight average of every item with a gradient in the same launch,
 *   as in yolo_sgd_step; both or neither). decoupled != 0: AdamW's p *= 1 - lr*wd; otherwise g += wd * p when wd != 0. */
int yolo_adam_prepare(const void* items_dev, int n_items, const double* hyper5_dev, int32_t* steps_dev, float* words_dev,
                      const float* found_inf_dev, void* stream);
int yolo_adam_step(const void* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, const float* words_dev,
                   const float* grad_scale_dev, const float* found_inf_dev, const void* clip_state_dev, const void* shadows_dev,
                   const void* ema_state_dev, int decoupled, int maximize, void* stream);

/* ---- post-processing ------------------------------------------------------------------- */
/* Replaces cells_to_boxes (utils.py:86-148) for one scale.
 * pred: (B,3,g,g,5+nc) fp32 addressed through element strides s[5] (so the reference's permuted
 * view and this library's contiguous head layout both work). is_pred != 0: pred[...,0:2] <-
 * sigmoid, pred[...,2:4] <- exp * anchors (IN PLACE, like the reference), obj = sigmoid,
 * cls = first argmax. boxes: (B, n_total, 6) fp32 rows [cx,cy,w,h,obj,cls]; this scale writes
 * rows box_offset + a*g*g + row*g + col  (n_total, box_offset let three scales share one
 * buffer in the reference's concatenation order, demo.py:44-51). is_pred == 0: 5+nc must be 6. */
int yolo_decode(void* pred, const int64_t* strides5, const float* anchors_3x2, int b, int g, int nc,
                int is_pred, float* boxes, int n_total, int box_offset, void* stream);
/* The three scales of one forward (is_pred = 1) in one launch: preds3[k] / strides15[5k..5k+4] / anchors3[k] / grids3[k] in the
 * reference's concatenation order (scale 0, 1, 2: demo.py:44-51); boxes (B, n_total, 6) with n_total = sum 3 g_k^2. */
int yolo_decode3(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids3, int b, int nc,
                 float* boxes, int n_total, void* stream);
/* write_back = 0: the same boxes WITHOUT the reference's in-place sigmoid / exp write-back into the prediction tensors
 * (utils.py:106-110) - for callers that never look at the predictions again (demo.py:44-55, utils.py:300-321): the kernel's
 * writes drop to the algorithmic 24 bytes per box. yolo_decode takes the same choice as is_pred = 2. */
int yolo_decode3_ex(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids3, int b, int nc,
                    int write_back, float* boxes, int n_total, void* stream);
/* Rectangular grids (B,3,gh,gw,5+nc): rows box_offset + a*gh*gw + row*gw + col, and per axis cx = (1/gw)(sig + col),
 * cy = (1/gh)(sig + row), w = (1/gw)(e^tw aw), h = (1/gh)(e^th ah) with anchors in grid cells. grids_hw6 = [gh0, gw0, gh1,
 * gw1, gh2, gw2]. The square functions above are the gh = gw case (same bits). */
int yolo_decode_hw(void* pred, const int64_t* strides5, const float* anchors_3x2, int b, int gh, int gw, int nc,
                   int is_pred, float* boxes, int n_total, int box_offset, void* stream);
int yolo_decode3_hw(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids_hw6, int b, int nc,
                    int write_back, float* boxes, int n_total, void* stream);
/* The same launch into a row block of a larger buffer: the three scales fill rows [box_offset, box_offset + sum 3 gh gw) of every
 * image of boxes (B, n_total, 6), nothing else is touched (the views of test-time augmentation share one buffer). box_offset >= 0
 * and the block inside n_total, else YOLO_ERR_ARG. */
int yolo_decode3_hw_at(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids_hw6, int b, int nc,
                       int write_back, float* boxes, int n_total, int box_offset, void* stream);

/* Replaces non_max_suppression (utils.py:150-191) with calc_iou (utils.py:38-84) inlined,
 * batched over images. boxes: (B, n, 6) fp32. keep_idx: (B, n) int32, keep_count: (B) int32:
 * for image b the first keep_count[b] entries are indices into its n input rows, in the
 * reference's output order (objectness descending, ties in input order). Bit-exact contract:
 * same kept set and order as the reference for any fp32 input. center != 0 <=> box_format ==
 * "center"; every other string means (x1,y1,w,h) as is (utils.py:57-67). */
/* Ascending sort of n UNIQUE 64-bit keys, none equal to ~0 (2,048-key chunks in LDS + rank merge, the ordering kernels of yolo_nms):
 * the stable list sorts of calc_mAP (utils.py:206,232) as one sort of (major | minor | original index) keys. n <= 262,144. */
size_t yolo_sort_u64_workspace_bytes(int n);
int yolo_sort_u64(const uint64_t* keys, uint64_t* sorted, int n, void* workspace, size_t workspace_bytes, void* stream);
size_t yolo_nms_workspace_bytes(int b, int n);
int yolo_nms(const float* boxes, int b, int n, double iou_threshold, double obj_threshold, int center,
             int32_t* keep_idx, int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- weighted box fusion (csrc/fuse.hip; nothing of the reference) ------------------------------------------------------- */
/* Merges the candidates of every image into clusters whose box is the score-weighted mean of the members' corners (WBF, Solovyev
 * et al.). This comment is the contract (DESIGN.md 7.20 has it step by step; tests/fuse_ref.py restates it in numpy). All fp32,
 * every operation rounded once (written fl), no fused multiply-add, IEEE division.
 * boxes: (b, n, 6) fp32 rows [x, y, w, h, obj, cls]. A row is a candidate iff (double) obj > obj_threshold (NaN fails); the
 * candidates are walked in the order of the NMS (obj descending, -0 = +0, ties by ascending row): g = a candidate's rank. Corners are
 * the NMS's: center != 0: x1 = x - w / 2, y1 = y - h / 2, else x1 = x, y1 = y; x2 = x1 + w, y2 = y1 + h, a = w h.
 * A cluster holds its founder's class (the float), rank and score, its member count n, S = sum of the members' scores, A[4] = sums
 * of fl(s corner) and its fused corners F[4]. IoU of a candidate against a cluster, the NMS's expression on F:
 * inter = max(min(x2, F.x2) - max(x1, F.x1), 0) max(min(y2, F.y2) - max(y1, F.y1), 0), ak = (F.x2 - F.x1) (F.y2 - F.y1),
 * iou = inter / (((a + ak) - inter) + 1e-6f). Eligible clusters: all if class_agnostic != 0, else those whose class == cls (float
 * equality). The candidate joins the eligible cluster of largest iou among those with iou > (float) iou_threshold, ties to the one
 * created first: n += 1, S = fl(S + s), A_t = fl(A_t + fl(s corner_t)), F_t = fl(A_t / S). Otherwise it founds a cluster: n = 1,
 * S = s, A_t = fl(s corner_t), F_t = corner_t.
 * Score of a cluster: conf_type 0 fl(S / (float) n), conf_type 1 the founder's score; for n_views > 0 multiplied by
 * fl((float) min(n, n_views) / (float) n_views).
 * fused (b, n, 6): rows 0 .. count[b]-1 are the clusters in the order score descending (-0 = +0), ties by founder rank ascending:
 * [x, y, w, h, score, founder's class] with w = fl(F.x2 - F.x1), h = fl(F.y2 - F.y1) and x = F.x1, y = F.y1, or for center != 0
 * x = fl(F.x1 + fl(w / 2)), y = fl(F.y1 + fl(h / 2)); members (b, n) int32: n of that row. Rows from count[b] on are zero in
 * both, so the result is input for yolo_nms, yolo_eval_detections or another fusion with any obj_threshold >= 0. assign (b, n)
 * int32 or NULL: the output row that input row i joined, -1 for a row that is no candidate.
 * Outside the bit contract, but terminating and in bounds: non-finite coordinates, and an obj_threshold < 0.
 * The outputs are fully written by the call; everything is stream-ordered, nothing is read back. n <= 163,456 and b <= 2,047
 * (the class-sorted ordering of yolo_nms), else YOLO_ERR_UNSUPPORTED. A segment (the candidates of one class of one image; of one
 * image if class_agnostic) is walked by one wave with its first yolo_fuse_onchip_clusters clusters in LDS and the others in the
 * workspace, its candidates prefetched yolo_fuse_chunk_candidates at a time. Workspace: 16-byte aligned, its size by
 * yolo_fuse_workspace_bytes (HOST ONLY, no GPU needed; 0 outside the limits); every byte that is read was written by the call. */
int yolo_fuse_onchip_clusters(void);
int yolo_fuse_chunk_candidates(void);
size_t yolo_fuse_workspace_bytes(int b, int n);
int yolo_fuse_boxes(const float* boxes, int b, int n, double iou_threshold, double obj_threshold, int center, int class_agnostic,
                    int n_views, int conf_type, float* fused, int32_t* members, int32_t* count, int32_t* assign, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- Soft-NMS and NMS options (csrc/nms_soft.hip; nothing of the reference) ---------------------------------------------- */
/* Suppression that lowers the score of an overlapped box instead of removing it (Soft-NMS, Bodla et al. 2017), with hard removal,
 * class-agnostic suppression, a cap on detections and a final score threshold on the same walk. This comment is the contract
 * (DESIGN.md 7.24 has it step by step; tests/soft_nms_ref.py restates it in numpy). All fp32, every operation rounded once (written
 * fl), no fused multiply-add, IEEE division; a score is compared with obj_threshold or score_threshold in double, as in yolo_nms;
 * iou_threshold and sigma are used as (float). boxes: (b, n, 6) fp32 rows [x, y, w, h, obj, cls]. Per image:
 * 1. Candidates. A row is a candidate iff (double) obj > obj_threshold (NaN and equality fail). Its corners and area are the NMS's
 *    (as for yolo_fuse_boxes), its class the float cls, its current score s = fl(obj + 0.0f) (-0 becomes +0).
 * 2. Interaction. Two candidates interact iff class_agnostic != 0 or their cls are equal as floats (a NaN class: with nothing).
 * 3. The walk. The live set is the candidates with (double) s > score_threshold. Repeat: stop if it is empty, or if max_det > 0 and
 *    max_det rows have been emitted; else the live row of largest s, ties to the lowest input row, is emitted with the score s and
 *    leaves the live set. (This is "take the candidate of largest score and stop if !((double) s > score_threshold)": scores only
 *    fall, so a row that fails the comparison once never passes it again; it also says what a NaN score does - it leaves.) For every
 *    live row j that interacts with the emitted row i: inter = max(min(x2_i, x2_j) - max(x1_i, x1_j), 0) max(min(y2_i, y2_j) -
 *    max(y1_i, y1_j), 0), iou = inter / (((a_i + a_j) - inter) + 1e-6f), the NMS's expression, then by method
 *      0 (hard)      !(iou < thr): j leaves the live set
 *      1 (linear)    iou > thr: s_j = fl(s_j fl(1.0f - iou))
 *      2 (Gaussian)  s_j = fl(s_j w(fl(fl(iou iou) / sigma))), always
 *    and for methods 1 and 2 j leaves the live set unless (double) s_j > score_threshold still holds.
 * 4. w(t) stands for exp(-t), t >= 0, and is this sequence of fp32 operations and nothing else (not the library's expf):
 *      t is NaN: w = t. kf = rint(fl(t 0x1.715476p+0f)), half to even. kf > 125.0f: w = 0.0f (beyond exp(-87), the underflow point).
 *      r = fl(fl(t - fl(kf 0x1.63p-1f)) - fl(kf -0x1.bd0106p-13f))                  (ln 2 in two parts; the first product is exact)
 *      p = -0x1.a01a02p-13f; then p = fl(fl(p r) + c) for c = 0x1.6c16c2p-10f, -0x1.111112p-7f, 0x1.555556p-5f, -0x1.555556p-3f,
 *      0x1p-1f, -0x1p+0f, 1.0f in turn (the degree-7 Taylor polynomial of exp(-r) by Horner, |r| <= 0.3466: remainder 5e-9)
 *      w = the float whose bits are bits(p) - ((int) kf << 23)                        (p is in [0.70, 1.42]: w is normal)
 *    w(0) == 1.0f exactly, 0 <= w <= 1, and |w - exp(-t)| <= 1e-6 exp(-t) wherever w != 0 (tests/test_soft_nms_host.py, against fp64).
 * 5. Outputs, all fully written by the call. keep_idx (b, n) int32: the emitted rows' input indices in emission order, -1 behind
 *    them; keep_count (b) int32; scores (b, n) fp32: scores[b][j] the emitted score of keep_idx[b][j], 0.0f behind them.
 *    rescore_rows: NULL, or a (b, n, 6) buffer - boxes itself is allowed, any other overlap with boxes is not -: column 4 of every
 *    emitted row receives its emitted score and nothing else is touched.
 * Scores only fall and the walk takes the maximum, so the emission order is "emitted score descending, ties by input row ascending",
 * and rows that do not interact evolve independently: the walk runs per class segment in parallel (one workgroup each; per image
 * if class_agnostic), each segment stops after max_det emissions of its own, and a merge orders the segments' emissions and applies
 * max_det. With method 0, class_agnostic 0, max_det 0 and score_threshold == obj_threshold the result is the keep list of yolo_nms,
 * bit for bit. Outside the bit contract, but terminating and in bounds: non-finite coordinates, and negative scores (they would
 * rise under a decay; a negative obj_threshold itself is accepted as in yolo_nms, and -0 counts as +0).
 * YOLO_ERR_ARG, with a message, before anything is launched and without needing a device: a null boxes, keep_idx, keep_count or
 * scores; b or n negative; method outside 0..2; max_det < 0; iou_threshold not finite or not >= 0; obj_threshold or score_threshold
 * not finite; score_threshold < obj_threshold; for method 2 a sigma that is not finite and > 0 as (float); for n > 0 a workspace
 * that is NULL, not 16-byte aligned or smaller than yolo_soft_nms_workspace_bytes (HOST ONLY, no GPU needed; 0 outside the limits);
 * rescore_rows overlapping boxes without being boxes. n <= 163,456 and b <= 2,047 (the class-sorted ordering of yolo_nms), else
 * YOLO_ERR_UNSUPPORTED. The first yolo_soft_nms_onchip_rows rows of a segment are held in LDS, the others in the workspace.
 * Everything is stream-ordered, nothing is read back and nothing is allocated: the call can be captured in a graph like
 * yolo_track_update (after one call outside a capture on that device, which sizes the kernel's LDS). Every workspace byte that is
 * read was written by the call. */
int yolo_soft_nms_onchip_rows(void);
size_t yolo_soft_nms_workspace_bytes(int b, int n);
int yolo_soft_nms(const float* boxes, int b, int n, double iou_threshold, double obj_threshold, double score_threshold, int center,
                  int method, double sigma, int class_agnostic, int max_det, int32_t* keep_idx, int32_t* keep_count, float* scores,
                  float* rescore_rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---- test-time augmentation (csrc/tta.hip; nothing of the reference) ---------------------------------------------------- */
/* A view of a batch: x_nchw (n, c, h, w) fp32 -> out_nchw (n, c, oh, ow), resized and / or mirrored; not in place.
 * (oh, ow) == (h, w): a mirrored copy, bit-exact. Otherwise bilinear with half-pixel centres and no antialias. Per axis, in double:
 * f = (Y + 0.5) (h / oh) - 0.5, s = floor(f), f -= s; s < 0 -> (s, f) = (0, 0); s >= h - 1 -> (h - 1, 0); rows s and
 * min(s + 1, h - 1), wy = (float) f; columns likewise. fp32, one rounding per operation: top = fl(fl(fl(1 - wx) p00) + fl(wx p01)),
 * bot likewise from the second row, value = fl(fl(fl(1 - wy) top) + fl(wy bot)), stored at
 * (flip_ud ? oh - 1 - Y : Y, flip_lr ? ow - 1 - X : X). */
int yolo_tta_view(const float* x_nchw, int n, int c, int h, int w, float* out_nchw, int oh, int ow, int flip_lr, int flip_ud,
                  void* stream);
/* Boxes of a mirrored view back to the frame: rows [row_offset, row_offset + rows) of every image of a (b, n_total, 6) buffer of
 * centre-format rows get cx <- fl(1 - cx) if flip_lr and cy <- fl(1 - cy) if flip_ud; nothing else is touched. (Decoded boxes
 * are normalised per axis: a resized view needs no unmapping.) */
int yolo_boxes_unflip(float* boxes, int b, int n_total, int row_offset, int rows, int flip_lr, int flip_ud, void* stream);

/* ---- tiled detection of frames larger than the network input (nothing of the reference: its dataset was tiled offline) -- */
/* HOST ONLY, no launch. Overlapping tiles of an h x w image: returns their number and, when origins_yx (HOST, may be NULL)
 * is given, writes [y0, x0] rows in row-major tile order; cap = rows origins_yx has room for. Per axis, with length L, tile t,
 * overlap o and stride s = t - o: L <= t is one tile at 0 (zero-padded at the bottom / right by the gather); otherwise
 * n = ceil((L - t) / s) + 1 tiles at k s for k < n - 1 and the last one at L - t, flush with the edge (no padding).
 * YOLO_ERR_ARG unless 0 <= o < t, all sizes are positive and cap covers the count. Any tile size (the network's multiple of 32
 * is the caller's business). */
int yolo_tile_grid(int h, int w, int tile_h, int tile_w, int overlap_h, int overlap_w, int32_t* origins_yx, int cap);
/* img_hwc: uint8 (h, w, 3); origins_yx (device): n_tiles rows [y0, x0], any values (odd ones too; no alignment is assumed);
 * out: (n_tiles, 3, tile_h, tile_w) fp32 = (float) u8 * (1.0f / 255.0f), the normalisation of yolo_letterbox; 0.0f outside the
 * image. n_tiles <= 65535. */
int yolo_tile_gather(const unsigned char* img_hwc, int h, int w, const int32_t* origins_yx, int n_tiles, int tile_h, int tile_w,
                     float* out, void* stream);
/* Threshold, remap to the frame and compact, in order. boxes: (n_tiles, n_per, 6) decoded rows [cx, cy, w, h, obj, cls]
 * normalised to the tile (what yolo_decode3_hw writes); tiles: int32 [n_tiles][4] = {image, y0, x0, 0}, an image outside
 * [0, n_images) (-1) marks a padding tile that contributes nothing; img_hw: int32 [n_images][2]; cand: (n_images, cap, 6);
 * count: int32 [n_images], the running number of candidates per image: READ and ADVANCED here, so the tiles of a frame may
 * arrive in several calls (zero it before the first). A row is a candidate iff (double) obj > obj_threshold (the test of
 * yolo_nms: NaN and equality are out) and its remapped centre has cx' <= 1 and cy' <= 1 (not in a tile's zero padding).
 * fp32, each operation rounded once: cx' = (cx tile_w + x0) / W, cy' = (cy tile_h + y0) / H, w' = (w tile_w) / W,
 * h' = (h tile_h) / H; obj and cls are copied. The candidates of an image are stored in (call, tile, row) order - the
 * input order yolo_nms breaks score ties by - at cand[image][count before ...]; rows at an index >= cap are not written but
 * counted, so count[image] > cap tells the caller about the overflow. Nothing else in cand is touched. Three launches (block
 * counts, one small in-order scan, writes), no atomics, no waiting between workgroups. n_tiles <= 65535 and
 * n_tiles * n_per < 2^31 per call. */
size_t yolo_tile_collect_workspace_bytes(int n_tiles, int n_per);
int yolo_tile_collect(const float* boxes, int n_tiles, int n_per, const int32_t* tiles, const int32_t* img_hw, int n_images, int tile_h,
                      int tile_w, double obj_threshold, float* cand, int cap, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream);
/* ---- pyramid levels: the same frame tiled again at other scales, and boxes cut by an interior tile edge dropped ---- */
/* HOST ONLY, no launch. The size of the level of an h x w frame at `scale`: level_h = max(1, (int) rint(h * scale)), level_w
 * likewise (round half to even, the rounding of the letterbox's resized size); scale 1.0 gives exactly (h, w). YOLO_ERR_ARG for
 * non-positive sizes, a scale that is not finite, <= 0 or > 8, and a result beyond int. The tiles of a level are
 * yolo_tile_grid(level_h, level_w, ...). */
int yolo_tile_level_hw(int h, int w, double scale, int* level_h, int* level_w);
/* yolo_tile_gather on the (level_h, level_w) level of the frame, which is never materialised: output pixel (ty, tx) of tile t is
 * level pixel (y0 + ty, x0 + tx); inside the level its three channels are the frame resized to the level by the library's one
 * uint8 INTER_LINEAR (OpenCV's fixed point, the arithmetic of yolo_letterbox), then (float) u8 * (1.0f / 255.0f); 0.0f outside the
 * level. With (level_h, level_w) == (h, w) the bytes are yolo_tile_gather's. Every output pixel reads a 2 x 2 neighbourhood of
 * the frame, so a scale below 0.5 skips source pixels exactly as yolo_letterbox does on a whole frame: there is no area filter.
 * Origins, limits and error codes as for yolo_tile_gather. */
int yolo_tile_gather_scaled(const unsigned char* img_hwc, int h, int w, int level_h, int level_w, const int32_t* origins_yx, int n_tiles,
                            int tile_h, int tile_w, float* out, void* stream);
/* yolo_tile_collect for tiles of several levels. tiles: int32 [n_tiles][4] = {image, y0, x0, level}, (y0, x0) in pixels of the
 * level; level_hw: int32 [n_levels][2] = {H, W} of every level (of all images: a level belongs to one image). A tile whose image
 * is outside [0, n_images) or whose level is outside [0, n_levels) contributes nothing. The remap is yolo_tile_collect's with
 * the level's size for the frame's (normalised coordinates do not depend on the scale): cx' = (cx tile_w + x0) / W,
 * cy' = (cy tile_h + y0) / H, w' = (w tile_w) / W, h' = (h tile_h) / H.
 * Seam test (off for edge_margin < 0; NaN is YOLO_ERR_ARG), fp32 with one rounding per operation, in tile pixels:
 * px = cx tile_w, pw = w tile_w, hx = pw 0.5, left = px - hx, right = px + hx, and top / bottom likewise from cy, h, tile_h. A side
 * of the tile is interior when it is not on the level's border: left iff x0 > 0, right iff x0 + tile_w < W, top iff y0 > 0,
 * bottom iff y0 + tile_h < H. The row is cut iff left < edge_margin at an interior left side, or
 * right > (float) tile_w - edge_margin at an interior right side, or the same for top / bottom. Equality is not cut and NaN
 * coordinates are not cut. A row is a candidate iff (double) obj > obj_threshold, cx' <= 1 and cy' <= 1, and it is not cut.
 * Order, the count protocol across calls, overflow, workspace (yolo_tile_collect_workspace_bytes), limits and "three launches, no
 * atomics, no waiting" are yolo_tile_collect's; with edge_margin < 0 and level_hw[level of a tile] = img_hw[its image] so are
 * the bytes. YOLO_ERR_ARG for n_levels <= 0. */
int yolo_tile_collect_ex(const float* boxes, int n_tiles, int n_per, const int32_t* tiles, const int32_t* level_hw, int n_levels,
                         int n_images, int tile_h, int tile_w, double obj_threshold, float edge_margin, float* cand, int cap,
                         int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training on tiles: box-aware crops of full-size images (csrc/crops.hip), the training-side counterpart of the tiled
 * detection above. Nothing of the reference: its dataset was tiled offline, which fixes the tile size, the overlap and the scale
 * once and gives every epoch the same cuts. Here the pool of images stays on the device and every batch is cut from it with fresh
 * windows. Parity with cv2 / albumentations UNPINNED, as for the training augmentation. This comment is the contract; the kernels and
 * tests/crops_ref.py are both written from it. ---------------------------------------------------------------------------------- */
/* Per-crop parameter row, float64 (the kernels hold no randomness). U_PICK, JX, JY are draws in [0, 1); BACKGROUND is a switch (on
 * when != 0); SCALE is the pyramid scale of the crop's level, in (0, 8] (a value outside, NaN too, is taken as 1). */
#define YOLO_CROP_U_PICK 0
#define YOLO_CROP_BACKGROUND 1
#define YOLO_CROP_JX 2
#define YOLO_CROP_JY 3
#define YOLO_CROP_SCALE 4
#define YOLO_CROP_NPARAM 5
/* Tables, all on the DEVICE and read only there (nothing on the host depends on an image's size): the pool layout of the training
 * augmentation - pool uint8 HWC images at byte offsets `offsets` (int64 [n_pool]; any offsets, odd ones too), hw_dev int32
 * [n_pool][2], boxes float64 [n_pool][max_in][5] yolo (x, y, w, h, class), nbox int32 [n_pool] (-1 = no label file) - and per crop
 * src_dev int32 [b] (the pool index), crop_params [b][YOLO_CROP_NPARAM], optionally origins_dev int32 [b][2] = [y0, x0] and
 * aug_params [b][YOLO_AUG_NPARAM] (NULL = no augmentation). Tile (tile_h, tile_w): multiples of 32. 1 <= b <= 65535.
 * A src entry outside [0, n_pool) gives an empty crop (windows row {-1, 0, 0, 1, 1, -1}, count 0, zero pixels); nothing is read for it.
 *
 * WINDOW of crop b, fp64 with every operation rounded once. k = src[b], (h, w) = hw[k].
 * 1. (LH, LW) = the level of (h, w) at SCALE by the arithmetic of yolo_tile_level_hw: max(1, rint(h SCALE)), half to even.
 * 2. The crop is an OBJECT crop iff BACKGROUND == 0 and nbox[k] > 0; then picked = min((int) floor(U_PICK nbox[k]), nbox[k] - 1).
 *    Otherwise (a background crop) picked = -1.
 * 3. Per axis (x shown; y alike with LH, tile_h, JY, cy): if LW <= tile_w, x0 = 0 (one tile at 0, zero-padded at the right / bottom,
 *    as yolo_tile_grid has it). Otherwise an object crop takes x0 = (int) floor(cx LW - JX (tile_w - 1)) with cx the picked row's
 *    centre as given, a background crop x0 = (int) floor(JX (LW - tile_w + 1)); both are then clamped to [0, LW - tile_w] (the clamp
 *    is taken on the double, NaN -> 0). So the window lies inside the level whenever the level is at least a tile, and the picked
 *    box's centre lies in the closed tile [0, 1]^2 whenever it lies in the image.
 * 4. With origins_dev, (y0, x0) is taken as given - any values, as for yolo_tile_gather - and picked = -1.
 * 5. windows[b] = {k, y0, x0, LH, LW, picked} (int32 [b][6]); yolo_crop_images reads it: run yolo_crop_boxes first, same stream.
 *
 * BOXES of crop b: every row i < nbox[k], in order:
 * 1. yolo -> (x_min, y_min, x_max, y_max) = (x - w / 2, y - h / 2, x_min + w, y_min + h), each clipped to [0, 1]; the row is dropped
 *    if its area (b2 w - b0 w)(b3 h - b1 h) on the (h, w) image is 0 (the rules of the training augmentation).
 * 2. To tile coordinates: t0 = (b0 LW - x0) / tile_w, t1 = (b1 LH - y0) / tile_h, and t2, t3 alike.
 * 3. ta = (t2 tile_w - t0 tile_w)(t3 tile_h - t1 tile_h); c = t clipped to [0, 1]; ca the same expression on c.
 * 4. The row is kept iff ca != 0 and ca / ta >= min_visibility (a double in [0, 1]; NaN or a value outside is YOLO_ERR_ARG; the
 *    reference's BboxParams has 0.4). A picked box that is larger than the tile can fall under min_visibility and be dropped: the
 *    crop then simply has fewer boxes, or none.
 * 5. With aug_params the row goes through the box chain of the training augmentation on the (tile_h, tile_w) canvas
 *    (ShiftScaleRotate with its own 0.4 visibility rule, flip); without, it is stored as it is: centre and size in fp64, one
 *    rounding to fp32.
 * out_boxes (b, max_out, 5) fp32 + counts (b): rows past counts[b] are zeroed; kept rows beyond max_out are not written.
 *
 * PIXELS of crop b: pixel (ty, tx) of the uint8 canvas is level pixel (y0 + ty, x0 + tx): the image resized to (LH, LW) by the
 * library's one uint8 INTER_LINEAR (the arithmetic of yolo_letterbox; the identity at scale 1; no area filter, so a scale below 0.5
 * skips source pixels), 0 outside the level. Without aug_params out_chw = (float) u8 * (1.0f / 255.0f): at scale 1 the bits of
 * yolo_tile_gather, at other scales those of yolo_tile_gather_scaled, and staging may be NULL. With aug_params the canvas gets the HSV
 * shift (on the zero padding too, as the reference shifts its padded canvas), is stored to `staging`
 * (yolo_augment_workspace_bytes(b, tile_h, tile_w); its uint8 rounding between the HSV shift and the warp is part of the
 * semantics), and the warp / flip / normalise of yolo_augment_images follows. Every crop is augmented, also one of an image
 * without a label file. out_chw: fp32 (b, 3, tile_h, tile_w). */
int yolo_crop_boxes(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, int n_pool, const int32_t* src_dev,
                    const double* crop_params, const int32_t* origins_dev, const double* aug_params, int b, int tile_h, int tile_w,
                    double min_visibility, float* out_boxes, int32_t* counts, int max_out, int32_t* windows, void* stream);
int yolo_crop_images(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, int n_pool, const int32_t* windows,
                     const double* aug_params, int b, int tile_h, int tile_w, void* staging, float* out_chw, void* stream);
/* The same with the augmentation extras ("augmentation extras" above): extra device [b][YOLO_AUGX_NPARAM], NULL = exactly the two
 * calls above, which forward here; extra without aug_params is YOLO_ERR_ARG. chain(r) is crop r as above plus its rotation and
 * vertical flip. With extra EVERY crop is stored to `staging`, also one without ShiftScaleRotate: another crop may mix it in, and
 * which crops are partners is known on the device only. max_out should hold a crop's boxes plus its partner's (2 max_in). */
int yolo_crop_boxes_ex(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, int n_pool, const int32_t* src_dev,
                       const double* crop_params, const int32_t* origins_dev, const double* aug_params, const double* extra, int b,
                       int tile_h, int tile_w, double min_visibility, float* out_boxes, int32_t* counts, int max_out, int32_t* windows,
                       void* stream);
int yolo_crop_images_ex(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, int n_pool, const int32_t* windows,
                        const double* aug_params, const double* extra, int b, int tile_h, int tile_w, void* staging, float* out_chw,
                        void* stream);

/* ---- anchors of a dataset: IoU k-means++ with restarts, and the fitness of an anchor set (csrc/anchors.hip) ---------------- */
/* wh: n rows (w, h) fp32 on the device, 8-byte aligned, every row with 0 < w, h <= 1 (the caller filters; the Python wrapper does).
 * This comment is the contract: the kernels and the CPU restatement of the tests are both written from it.
 *
 * IoU(b, c) = inter / (bw bh + cw ch - inter), inter = min(bw, cw) min(bh, ch): fp32, every operation rounded once, no fused
 * multiply-add. It is the expression yolo_build_targets_hw ranks the anchors of a box by, so the anchors optimise what the target
 * builder uses.
 *
 * Seeding (k-means++), restart r, u = draws[r] (k doubles in [0, 1)): seed 0 is box min((int)(u[0] n), n - 1). For j = 1 .. k - 1,
 * with best_i = max over the seeds chosen so far of IoU(b_i, seed) (fp32): d_i = (double)(1.0f - best_i), the weights are d_i d_i in
 * fp64, T = sum of the weights, and seed j is the smallest i whose running sum of the weights (in index order) exceeds u[j] T,
 * clamped to n - 1; if T == 0, seed j is min((int)(u[j] n), n - 1). The association of the fp64 sums is the implementation's (fixed,
 * so a call repeats bit for bit); a draw that lands within a few ulp of T of a running-sum boundary may pick either neighbour.
 *
 * Lloyd step: label_i = argmax_j IoU(b_i, c_j), ties to the lowest j; the new c_j is the mean of its boxes' (w, h): sums in fp64,
 * divided by the count, rounded once to fp32; a cluster with no box keeps its centroid. Stop when every new centroid is bit-equal
 * to the old one (converged = 1, iterations = the steps taken, the one that changed nothing included) or after max_iter steps
 * (converged = 0, iterations = max_iter).
 *
 * Fitness: the mean over the boxes of max_j IoU(b_i, c_j) against the final centroids, summed in fp64.
 *
 * Outputs (device): centroids [restarts][k][2] fp32 in seed order (not sorted), fitness [restarts] fp64 (8-byte aligned),
 * iterations / converged [restarts] int32, picks [restarts][k] int32 = the box index of every seed (may be NULL). Nothing outside
 * these extents is written and the inputs are not written.
 * Deterministic: no floating-point atomics; every block writes its partial sums to the workspace and one block per restart adds
 * them in ascending block order. The restarts run side by side, each with a done-flag in the workspace: max_iter steps are always
 * enqueued on `stream`, and a restart that has converged leaves the later ones at once. The call does not wait for the device
 * and copies nothing to the host. Every workspace byte that is read was written by the same call.
 * Limits: 1 <= k <= 16, k <= n, 1 <= restarts <= 64, max_iter >= 1, no null pointer but picks, the alignments above: otherwise
 * YOLO_ERR_ARG. A workspace that is NULL, not 16-byte aligned or smaller than yolo_anchor_kmeans_workspace_bytes (0 for
 * shapes outside the limits; it does not decrease as n grows): YOLO_ERR_WORKSPACE. Both are returned before any launch. */
size_t yolo_anchor_kmeans_workspace_bytes(int n, int k, int restarts);
int yolo_anchor_kmeans(const float* wh, int n, int k, int restarts, const double* draws, int max_iter, float* centroids, double* fitness,
                       int32_t* iterations, int32_t* converged, int32_t* picks, void* workspace, size_t workspace_bytes, void* stream);
/* Any k anchors (k x 2 fp32, device) against the boxes, by the same IoU and the same first-maximum label:
 * mean_iou_and_recall[0] = the fitness above, [1] = the share of boxes whose best IoU is > iou_threshold (fp32 comparison);
 * counts [k] int32 = boxes won by every anchor; labels [n] int32 (may be NULL). Two launches, same rules: fixed-order fp64 sums, no
 * waiting, workspace fully written before it is read. n >= 1, 1 <= k <= 16, a threshold that is not NaN, no null pointer but
 * labels, wh and the result 8-byte aligned, else YOLO_ERR_ARG; workspace as above (8-byte aligned). */
size_t yolo_anchor_fitness_workspace_bytes(int n, int k);
int yolo_anchor_fitness(const float* wh, int n, const float* anchors, int k, float iou_threshold, double* mean_iou_and_recall,
                        int32_t* counts, int32_t* labels, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-object tracking (csrc/track.hip; nothing of the reference) ---------------------------------------------------- */
/* A ByteTrack-style tracker (Zhang et al.) for b independent streams: one call per frame carries every stream's tracks one frame on.
 * This comment is the contract (DESIGN.md 7.23 has it step by step; tests/track_ref.py restates it in numpy). All fp32, every
 * operation rounded once (written fl), no fused multiply-add, IEEE division. Comparisons of obj with a threshold are in double.
 *
 * State: one device buffer of yolo_track_state_bytes = b (4 + 26 max_tracks) 4 bytes (4-byte aligned) that the caller owns and only
 * these calls write. Per stream 4 + 26 max_tracks 32-bit words: [frame, next_id, overflow, 0] (int32), then per slot 26 words:
 *   0 state (int32: 0 Free, 1 Tentative, 2 Tracked, 3 Lost)   1 id (int32)   2 cls (float)   3 score (float)   4 lost_frames (int32)
 *   5..12 mean = cx, cy, w, h, then their velocities   13..24 cov = (P00, P01, P11) of cx, of cy, of w, of h   25 zero
 * yolo_track_reset zeroes the streams whose stream_mask byte is not 0 (NULL: all) and sets their next_id to 1. Every word of a Free
 * slot is zero.
 *
 * Detections of stream s, from boxes (b, n, 6) fp32 rows [x, y, w, h, obj, cls]: with keep_idx (b, n) and keep_count (b) (the output
 * of yolo_nms) the rows boxes[s][keep_idx[s][j]], j < keep_count[s], detection index j (an index outside [0, n) is no detection);
 * with keep_count alone (the output of yolo_fuse_boxes) the first keep_count[s] rows; with neither every row. keep_count is clamped
 * to [0, n]; keep_idx without keep_count is YOLO_ERR_ARG. A detection is HIGH iff (double) obj > high_threshold, LOW iff
 * low_threshold < (double) obj <= high_threshold (NaN fails both). Its measurement is z = (cx, cy, w, h): center != 0: cx = x,
 * cy = y; else cx = fl(x + fl(w / 2)), cy = fl(y + fl(h / 2)). Its corners and area are the NMS's (as for yolo_fuse_boxes).
 *
 * A slot's filter is four independent constant-velocity filters, one per coordinate c of (cx, cy, w, h), with mean (p, v) and
 * covariance (P00, P01, P11): the block structure of the usual 8-state filter with diagonal noise. wp = 0.05f, wv = 0.00625f;
 * s_c = the slot's w for cx and w, its h for cy and h, read before the step changes them.
 * Predict: a Lost slot first sets the velocities of w and h to 0. q_p = fl(fl(wp s_c) fl(wp s_c)), q_v likewise with wv;
 *   p = fl(p + v); P00 = fl(fl(fl(P00 + fl(2 P01)) + P11) + q_p); P01 = fl(P01 + P11); P11 = fl(P11 + q_v) (old P01, P11 on the right).
 * Update with z_c (s_c from the predicted mean): r = fl(fl(wp s_c) fl(wp s_c)); S = fl(P00 + r); K0 = fl(P00 / S); K1 = fl(P01 / S);
 *   y = fl(z_c - p); p = fl(p + fl(K0 y)); v = fl(v + fl(K1 y)); from the old P00, P01: P00' = fl(P00 - fl(K0 P00)),
 *   P01' = fl(P01 - fl(K0 P01)), P11' = fl(P11 - fl(K1 P01)).
 * Found from z (s_c from z): p = z_c, v = 0, P00 = fl(t t) with t = fl(fl(2 wp) s_c), P01 = 0, P11 = fl(u u) with u = fl(fl(10 wv) s_c).
 *
 * IoU of a slot's predicted box against a detection, the NMS's expression: the slot's x1 = fl(cx - fl(w / 2)), y1 likewise,
 * x2 = fl(x1 + w), y2 = fl(y1 + h), ak = fl(w h); inter = max(min(x2, X2) - max(x1, X1), 0) max(min(y2, Y2) - max(y1, Y1), 0),
 * iou = inter / (((a + ak) - inter) + 1e-6f). A pair is eligible at threshold m iff iou > (float) m and (class_agnostic != 0 or the
 * slot's cls == the detection's cls, float equality). The matching of a slot set against a detection set is the greedy one: walk
 * the eligible pairs in the order (iou descending, slot index ascending, detection index ascending) and take a pair iff neither
 * side is taken yet.
 *
 * One call, per stream: 1. predict every slot that is not Free. 2. Match the Tracked and Lost slots against the HIGH detections at
 * match_iou[0]. 3. Match the Tracked (not Lost) slots still unmatched against the LOW detections at match_iou[1]. 4. Match the
 * Tentative slots against the HIGH detections still unmatched at match_iou[2]; an unmatched Tentative slot becomes Free. 5. An
 * unmatched Tracked or Lost slot becomes Lost with lost_frames += 1, and Free if then lost_frames > max_age. 6. Every matched slot is
 * updated with its detection and becomes Tracked, score = the detection's obj, lost_frames = 0. 7. Every HIGH detection still
 * unmatched with (double) obj > new_threshold founds a track, in ascending detection index, in the lowest Free slot (those freed in
 * 4 and 5 included): id = next_id++ (ids start at 1 per stream), cls and score the detection's, Tracked if frame == 0 else
 * Tentative; without a Free slot the detection is dropped and overflow += 1. 8. frame += 1.
 *
 * Outputs, fully written by the call: out_boxes (b, max_tracks, 6), out_ids (b, max_tracks), out_count (b): the slots that are
 * Tracked and were matched or founded in this call, in ascending id, as rows [x, y, w, h, score, cls] from the updated mean
 * (center != 0: x = cx, y = cy; else x = fl(cx - fl(w / 2)), y = fl(cy - fl(h / 2))); zero behind out_count. det_ids (b, n), per
 * input row: the id of the track it updated or founded, negated if that track is Tentative after the call; 0 for none and for a
 * row that is no detection.
 *
 * Limits: 1 <= max_tracks <= 512, 1 <= b <= 2047, 0 <= n <= 163,456, else YOLO_ERR_UNSUPPORTED and nothing is launched. A null
 * pointer (boxes may be NULL for n == 0; keep_idx, keep_count as above), a NaN threshold, a match_iou outside [0, 1] or max_age < 0:
 * YOLO_ERR_ARG. Workspace: 4-byte aligned, yolo_track_workspace_bytes = 8 b n bytes (two int32 per detection index; 0, and then
 * it may be NULL, for n == 0; 0 outside the limits), else YOLO_ERR_WORKSPACE; every byte that is read was written by the call.
 * Both size functions are HOST ONLY. One workgroup per stream; one launch; stream-ordered, nothing is read back, so the call can
 * be captured in a graph. Outside the bit contract, but terminating and in bounds: non-finite coordinates, an index that occurs
 * twice in keep_idx. */
typedef struct {
    double high_threshold, low_threshold, new_threshold;
    double match_iou[3];     /* steps 2, 3, 4 */
    int32_t max_age;
    int32_t center;          /* box format of boxes and out_boxes: != 0 centre, 0 corner */
    int32_t class_agnostic;
    int32_t reserved;        /* 0 */
} yolo_track_params;         /* 64 bytes */
size_t yolo_track_state_bytes(int b, int max_tracks);
size_t yolo_track_workspace_bytes(int b, int n, int max_tracks);
int yolo_track_reset(void* state, int b, int max_tracks, const uint8_t* stream_mask_dev, void* stream);
int yolo_track_update(void* state, int b, int max_tracks, const float* boxes, int n, const int32_t* keep_idx, const int32_t* keep_count,
                      const yolo_track_params* p, float* out_boxes, int32_t* out_ids, int32_t* out_count, int32_t* det_ids,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- Drawing detections and tracks onto frames (csrc/draw.hip) ----------------------------------------------------
 * yolo_draw_boxes paints the selected rows of boxes (b, n, 6) fp32 [x, y, w, h, score, cls] onto b frames of h x w pixels: contiguous
 * uint8 HWC, 3 bytes per pixel (r, g, b). frames_out == frames_in draws in place; otherwise frames_out receives the drawn copy and
 * the two buffers must not overlap. Every pixel is read once and written at most once, there are no atomics, and the result is
 * defined to the bit below; pixels outside every command's rectangles keep their input bytes. All arithmetic on coordinates is
 * fp32 with every operation rounded once (written fl), no fused multiply-add, IEEE division.
 *
 * Selection, as for yolo_track_update: with keep_idx (b, n) and keep_count (b) command j < keep_count[s] of frame s is the row
 * boxes[s][keep_idx[s][j]] (an index outside [0, n) draws nothing); with keep_count alone the first keep_count[s] rows; with neither
 * every row. keep_count is clamped to [0, n]; keep_idx without keep_count is YOLO_ERR_ARG. ids (b, n) int32, optional, is indexed by
 * the row, like boxes (the ids of a track result, or det_ids beside the detections).
 *
 * Un-mapping (meta != NULL): meta is a device (b, 6) int32 table of the letterbox's (orig_h, orig_w, new_h, new_w, pad_top, pad_left)
 * and canvas_hw the HOST pair (canvas_h, canvas_w). Before anything else, x = fl(fl(fl(x canvas_w) - pad_left) / new_w),
 * y = fl(fl(fl(y canvas_h) - pad_top) / new_h); a centre-format row then takes w = fl(fl(w canvas_w) / new_w), h = fl(fl(h canvas_h) / new_h),
 * a corner-format row maps its second corner like its first. This is unletterbox_boxes(..., meta=) of the Python layer.
 *
 * Geometry on the h x w frame (W = (float) w, H = (float) h). center != 0: l = fl(fl(x - fl(w / 2)) W), r = fl(fl(x + fl(w / 2)) W),
 * t = fl(fl(y - fl(h / 2)) H), b = fl(fl(y + fl(h / 2)) H). center == 0, rows [x0, y0, x1, y1, ..]: l = fl(x0 W), t = fl(y0 H),
 * r = fl(x1 W), b = fl(y1 H). A row of which one of l, t, r, b is not finite, or with r < l or b < t, draws nothing. Each edge e is
 * clamped to [-2^20, 2^20] and becomes the integer (int) floorf(fl(e + 0.5f)): the box is [x0, x1) x [y0, y1), x1 and y1 exclusive.
 * Outline of thickness T, centred on the edge: the outer rectangle is the box grown by T / 2 on every side, the inner rectangle the
 * box shrunk by T - T / 2 (integer divisions); the ring is outer minus inner, so an empty inner rectangle makes it solid. A row
 * whose outer rectangle is empty or does not meet the frame draws nothing, not even a label. Everything is clipped to the frame.
 *
 * Colour: palette (n_colors, 3) uint8; index (k mod n_colors), the non-negative remainder, with k = the row's id if color_by_id
 * (then ids must be given) else its class c: c = (int) cls (truncation) if |cls| <= 2^30, else -1 (NaN included).
 * Blend of a pixel with the colour at alpha a in 0 .. 255, per channel in integers: out = (src (255 - a) + colour a + 127) / 255,
 * so a = 255 gives colour and a = 0 gives src. The inner rectangle is blended at fill_alpha, the ring at line_alpha.
 *
 * Label (labels != 0). The text is: the class name, row c of class_names (n_classes, name_width) uint8, zero-padded, a byte outside
 * 0x20 .. 0x7E shown as '?' (without class_names: no name); then, if ids is given and the id > 0 (the tracker's tentative and "none"
 * are <= 0), " #" and the id in decimal; then, if scores != 0, " NN%" with pct = (int) floorf(fl(fl(score 100) + 0.5f)) clamped to
 * [0, 100] (NaN: 0), two digits, three for 100. The separating blank is left out at the start of the text. Text beyond
 * yolo_draw_text_capacity() = 32 characters is cut off; an empty text has no plate. With class_names a row whose class is outside
 * [0, n_classes) draws nothing. Font: yolo_draw_font, 95 glyphs of 0x20 .. 0x7E, 5 x 7 in a 6 x 8 cell, 8 bytes per glyph, one per
 * row from the top, bit 4 the left column; row 7 and column 5 are blank. Each font pixel is font_scale x font_scale frame pixels.
 * The plate is 6 font_scale len wide and 8 font_scale high. It stands on the outer rectangle's top-left corner: left = outer x0,
 * top = outer y0 - height; a top < 0 becomes outer y0 (the plate moves inside the box); a right edge > w makes left = max(0, w -
 * width). Plate pixels take the colour (alpha 255), glyph pixels white (255, 255, 255).
 *
 * Order: commands j = 0, 1, .. in selection order, a later one over an earlier one; inside a command fill, outline, plate, glyphs.
 *
 * typedef YoloDrawParams: thickness in [1, 64], font_scale in [1, 8], line_alpha and fill_alpha in [0, 255], else YOLO_ERR_ARG, as
 * are a null frames_in, frames_out, params, palette or (n > 0) boxes, n_colors < 1, class_names with n_classes < 1 or name_width
 * < 1, color_by_id without ids and meta without canvas_hw. Limits: 1 <= h, w <= 16384, 1 <= b <= 65535 (the grid's z), 0 <= n <=
 * 2^24, and a workspace that is not NULL, 16-byte aligned and at least yolo_draw_workspace_bytes(b, n) = round16(4 b) + 112 b n bytes
 * (0 outside the limits), else YOLO_ERR_UNSUPPORTED; all are returned before any launch. Every workspace byte that is read was
 * written by the call. Two launches: one thread per (frame, command) writes a 96-byte record and a 16-byte bounding rectangle; one
 * workgroup per pixel tile (yolo_draw_tile: 128 x 32) tests the frame's commands yolo_draw_chunk() = 256 at a time, keeps the hits
 * in order and composites its pixels in registers. A thread moves a run of 4 pixels as three dwords when both frame pointers and
 * 3 w are multiples of 4, else byte by byte; the bytes are the same. In place, a tile that no command touches is neither read nor
 * written. Stream-ordered, nothing is read back: the call can be captured in a graph. yolo_draw_tile, yolo_draw_chunk,
 * yolo_draw_text_capacity, yolo_draw_font and yolo_draw_workspace_bytes are HOST ONLY. */
typedef struct YoloDrawParams {
    int32_t thickness;       /* T, pixels */
    int32_t font_scale;
    int32_t line_alpha;      /* 0 .. 255, of the ring */
    int32_t fill_alpha;      /* 0 .. 255, of the inner rectangle */
    int32_t labels;          /* != 0: plates with text */
    int32_t scores;          /* != 0: the text ends in the score */
    int32_t color_by_id;     /* != 0: palette index from ids, else from the class */
    int32_t reserved;        /* 0 */
} YoloDrawParams;            /* 32 bytes */
void yolo_draw_tile(int* w, int* h);
int yolo_draw_chunk(void);
int yolo_draw_text_capacity(void);
void yolo_draw_font(unsigned char* rows_95x8);
size_t yolo_draw_workspace_bytes(int b, int n);
int yolo_draw_boxes(const uint8_t* frames_in, uint8_t* frames_out, int b, int h, int w, const float* boxes, int n, int center,
                    const int32_t* keep_idx, const int32_t* keep_count, const int32_t* ids, const int32_t* meta, const int32_t* canvas_hw,
                    const YoloDrawParams* params, const uint8_t* class_names, int n_classes, int name_width, const uint8_t* palette,
                    int n_colors, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The frame front end: RGB24 / BGR24 / NV12 frames to the network's input, batched (csrc/frames.hip) ----------
 * PARITY UNPINNED, for the resize as for yolo_letterbox and for the NV12 conversion too: both follow OpenCV's published integer
 * arithmetic (BT.601 limited range with OpenCV's own literals, so that a cv2.cvtColor user is meant to see the same bits), neither
 * was run against cv2; they are tested against a numpy restatement (tests/frames_ref.py).
 *
 * Frames lie in a uint8 device pool; a device table has one yolo_frame_row per frame: the byte offset of the frame's first row from
 * pool (any int64, so frames that were allocated apart can be addressed from the lowest of them), its size h x w in pixels and its
 * row pitch in bytes. RGB24 / BGR24: h rows of w packed pixels, pitch >= 3 w. NV12: h rows of w luma bytes, then at offset + h pitch
 * the h / 2 rows of interleaved (U, V) pairs with the same pitch, pitch >= w, h and w even. The table is 8-byte aligned.
 *
 * yolo_frames_letterbox: out (n, 3, canvas_h, canvas_w) fp32, planes in R, G, B order whatever the source order, is "convert frame i
 * to packed RGB uint8 at its own resolution, then yolo_letterbox_hw it onto the canvas", to the bit: the resized size (new_h, new_w)
 * and the padding (canvas - new) / 2 per axis are computed in the kernel from (h, w, size, canvas), each output pixel blends four
 * source pixels, each converted to uint8 RGB first, with the fixed-point coefficients of yolo_letterbox, and is scaled by
 * (float) u8 * (1.0f / 255.0f); 0.0f in the padding. meta_out (n, 6) int32, device, optional: (orig_h, orig_w, new_h, new_w,
 * pad_top, pad_left) per frame, the table yolo_draw_boxes and yolo_boxes_to_frames take. One launch for the batch, its grid
 * depends on (n, canvas_h, canvas_w) only; nothing is read back, so the call can be captured in a graph. THE CALLER GUARANTEES what
 * the device cannot report without a wait: every row has h, w >= 1 (NV12: even), a pitch of at least the row's bytes, and a resized
 * size that fits the canvas (yolo_letterbox_canvas gives such a canvas). YOLO_ERR_ARG: a null pool, table or out, n < 1, an unknown
 * format or csc, size or a canvas side <= 0, and n ceil(canvas_h / 16) ceil(canvas_w / 64) > INT_MAX (the frame index is folded into
 * the grid's x, which is the only limit on n). yolo_frames_tile: the 64 x 16 output tile of one workgroup (HOST ONLY).
 *
 * NV12 -> RGB: chroma is replicated over its 2 x 2 luma block; with u = U - 128, v = V - 128, y = max(0, Y - yoff) CY, in int32,
 *   R = clip((y + (1 << 19) + CVR v) >> 20), G = clip((y + (1 << 19) + CVG v + CUG u) >> 20), B = clip((y + (1 << 19) + CUB u) >> 20),
 * arithmetic shifts, clip to 0 .. 255. csc picks (CY, CVR, CVG, CUG, CUB, yoff), which yolo_frames_csc_constants returns (HOST ONLY):
 *   YOLO_CSC_BT601       1220542, 1673527, -852492, -409993, 2116026, 16   (OpenCV's ITUR_BT_601_* literals)
 *   YOLO_CSC_BT601_FULL  1048576, 1470104, -748826, -360853, 1858077,  0
 *   YOLO_CSC_BT709       1220945, 1879825, -558796, -223607, 2215014, 16
 *   YOLO_CSC_BT709_FULL  1048576, 1651297, -490864, -196424, 1945738,  0
 * the last three round(c 2^20) of the exact coefficients from the standard's Kr, Kb. csc is ignored for RGB24 / BGR24.
 *
 * yolo_frames_to_rgb: the conversion alone, out (n, h, w, 3) packed RGB uint8 at source resolution; all n frames are h x w (the
 * arguments; of the table the call reads offset and pitch), 1 <= h, w <= 16384, NV12 even, else YOLO_ERR_ARG.
 *
 * yolo_boxes_to_frames: boxes (b, n, 6) fp32 rows [x, y, w, h, score, cls] normalised to the canvas -> out, normalised to each
 * frame, with meta (b, 6) as above: x = ((double) x canvas_w - pad_left) / new_w, y = ((double) y canvas_h - pad_top) / new_h,
 * w = ((double) w canvas_w) / new_w, h = ((double) h canvas_h) / new_h, every operation in fp64 in that order and one rounding to
 * fp32; columns 4 and 5 are copied. This is unletterbox_boxes(..., meta=) of the Python layer rounded to fp32 (yolo_draw_boxes maps
 * in fp32 steps instead). out may be boxes. n == 0 launches nothing. Stream-ordered, no read-back. */
#define YOLO_FRAMES_RGB24 0
#define YOLO_FRAMES_BGR24 1
#define YOLO_FRAMES_NV12 2
#define YOLO_CSC_BT601 0
#define YOLO_CSC_BT601_FULL 1
#define YOLO_CSC_BT709 2
#define YOLO_CSC_BT709_FULL 3
typedef struct yolo_frame_row {
    int64_t offset;          /* bytes from pool to the frame's first row */
    int32_t h, w;            /* pixels */
    int32_t pitch;           /* bytes per row */
    int32_t reserved;        /* 0 */
} yolo_frame_row;            /* 24 bytes */
void yolo_frames_tile(int* w, int* h);
int yolo_frames_csc_constants(int csc, int32_t* out6);
int yolo_frames_letterbox(const uint8_t* pool, const yolo_frame_row* table, int n, int format, int csc, int size, int canvas_h,
                          int canvas_w, float* out, int32_t* meta_out, void* stream);
int yolo_frames_to_rgb(const uint8_t* pool, const yolo_frame_row* table, int n, int h, int w, int format, int csc, uint8_t* out,
                       void* stream);
int yolo_boxes_to_frames(const float* boxes, int b, int n, const int32_t* meta, int canvas_h, int canvas_w, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLO_MI355X_H */
