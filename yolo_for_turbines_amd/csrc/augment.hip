// augment.hip — the training transform chain of the reference on the device: config.set_train_transforms (config.py:60-87)
// = LongestMaxSize -> centred PadIfNeeded(0) -> HueSaturationValue(2, 50, 40) -> ShiftScaleRotate(scale (1, 1.5), shift
// 0.0625, rotate 0, constant border 0) -> HorizontalFlip -> Normalize(0, 1, 255), with BboxParams(yolo, min_visibility 0.4,
// clip), and mosaic_augmentation (utils.py:503-662) in front of it when the caller asks for mosaic (dataset.py:75-111).
//
// The kernels hold no randomness: every draw comes from a per-image parameter row (YOLO_AUG_* in the header), so each
// transform can be switched on alone. Three launches per batch, in this order on one stream:
//   aug_boxes          one thread per image (sequential, like build_targets_kernel): letterbox / mosaic box mapping, mosaic
//                      cutout choice, the affine, clip + visibility filter, flip; compacts the kept boxes into (B, M, 5) +
//                      counts (B) — the input of yolo_build_targets_hw — and writes sel[b], the path image b takes;
//   aug_canvas_u8      one thread per output pixel: letterbox or mosaic sample (the INTER_LINEAR fixed-point resize of
//                      resample.h), HSV shift, stored as a uint8 HWC staging canvas (the reference rounds to uint8 between
//                      the HSV and the warp, so the staging buffer is part of the semantics);
//   aug_warp_normalize one thread per output pixel: fixed-point warpAffine sample of the staging canvas (or a copy), flip,
//                      x (1/255), fp32 CHW.
//
// PARITY UNPINNED, like preprocess.hip: cv2 / albumentations are not installed where this was built. The kernels follow
// OpenCV's published uint8 algorithms (RGB2HSV_b / HSV2RGB_b, warpAffine with AB_BITS 10, INTER_BITS 5 and the 15-bit
// bilinear table) and albumentations 1.x's box rules; they are tested bit for bit against tests/augment_ref.py, a numpy
// restatement of the same rules. Box arithmetic is double, rounded to fp32 at the store (the convention of targets.hip).
#include "common.h"
#include "resample.h"
#include "augment.h"          // the box rules, the HSV shift and the warp of one pixel, shared with crops.hip

namespace yolo {

enum { SEL_LETTERBOX = -2, SEL_STANDARD = -1 };   // sel[b] >= 0: mosaic, index of the cutout draw that won

// ---------------------------------------------------------------------------------------------------- boxes
// box i of quadrant q in the padded 2S x 2S mosaic (utils.py:546-592), yolo; false when albumentations drops it
__device__ bool mosaic_box(const double* in, int q, int h, int w, int S, double o[4]) {
    double b[4];
    yolo_to_albu(in[0], in[1], in[2], in[3], b);                           // resize_aug: LongestMaxSize, boxes unchanged
    if (!area_nz(b, h, w)) return false;
    double cx = (b[0] + b[2]) / 2.0, cy = (b[1] + b[3]) / 2.0, bw = b[2] - b[0], bh = b[3] - b[1];
    cx /= 2; cy /= 2; bw /= 2; bh /= 2;                                      // relative to the 2h x 2w tile
    if (q & 1) cx += 0.5;
    if (q & 2) cy += 0.5;
    yolo_to_albu(cx, cy, bw, bh, b);                                         // pad_aug: PadIfNeeded(2S, 2S, 255)
    if (!area_nz(b, 2 * h, 2 * w)) return false;
    const int top = (2 * S - 2 * h) / 2, left = (2 * S - 2 * w) / 2;
    b[0] = (b[0] * (2 * w) + left) / (2 * S);
    b[2] = (b[2] * (2 * w) + left) / (2 * S);
    b[1] = (b[1] * (2 * h) + top) / (2 * S);
    b[3] = (b[3] * (2 * h) + top) / (2 * S);
    if (!area_nz(b, 2 * S, 2 * S)) return false;
    o[0] = (b[0] + b[2]) / 2.0; o[1] = (b[1] + b[3]) / 2.0; o[2] = b[2] - b[0]; o[3] = b[3] - b[1];
    return true;
}

// the cutout test of utils.py:603-621 at draw a: the cx -> x1 conversion applied a + 1 times (the reference re-applies it on
// every attempt), then the intersection with [x, x + 0.5] x [y, y + 0.5]
__device__ __forceinline__ bool cutout_hit(const double o[4], int a, double x, double y, double* bx, double* by) {
    double u = o[0], v = o[1];
    for (int r = 0; r <= a; ++r) { u = u - o[2] / 2; v = v - o[3] / 2; }
    *bx = u; *by = v;
    const double xa = fmax(u, x), ya = fmax(v, y), xb = fmin(u + o[2], x + 0.5), yb = fmin(v + o[3], y + 0.5);
    return fmax(0.0, xb - xa) * fmax(0.0, yb - ya) > 0.0;
}

// The kept boxes of output row s4 = src[r] under its parameter row p, appended to ob at *np (at most max_out rows); returns the path
// the row takes. EX: the chain runs with the row's extras e and the rectangles of ec, the extras of the row being written.
template <bool EX>
__device__ __forceinline__ int row_boxes(const double* __restrict__ boxes, const int* __restrict__ nbox, int max_in,
                                         const int* __restrict__ hw, const int* s4, const double* p, const double* e, const double* ec,
                                         int H, int W, float* ob, int* np, int max_out) {
    int n = *np;
    int path = SEL_STANDARD;
    if (nbox[s4[0]] < 0) {
        path = SEL_LETTERBOX;                                                // no label file: letterbox only (dataset.py:162-165)
    } else if (s4[1] >= 0) {
        const int S = W;
        int h, w;
        resized_hw(hw[2 * s4[0]], hw[2 * s4[0] + 1], S, &h, &w);
        bool any = false;
        for (int a = 0; a < 10 && path == SEL_STANDARD; ++a) {
            const double x = p[YOLO_AUG_MOSAIC + 2 * a], y = p[YOLO_AUG_MOSAIC + 2 * a + 1];
            for (int q = 0; q < 4 && path == SEL_STANDARD; ++q) {
                const int nq = nbox[s4[q]];
                for (int i = 0; i < nq; ++i) {
                    double o[4], bx, by;
                    if (!mosaic_box(boxes + ((size_t)s4[q] * max_in + i) * 5, q, h, w, S, o)) continue;
                    any = true;
                    if (cutout_hit(o, a, x, y, &bx, &by)) { path = a; break; }
                }
            }
            if (!any) break;                                                 // no box at all: the reference cannot run
        }
        if (path >= 0) {
            const int a = path;
            const double x = p[YOLO_AUG_MOSAIC + 2 * a], y = p[YOLO_AUG_MOSAIC + 2 * a + 1];
            for (int q = 0; q < 4; ++q) {
                const int nq = nbox[s4[q]];
                for (int i = 0; i < nq; ++i) {
                    const double* in = boxes + ((size_t)s4[q] * max_in + i) * 5;
                    double o[4], bx, by;
                    if (!mosaic_box(in, q, h, w, S, o) || !cutout_hit(o, a, x, y, &bx, &by)) continue;
                    double bw = o[2], bh = o[3];                             // utils.py:632-659
                    if (bx < x) { bw -= x - bx; bx = x; }
                    if (by < y) { bh -= y - by; by = y; }
                    if (bx >= x) bx -= x;
                    if (by >= y) by -= y;
                    if (bw + bx > x + 0.5) bw = (x + 0.5) - bx;
                    if (bh + by > y + 0.5) bh = (y + 0.5) - by;
                    bx *= 2; by *= 2; bw *= 2; bh *= 2;
                    double bb[4];
                    yolo_to_albu(bx + bw / 2, by + bh / 2, bw, bh, bb);      // set_train_transforms(mosaic=True) on S x S
                    if (!area_nz(bb, S, S)) continue;
                    if (n < max_out && finish_box_x<EX>(bb, in[4], p, e, ec, S, S, ob + 5 * n)) ++n;
                }
            }
        }
    }
    if (path == SEL_STANDARD) {                                              // also the mosaic fallback (src[b, 0] alone)
        const int s0 = s4[0], h0 = hw[2 * s0], w0 = hw[2 * s0 + 1];
        int nh, nw;
        resized_hw(h0, w0, H > W ? H : W, &nh, &nw);
        const int top = (H - nh) / 2, left = (W - nw) / 2;
        for (int i = 0; i < nbox[s0]; ++i) {
            const double* in = boxes + ((size_t)s0 * max_in + i) * 5;
            double bb[4];
            yolo_to_albu(in[0], in[1], in[2], in[3], bb);
            if (!area_nz(bb, nh, nw)) continue;
            bb[0] = (bb[0] * nw + left) / W;
            bb[2] = (bb[2] * nw + left) / W;
            bb[1] = (bb[1] * nh + top) / H;
            bb[3] = (bb[3] * nh + top) / H;
            if (n < max_out && finish_box_x<EX>(bb, in[4], p, e, ec, H, W, ob + 5 * n)) ++n;
        }
    }
    *np = n;
    return path;
}

__global__ void aug_boxes(const double* __restrict__ boxes, const int* __restrict__ nbox, int max_in, const int* __restrict__ hw,
                          const int* __restrict__ src, const double* __restrict__ params, int B, int H, int W, float* __restrict__ out,
                          int* __restrict__ counts, int max_out, int* __restrict__ sel) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* ob = out + (size_t)b * max_out * 5;
    int n = 0;
    const int path = row_boxes<false>(boxes, nbox, max_in, hw, src + 4 * b, params + (size_t)b * YOLO_AUG_NPARAM, nullptr, nullptr, H, W,
                                      ob, &n, max_out);
    for (int k = 5 * n; k < 5 * max_out; ++k) ob[k] = 0.f;
    counts[b] = n;
    sel[b] = path;
}

// with the extras: the row's own chain, then its MixUp partner's chain appended (each by its own row's rules, both under the
// rectangles of row b); sel[b] stays the path of row b's own image
__global__ void aug_boxes_ex(const double* __restrict__ boxes, const int* __restrict__ nbox, int max_in, const int* __restrict__ hw,
                             const int* __restrict__ src, const double* __restrict__ params, const double* __restrict__ extra, int B,
                             int H, int W, float* __restrict__ out, int* __restrict__ counts, int max_out, int* __restrict__ sel) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* ob = out + (size_t)b * max_out * 5;
    const double* e = extra + (size_t)b * YOLO_AUGX_NPARAM;
    int n = 0;
    const int path = row_boxes<true>(boxes, nbox, max_in, hw, src + 4 * b, params + (size_t)b * YOLO_AUG_NPARAM, e, e, H, W, ob, &n,
                                     max_out);
    const int pt = mix_partner(e, b, B);
    if (pt >= 0)
        row_boxes<true>(boxes, nbox, max_in, hw, src + 4 * pt, params + (size_t)pt * YOLO_AUG_NPARAM,
                        extra + (size_t)pt * YOLO_AUGX_NPARAM, e, H, W, ob, &n, max_out);
    for (int k = 5 * n; k < 5 * max_out; ++k) ob[k] = 0.f;
    counts[b] = n;
    sel[b] = path;
}

// ---------------------------------------------------------------------------------------------------- pixels
__global__ __launch_bounds__(256) void aug_canvas_u8(const unsigned char* __restrict__ pool, const long long* __restrict__ offsets,
                                                     const int* __restrict__ hw, const int* __restrict__ src,
                                                     const double* __restrict__ params, const int* __restrict__ sel, int H, int W,
                                                     unsigned char* __restrict__ staging) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int y = idx / W, x = idx - y * W;
    const double* p = params + (size_t)b * YOLO_AUG_NPARAM;
    const int* s4 = src + 4 * b;
    const int path = sel[b];
    unsigned char px[3] = {0, 0, 0};
    if (path >= 0) {                                                          // mosaic (square: S = W = H)
        const int S = W;
        int h, w;
        resized_hw(hw[2 * s4[0]], hw[2 * s4[0] + 1], S, &h, &w);
        const int xp = (int)((p[YOLO_AUG_MOSAIC + 2 * path] * 2) * S), yp = (int)((p[YOLO_AUG_MOSAIC + 2 * path + 1] * 2) * S);
        const int Y = y + yp - (2 * S - 2 * h) / 2, X = x + xp - (2 * S - 2 * w) / 2;
        if ((unsigned)Y < (unsigned)(2 * h) && (unsigned)X < (unsigned)(2 * w)) {
            const int q = (Y >= h ? 2 : 0) + (X >= w ? 1 : 0), k = s4[q];
            resize_px(pool + offsets[k], hw[2 * k], hw[2 * k + 1], h, w, Y >= h ? Y - h : Y, X >= w ? X - w : X, px);
        } else {
            px[0] = px[1] = px[2] = 255;                                      // PadIfNeeded(2S, 2S, value 255)
        }
    } else {
        const int k = s4[0], h0 = hw[2 * k], w0 = hw[2 * k + 1];
        int nh, nw;
        resized_hw(h0, w0, H > W ? H : W, &nh, &nw);
        const int yy = y - (H - nh) / 2, xx = x - (W - nw) / 2;
        if ((unsigned)yy < (unsigned)nh && (unsigned)xx < (unsigned)nw) resize_px(pool + offsets[k], h0, w0, nh, nw, yy, xx, px);
    }
    if (path != SEL_LETTERBOX && hsv_on(p))
        hsv_shift(px, p[YOLO_AUG_HUE], p[YOLO_AUG_SAT], p[YOLO_AUG_VAL]);
    unsigned char* o = staging + ((size_t)b * H * W + idx) * 3;
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
}

__global__ __launch_bounds__(256) void aug_warp_normalize(const unsigned char* __restrict__ staging, const double* __restrict__ params,
                                                          const int* __restrict__ sel, int H, int W, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    warp_normalize_px(staging + (size_t)b * H * W * 3, params + (size_t)b * YOLO_AUG_NPARAM, sel[b] != SEL_LETTERBOX, H, W, idx,
                      out + (size_t)b * 3 * H * W + idx);
}

// aug_warp_normalize with the extras: chain(b), blended with chain(partner), then erased; still one thread per output pixel
__global__ __launch_bounds__(256) void aug_warp_normalize_ex(const unsigned char* __restrict__ staging, const double* __restrict__ params,
                                                             const double* __restrict__ extra, const int* __restrict__ sel, int B, int H,
                                                             int W, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int pt = mix_partner(extra + (size_t)b * YOLO_AUGX_NPARAM, b, B);
    extras_px(staging, params, extra, b, pt, sel[b] != SEL_LETTERBOX, pt >= 0 && sel[pt] != SEL_LETTERBOX, H, W, idx,
              out + (size_t)b * 3 * H * W + idx);
}

// host validation shared by both entry points; on success *S is the resize target (the longer canvas side)
static int check_tables(const int32_t* hw, int n_pool, const int32_t* src, int B, int H, int W, const char* what) {
    if (!hw || !src || n_pool <= 0 || B <= 0 || H < 32 || W < 32 || H % 32 || W % 32)
        return fail(YOLO_ERR_ARG, "%s: bad arguments (B %d, n_pool %d, canvas %dx%d: multiples of 32 needed)", what, B, n_pool, H, W);
    for (int i = 0; i < n_pool; ++i)
        if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0) return fail(YOLO_ERR_ARG, "%s: pool image %d has no pixels", what, i);
    const int S = H > W ? H : W;
    for (int b = 0; b < B; ++b) {
        const int32_t* s4 = src + 4 * b;
        if (s4[0] < 0 || s4[0] >= n_pool) return fail(YOLO_ERR_ARG, "%s: src[%d][0] = %d out of range [0, %d)", what, b, s4[0], n_pool);
        if (s4[1] < 0) {
            if (s4[1] != -1 || s4[2] != -1 || s4[3] != -1)
                return fail(YOLO_ERR_ARG, "%s: src row %d: slots 1..3 are all -1 (standard) or all images (mosaic)", what, b);
            int nh, nw;
            resized_hw(hw[2 * s4[0]], hw[2 * s4[0] + 1], S, &nh, &nw);
            if (nh > H || nw > W) return fail(YOLO_ERR_ARG, "%s: image %d resized to %dx%d exceeds the %dx%d canvas", what, b, nh, nw, H, W);
            continue;
        }
        if (H != W) return fail(YOLO_ERR_ARG, "%s: mosaic needs a square canvas (got %dx%d)", what, H, W);
        int h0, w0;
        resized_hw(hw[2 * s4[0]], hw[2 * s4[0] + 1], S, &h0, &w0);
        for (int q = 1; q < 4; ++q) {
            if (s4[q] < 0 || s4[q] >= n_pool)
                return fail(YOLO_ERR_ARG, "%s: src[%d][%d] = %d out of range [0, %d)", what, b, q, s4[q], n_pool);
            int h, w;
            resized_hw(hw[2 * s4[q]], hw[2 * s4[q] + 1], S, &h, &w);
            if (h != h0 || w != w0)
                return fail(YOLO_ERR_ARG, "%s: mosaic row %d: image %d resizes to %dx%d, image 0 to %dx%d (they must match)", what, b, q,
                            h, w, h0, w0);
        }
    }
    return YOLO_OK;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

size_t yolo_augment_workspace_bytes(int b, int out_h, int out_w) {
    if (b <= 0 || out_h <= 0 || out_w <= 0) return 0;
    return ((size_t)b * out_h * out_w * 3 + 255) / 256 * 256;
}

int yolo_augment_boxes_ex(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, const int32_t* src_dev,
                          const int32_t* hw, int n_pool, const int32_t* src, const double* params, const double* extra, int b,
                          int out_h, int out_w, float* out_boxes, int32_t* counts, int max_out, int32_t* sel, void* stream) {
    if (!boxes || !nbox || !hw_dev || !src_dev || !params || !out_boxes || !counts || !sel || max_in <= 0 || max_out <= 0)
        return fail(YOLO_ERR_ARG, "augment_boxes: bad arguments");
    const int rc = check_tables(hw, n_pool, src, b, out_h, out_w, "augment_boxes");
    if (rc != YOLO_OK) return rc;
    if (extra)
        hipLaunchKernelGGL(aug_boxes_ex, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, boxes, nbox, max_in, hw_dev, src_dev,
                           params, extra, b, out_h, out_w, out_boxes, counts, max_out, sel);
    else
        hipLaunchKernelGGL(aug_boxes, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, boxes, nbox, max_in, hw_dev, src_dev,
                           params, b, out_h, out_w, out_boxes, counts, max_out, sel);
    return check_launch("augment_boxes");
}

int yolo_augment_boxes(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, const int32_t* src_dev,
                       const int32_t* hw, int n_pool, const int32_t* src, const double* params, int b, int out_h, int out_w,
                       float* out_boxes, int32_t* counts, int max_out, int32_t* sel, void* stream) {
    return yolo_augment_boxes_ex(boxes, nbox, max_in, hw_dev, src_dev, hw, n_pool, src, params, nullptr, b, out_h, out_w, out_boxes,
                                 counts, max_out, sel, stream);
}

int yolo_augment_images_ex(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, const int32_t* src_dev,
                           const int32_t* hw, int n_pool, const int32_t* src, const double* params, const double* extra,
                           const int32_t* sel, int b, int out_h, int out_w, void* staging, float* out_chw, void* stream) {
    if (!pool || !offsets || !hw_dev || !src_dev || !params || !sel || !staging || !out_chw)
        return fail(YOLO_ERR_ARG, "augment_images: bad arguments");
    const int rc = check_tables(hw, n_pool, src, b, out_h, out_w, "augment_images");
    if (rc != YOLO_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ceil_div(out_h * out_w, 256), b);
    hipLaunchKernelGGL(aug_canvas_u8, grid, dim3(256), 0, s, pool, (const long long*)offsets, hw_dev, src_dev, params, sel, out_h, out_w,
                       (unsigned char*)staging);
    int e = check_launch("augment_images (canvas)");
    if (e != YOLO_OK) return e;
    if (extra)
        hipLaunchKernelGGL(aug_warp_normalize_ex, grid, dim3(256), 0, s, (const unsigned char*)staging, params, extra, sel, b, out_h,
                           out_w, out_chw);
    else
        hipLaunchKernelGGL(aug_warp_normalize, grid, dim3(256), 0, s, (const unsigned char*)staging, params, sel, out_h, out_w, out_chw);
    return check_launch("augment_images (warp)");
}

int yolo_augment_images(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, const int32_t* src_dev,
                        const int32_t* hw, int n_pool, const int32_t* src, const double* params, const int32_t* sel, int b, int out_h,
                        int out_w, void* staging, float* out_chw, void* stream) {
    return yolo_augment_images_ex(pool, offsets, hw_dev, src_dev, hw, n_pool, src, params, nullptr, sel, b, out_h, out_w, staging,
                                  out_chw, stream);
}

}  // extern "C"
