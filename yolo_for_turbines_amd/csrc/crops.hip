// crops.hip — training on tiles: box-aware windows cut from a device-resident pool of full-size images, the training-side
// counterpart of tiles.hip. Nothing of the reference is replaced: its dataset was tiled offline. The contract is in
// include/yolo_mi355x.h ("training on tiles") and DESIGN.md 7.27.
//
// The kernels hold no randomness: every draw comes from a per-crop parameter row (YOLO_CROP_*). Launches, on one stream:
//   crop_boxes          one thread per crop (sequential over its rows, like aug_boxes): the level size, the window, the picked
//                       box; every row of the image mapped to the tile, clipped, filtered by visibility, then finish_box of
//                       augment.h; writes windows[b] = {image, y0, x0, LH, LW, picked}, which the pixel kernel reads;
//   crop_tile<false>    augmentation off: one workgroup per 64 x 16 output tile of one crop, level pixels straight to fp32 CHW;
//   crop_tile<true>     the same sample, HSV shift; a crop with ShiftScaleRotate on is stored as the uint8 HWC staging canvas of
//                       augment.hip, a crop without it is flipped, normalised and written straight to the output (the warp would
//                       only copy its canvas pixel: the same bits without the staging round trip);
//   crop_warp_normalize the warp / flip / normalise of augment.h on the staged crops.
// With the augmentation extras (rotation, vertical flip, MixUp, Cutout: yolo_crop_*_ex) crop_boxes_ex appends the partner's boxes,
// crop_tile<true, true> stages EVERY crop (a crop without ShiftScaleRotate may be another crop's MixUp partner, and which crops are
// partners is known on the device only) and crop_warp_normalize_ex warps, blends and erases in one launch.
// A level pixel is resize_px of resample.h (the library's one INTER_LINEAR; the identity at scale 1), so without augmentation the
// output has the bits of yolo_tile_gather / yolo_tile_gather_scaled. PARITY UNPINNED, like augment.hip.
// Built with -ffp-contract=off: the window and box arithmetic is fp64 with every operation rounded once.
#include <cstdint>
#include "common.h"
#include "resample.h"
#include "augment.h"

namespace yolo {

constexpr int kCropTileW = 64, kCropTileH = 16;              // output pixels per workgroup: 16 lanes x 4 pixels across, 16 rows
constexpr int kCropThreads = 256;
constexpr int kCropWin = 6;                                  // int32 per windows row

// max(1, rint(n scale)), half to even: one side of yolo_tile_level_hw. n scale < 2^31 for scale <= 8 and the sizes a pool holds.
__device__ __forceinline__ int level_side(int n, double scale) {
    const double v = rint(n * scale);
    return v < 1.0 ? 1 : (v > 2147483647.0 ? 2147483647 : (int)v);
}

// one axis of the window: level length L, tile t, jitter j, the picked centre c (object crop) or no centre (background)
__device__ __forceinline__ int window_origin(int L, int t, double j, bool object, double c) {
    if (L <= t) return 0;
    const double v = object ? floor(c * L - j * (t - 1)) : floor(j * (L - t + 1));
    return (int)fmin(fmax(v, 0.0), (double)(L - t));         // NaN -> 0
}

// Crop r: its windows row (written to win unless NULL) and its kept boxes, appended to ob at *np (at most max_out rows). EX: the box
// chain runs with the crop's extras e and the rectangles of ec, the extras of the crop being written.
template <bool EX>
__device__ __forceinline__ void crop_row_boxes(const double* __restrict__ boxes, const int* __restrict__ nbox, int max_in,
                                               const int* __restrict__ hw, int n_pool, const int* __restrict__ src,
                                               const double* __restrict__ crop_params, const int* __restrict__ origins,
                                               const double* __restrict__ aug_params, const double* e, const double* ec, int r, int th,
                                               int tw, double min_vis, float* ob, int* np, int max_out, int* win) {
    const int k = src[r];
    int n = *np;
    if ((unsigned)k >= (unsigned)n_pool) {                   // an index outside the pool: an empty crop, nothing is read
        if (win) { win[0] = -1; win[1] = win[2] = 0; win[3] = win[4] = 1; win[5] = -1; }
        return;
    }
    const double* cp = crop_params + (size_t)r * YOLO_CROP_NPARAM;
    const int h = hw[2 * k], w = hw[2 * k + 1], nb = min(nbox[k], max_in);
    double scale = cp[YOLO_CROP_SCALE];
    if (!(scale > 0.0 && scale <= 8.0)) scale = 1.0;
    const int LH = level_side(h, scale), LW = level_side(w, scale);
    int picked = -1, y0, x0;
    if (origins) {
        y0 = origins[2 * r]; x0 = origins[2 * r + 1];
    } else {
        double cx = 0.0, cy = 0.0;
        if (cp[YOLO_CROP_BACKGROUND] == 0.0 && nb > 0) {
            const double u = floor(cp[YOLO_CROP_U_PICK] * nb);
            picked = (int)fmin(fmax(u, 0.0), (double)(nb - 1));
            const double* in = boxes + ((size_t)k * max_in + picked) * 5;
            cx = in[0]; cy = in[1];
        }
        x0 = window_origin(LW, tw, cp[YOLO_CROP_JX], picked >= 0, cx);
        y0 = window_origin(LH, th, cp[YOLO_CROP_JY], picked >= 0, cy);
    }
    if (win) { win[0] = k; win[1] = y0; win[2] = x0; win[3] = LH; win[4] = LW; win[5] = picked; }
    const double* ap = aug_params ? aug_params + (size_t)r * YOLO_AUG_NPARAM : nullptr;
    for (int i = 0; i < nb && i < max_in; ++i) {
        const double* in = boxes + ((size_t)k * max_in + i) * 5;
        double bb[4];
        yolo_to_albu(in[0], in[1], in[2], in[3], bb);
        if (!area_nz(bb, h, w)) continue;
        const double t[4] = {(bb[0] * LW - x0) / tw, (bb[1] * LH - y0) / th, (bb[2] * LW - x0) / tw, (bb[3] * LH - y0) / th};
        const double ta = (t[2] * tw - t[0] * tw) * (t[3] * th - t[1] * th);
        double c[4];
        for (int q = 0; q < 4; ++q) c[q] = clip01(t[q]);
        const double ca = (c[2] * tw - c[0] * tw) * (c[3] * th - c[1] * th);
        if (!(ca != 0.0 && ca / ta >= min_vis)) continue;
        if (n >= max_out) continue;
        if (ap) {
            if (finish_box_x<EX>(c, in[4], ap, e, ec, th, tw, ob + 5 * n)) ++n;
        } else {
            store_box(c, in[4], ob + 5 * n);
            ++n;
        }
    }
    *np = n;
}

__global__ void crop_boxes(const double* __restrict__ boxes, const int* __restrict__ nbox, int max_in, const int* __restrict__ hw,
                           int n_pool, const int* __restrict__ src, const double* __restrict__ crop_params,
                           const int* __restrict__ origins, const double* __restrict__ aug_params, int B, int th, int tw,
                           double min_vis, float* __restrict__ out, int* __restrict__ counts, int max_out, int* __restrict__ windows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* ob = out + (size_t)b * max_out * 5;
    int n = 0;
    crop_row_boxes<false>(boxes, nbox, max_in, hw, n_pool, src, crop_params, origins, aug_params, nullptr, nullptr, b, th, tw, min_vis, ob,
                          &n, max_out, windows + (size_t)b * kCropWin);
    for (int q = 5 * n; q < 5 * max_out; ++q) ob[q] = 0.f;
    counts[b] = n;
}

// with the extras (aug_params is not NULL): the crop's own boxes, then those of its MixUp partner's crop appended, each by its own
// row's rules and both under the rectangles of crop b
__global__ void crop_boxes_ex(const double* __restrict__ boxes, const int* __restrict__ nbox, int max_in, const int* __restrict__ hw,
                              int n_pool, const int* __restrict__ src, const double* __restrict__ crop_params,
                              const int* __restrict__ origins, const double* __restrict__ aug_params, const double* __restrict__ extra,
                              int B, int th, int tw, double min_vis, float* __restrict__ out, int* __restrict__ counts, int max_out,
                              int* __restrict__ windows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* ob = out + (size_t)b * max_out * 5;
    const double* e = extra + (size_t)b * YOLO_AUGX_NPARAM;
    int n = 0;
    crop_row_boxes<true>(boxes, nbox, max_in, hw, n_pool, src, crop_params, origins, aug_params, e, e, b, th, tw, min_vis, ob, &n, max_out,
                         windows + (size_t)b * kCropWin);
    const int pt = mix_partner(e, b, B);
    if (pt >= 0)
        crop_row_boxes<true>(boxes, nbox, max_in, hw, n_pool, src, crop_params, origins, aug_params, extra + (size_t)pt * YOLO_AUGX_NPARAM,
                             e, pt, th, tw, min_vis, ob, &n, max_out, nullptr);
    for (int q = 5 * n; q < 5 * max_out; ++q) ob[q] = 0.f;
    counts[b] = n;
}

// One workgroup per 64 x 16 tile of one crop's canvas: grid (tiles of a crop, crops). Lane l of a wave holds pixels
// 4 (l % 16) .. + 3 of row l / 16 of the wave's four rows: 48 bytes a row segment of 16 lanes is 192 contiguous source bytes at
// scale 1, and a wave writes four 256-byte fp32 row segments per plane (or four 192-byte segments of the staging canvas).
// al4: the pool's first byte is 4-byte aligned, so a lane's 12 source bytes may come from the dwords around them.
// vec: bit 0 the staging canvas takes dword stores, bit 1 the output takes 16-byte stores.
// ALL: every crop is stored to the staging canvas, also one without ShiftScaleRotate (the extras: another crop may mix it in).
template <bool AUG, bool ALL = false>
__global__ __launch_bounds__(kCropThreads) void crop_tile_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ offsets,
                                                                  const int* __restrict__ hw, int n_pool, const int* __restrict__ windows,
                                                                  const double* __restrict__ aug_params, int th, int tw, int tiles_x,
                                                                  int al4, int vec, unsigned char* __restrict__ staging,
                                                                  float* __restrict__ out) {
    __shared__ int sx0[kCropTileW], sx1[kCropTileW], sa[kCropTileW];                // source columns; a0 | a1 << 16
    __shared__ int sy0[kCropTileH], sy1[kCropTileH], sb[kCropTileH];                // source rows; b0 | b1 << 16
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
    const int oy0 = tyi * kCropTileH, ox0 = txi * kCropTileW;
    const int* win = windows + (size_t)b * kCropWin;
    const int k = win[0];
    const bool live = (unsigned)k < (unsigned)n_pool;                               // uniform over the block
    const long long y0 = win[1], x0 = win[2];
    const int LH = live ? win[3] : 0, LW = live ? win[4] : 0;
    const int h = live ? hw[2 * k] : 1, w = live ? hw[2 * k + 1] : 1;
    const bool ident = LH == h && LW == w;                    // resize_px copies
    if (live && !ident) {
        if (tid < kCropTileW) {
            const long long X = x0 + ox0 + tid;
            int a = 0, c = 0, a0 = 0, a1 = 0;
            if (X >= 0 && X < LW) lin_coef((int)X, (double)w / LW, w, &a, &c, &a0, &a1);
            sx0[tid] = a; sx1[tid] = c; sa[tid] = a0 | (a1 << 16);
        } else if (tid < kCropTileW + kCropTileH) {
            const int i = tid - kCropTileW;
            const long long Y = y0 + oy0 + i;
            int a = 0, c = 0, b0 = 0, b1 = 0;
            if (Y >= 0 && Y < LH) lin_coef((int)Y, (double)h / LH, h, &a, &c, &b0, &b1);
            sy0[i] = a; sy1[i] = c; sb[i] = b0 | (b1 << 16);
        }
    }
    __syncthreads();
    const int r = tid >> 4, ty = oy0 + r, tx = ox0 + (tid & 15) * 4;
    if (ty >= th || tx >= tw) return;                         // tw % 4 == 0: a lane's four pixels are inside together
    const long long Y = y0 + ty, X = x0 + tx;
    const bool row_in = live && Y >= 0 && Y < LH;
    unsigned char px[4][3] = {};
    if (row_in) {
        const size_t base = (size_t)offsets[k];
        if (ident && X >= 0 && X + 3 < LW) {
            // scale 1, four pixels of one source row: 12 contiguous bytes at any (odd) address
            const size_t at = base + ((size_t)Y * w + (size_t)X) * 3, lo = at & ~(size_t)3;
            const unsigned sh = (unsigned)(at & 3) * 8;
            const size_t img_end = base + (size_t)h * w * 3;
            if (al4 && (sh == 0 || lo + 16 <= img_end)) {      // the dwords that hold them lie inside the image's bytes
                const unsigned* d = reinterpret_cast<const unsigned*>(pool + lo);
                unsigned q[3];
                if (sh == 0) {
                    q[0] = d[0]; q[1] = d[1]; q[2] = d[2];
                } else {
                    const unsigned d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
                    q[0] = (d0 >> sh) | (d1 << (32 - sh));
                    q[1] = (d1 >> sh) | (d2 << (32 - sh));
                    q[2] = (d2 >> sh) | (d3 << (32 - sh));
                }
                for (int i = 0; i < 12; ++i) px[i / 3][i % 3] = (unsigned char)(q[i >> 2] >> (8 * (i & 3)));
            } else {
                for (int i = 0; i < 12; ++i) px[i / 3][i % 3] = pool[at + i];
            }
        } else {
            const unsigned char* img = pool + base;
            const int yA = ident ? (int)Y : sy0[r], yB = ident ? (int)Y : sy1[r];
            const int b0 = sb[r] & 0xffff, b1 = sb[r] >> 16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (X + e < 0 || X + e >= LW) continue;
                if (ident) {
                    const unsigned char* s = img + ((size_t)Y * w + (size_t)(X + e)) * 3;
                    px[e][0] = s[0]; px[e][1] = s[1]; px[e][2] = s[2];
                    continue;
                }
                const int j = (tid & 15) * 4 + e;
                const int xA = sx0[j], xB = sx1[j], a0 = sa[j] & 0xffff, a1 = sa[j] >> 16;
                const unsigned char* p00 = img + ((size_t)yA * w + xA) * 3;
                const unsigned char* p01 = img + ((size_t)yA * w + xB) * 3;
                const unsigned char* p10 = img + ((size_t)yB * w + xA) * 3;
                const unsigned char* p11 = img + ((size_t)yB * w + xB) * 3;
                for (int c = 0; c < 3; ++c) {                 // the blend of resize_px (resample.h) on taps from the LDS tables
                    const int r0 = p00[c] * a0 + p01[c] * a1;
                    const int r1 = p10[c] * a0 + p11[c] * a1;
                    const int t = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                    px[e][c] = (unsigned char)(t < 0 ? 0 : (t > 255 ? 255 : t));
                }
            }
        }
    }
    const size_t at = ((size_t)b * th + ty) * (size_t)tw + tx;                      // first of the lane's four pixels on the canvas
    if constexpr (AUG) {
        const double* p = aug_params + (size_t)b * YOLO_AUG_NPARAM;
        if (hsv_on(p)) {                                      // on the zero padding too (the reference shifts the padded canvas)
            const double hue = p[YOLO_AUG_HUE], sat = p[YOLO_AUG_SAT], val = p[YOLO_AUG_VAL];
            for (int e = 0; e < 4; ++e) hsv_shift(px[e], hue, sat, val);
        }
        if (!ALL && p[YOLO_AUG_DO_SSR] == 0.0) {
            // no warp for this crop: warp_normalize_px would copy the canvas pixel, so flip and normalise here and skip the
            // staging round trip (crop_warp_normalize leaves such a crop alone)
            const bool flip = p[YOLO_AUG_DO_FLIP] != 0.0;
            const float inv = 1.0f / 255.0f;
            const size_t plane = (size_t)th * tw;
            float* o = out + (size_t)b * 3 * plane + (size_t)ty * tw + (flip ? tw - 4 - tx : tx);
            for (int c = 0; c < 3; ++c) {
                const float f[4] = {(float)px[0][c] * inv, (float)px[1][c] * inv, (float)px[2][c] * inv, (float)px[3][c] * inv};
                const f32x4 v = flip ? f32x4{f[3], f[2], f[1], f[0]} : f32x4{f[0], f[1], f[2], f[3]};
                if (vec & 2) *reinterpret_cast<f32x4*>(o + c * plane) = v;
                else for (int e = 0; e < 4; ++e) o[c * plane + e] = v[e];
            }
            return;
        }
        unsigned char* o = staging + at * 3;                  // 12 bytes at a multiple of 12
        if (vec & 1) {
            unsigned* d = reinterpret_cast<unsigned*>(o);
            for (int q = 0; q < 3; ++q) {
                unsigned v = 0;
                for (int i = 0; i < 4; ++i) v |= (unsigned)px[(4 * q + i) / 3][(4 * q + i) % 3] << (8 * i);
                d[q] = v;
            }
        } else {
            for (int i = 0; i < 12; ++i) o[i] = px[i / 3][i % 3];
        }
    } else {
        const float inv = 1.0f / 255.0f;                      // the normalisation of yolo_letterbox
        const size_t plane = (size_t)th * tw;
        float* o = out + (size_t)b * 3 * plane + (size_t)ty * tw + tx;
        for (int c = 0; c < 3; ++c) {
            const f32x4 v = {(float)px[0][c] * inv, (float)px[1][c] * inv, (float)px[2][c] * inv, (float)px[3][c] * inv};
            if (vec & 2) *reinterpret_cast<f32x4*>(o + c * plane) = v;
            else for (int e = 0; e < 4; ++e) o[c * plane + e] = v[e];
        }
    }
}

// aug_warp_normalize of augment.hip on the staged crops (those with ShiftScaleRotate on): every row is augmented
__global__ __launch_bounds__(256) void crop_warp_normalize(const unsigned char* __restrict__ staging, const double* __restrict__ params,
                                                           int H, int W, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    if (params[(size_t)b * YOLO_AUG_NPARAM + YOLO_AUG_DO_SSR] == 0.0) return;      // crop_tile_kernel has written this crop's output
    warp_normalize_px(staging + (size_t)b * H * W * 3, params + (size_t)b * YOLO_AUG_NPARAM, true, H, W, idx,
                      out + (size_t)b * 3 * H * W + idx);
}

// aug_warp_normalize_ex of augment.hip on the crops, all of them staged: chain(b), blended with chain(partner), then erased
__global__ __launch_bounds__(256) void crop_warp_normalize_ex(const unsigned char* __restrict__ staging, const double* __restrict__ params,
                                                              const double* __restrict__ extra, int B, int H, int W,
                                                              float* __restrict__ out) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int pt = mix_partner(extra + (size_t)b * YOLO_AUGX_NPARAM, b, B);
    extras_px(staging, params, extra, b, pt, true, true, H, W, idx, out + (size_t)b * 3 * H * W + idx);
}

static int crop_args(const char* what, int n_pool, int b, int th, int tw) {
    if (n_pool <= 0 || b <= 0 || b > 65535) return fail(YOLO_ERR_ARG, "%s: bad arguments (n_pool %d, b %d: 1 .. 65535 crops)", what, n_pool, b);
    if (th < 32 || tw < 32 || th % 32 || tw % 32 || (long long)th * tw > 0x7fffffffll / 3)
        return fail(YOLO_ERR_ARG, "%s: tile %dx%d: positive multiples of 32 needed", what, th, tw);
    return YOLO_OK;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_crop_boxes_ex(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, int n_pool, const int32_t* src_dev,
                       const double* crop_params, const int32_t* origins_dev, const double* aug_params, const double* extra, int b,
                       int tile_h, int tile_w, double min_visibility, float* out_boxes, int32_t* counts, int max_out, int32_t* windows,
                       void* stream) {
    if (!boxes || !nbox || !hw_dev || !src_dev || !crop_params || !out_boxes || !counts || !windows || max_in <= 0 || max_out <= 0)
        return fail(YOLO_ERR_ARG, "crop_boxes: bad arguments");
    if (extra && !aug_params) return fail(YOLO_ERR_ARG, "crop_boxes: extra (the augmentation extras) needs aug_params");
    if (int rc = crop_args("crop_boxes", n_pool, b, tile_h, tile_w)) return rc;
    if (!(min_visibility >= 0.0 && min_visibility <= 1.0))   // NaN too
        return fail(YOLO_ERR_ARG, "crop_boxes: min_visibility %g is not in [0, 1]", min_visibility);
    if (extra)
        hipLaunchKernelGGL(crop_boxes_ex, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, boxes, nbox, max_in, hw_dev, n_pool,
                           src_dev, crop_params, origins_dev, aug_params, extra, b, tile_h, tile_w, min_visibility, out_boxes, counts,
                           max_out, windows);
    else
        hipLaunchKernelGGL(crop_boxes, dim3(ceil_div(b, 64)), dim3(64), 0, (hipStream_t)stream, boxes, nbox, max_in, hw_dev, n_pool,
                           src_dev, crop_params, origins_dev, aug_params, b, tile_h, tile_w, min_visibility, out_boxes, counts, max_out,
                           windows);
    return check_launch("crop_boxes");
}

int yolo_crop_boxes(const double* boxes, const int32_t* nbox, int max_in, const int32_t* hw_dev, int n_pool, const int32_t* src_dev,
                    const double* crop_params, const int32_t* origins_dev, const double* aug_params, int b, int tile_h, int tile_w,
                    double min_visibility, float* out_boxes, int32_t* counts, int max_out, int32_t* windows, void* stream) {
    return yolo_crop_boxes_ex(boxes, nbox, max_in, hw_dev, n_pool, src_dev, crop_params, origins_dev, aug_params, nullptr, b, tile_h,
                              tile_w, min_visibility, out_boxes, counts, max_out, windows, stream);
}

int yolo_crop_images_ex(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, int n_pool, const int32_t* windows,
                        const double* aug_params, const double* extra, int b, int tile_h, int tile_w, void* staging, float* out_chw,
                        void* stream) {
    if (!pool || !offsets || !hw_dev || !windows || !out_chw || (aug_params && !staging))
        return fail(YOLO_ERR_ARG, "crop_images: bad arguments");
    if (extra && !aug_params) return fail(YOLO_ERR_ARG, "crop_images: extra (the augmentation extras) needs aug_params");
    if (int rc = crop_args("crop_images", n_pool, b, tile_h, tile_w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = ceil_div(tile_w, kCropTileW);
    const dim3 grid(tiles_x * ceil_div(tile_h, kCropTileH), b), block(kCropThreads);
    const int al4 = ((uintptr_t)pool & 3) == 0;
    const int vec_out = ((uintptr_t)out_chw & 15) == 0 ? 2 : 0;   // vec: bit 0 dword stores to the staging canvas, bit 1 16-byte stores to out
    if (!aug_params) {
        hipLaunchKernelGGL(crop_tile_kernel<false>, grid, block, 0, s, pool, (const long long*)offsets, hw_dev, n_pool, windows, aug_params,
                           tile_h, tile_w, tiles_x, al4, vec_out, (unsigned char*)nullptr, out_chw);
        return check_launch("crop_images");
    }
    const int vec = vec_out | (int)(((uintptr_t)staging & 3) == 0);
    const dim3 wgrid(ceil_div(tile_h * tile_w, 256), b);
    if (extra) {
        hipLaunchKernelGGL((crop_tile_kernel<true, true>), grid, block, 0, s, pool, (const long long*)offsets, hw_dev, n_pool, windows,
                           aug_params, tile_h, tile_w, tiles_x, al4, vec, (unsigned char*)staging, out_chw);
        int e = check_launch("crop_images (canvas)");
        if (e != YOLO_OK) return e;
        hipLaunchKernelGGL(crop_warp_normalize_ex, wgrid, dim3(256), 0, s, (const unsigned char*)staging, aug_params, extra, b, tile_h,
                           tile_w, out_chw);
        return check_launch("crop_images (warp)");
    }
    hipLaunchKernelGGL(crop_tile_kernel<true>, grid, block, 0, s, pool, (const long long*)offsets, hw_dev, n_pool, windows, aug_params, tile_h,
                       tile_w, tiles_x, al4, vec, (unsigned char*)staging, out_chw);
    int e = check_launch("crop_images (canvas)");
    if (e != YOLO_OK) return e;
    hipLaunchKernelGGL(crop_warp_normalize, wgrid, dim3(256), 0, s, (const unsigned char*)staging, aug_params, tile_h, tile_w, out_chw);
    return check_launch("crop_images (warp)");
}

int yolo_crop_images(const unsigned char* pool, const int64_t* offsets, const int32_t* hw_dev, int n_pool, const int32_t* windows,
                     const double* aug_params, int b, int tile_h, int tile_w, void* staging, float* out_chw, void* stream) {
    return yolo_crop_images_ex(pool, offsets, hw_dev, n_pool, windows, aug_params, nullptr, b, tile_h, tile_w, staging, out_chw, stream);
}

}  // extern "C"
