// tta.hip — test-time augmentation: the views of a batch (mirrored and / or resized copies) and the unmapping of the boxes a
// mirrored view reports.   BUILD WITH -ffp-contract=off.
//
// Nothing of the reference. The arithmetic is defined in include/yolo_mi355x.h and DESIGN.md 7.20 (bilinear with half-pixel centres,
// coordinates in double, the edge rule of lin_coef in resample.h, the blend in fp32 with one rounding per operation);
// tests/fuse_ref.py restates it. Decoded boxes are normalised per axis, so a resized view needs no unmapping at all and a mirrored
// one only cx <- 1 - cx / cy <- 1 - cy.
#include "common.h"

namespace yolo {

// source rows s, s + 1 (clamped) and the weight of the second, for output index d of an axis resized from src_n to dst_n
__device__ __forceinline__ void view_coef(int d, double scale, int src_n, int* s0, int* s1, float* wt) {
    double f = (d + 0.5) * scale - 0.5;
    int s = (int)floor(f);
    f -= s;
    if (s < 0) { s = 0; f = 0; }
    if (s >= src_n - 1) { s = src_n - 1; f = 0; }
    *s0 = s;
    *s1 = s + 1 < src_n ? s + 1 : s;
    *wt = (float)f;
}

// grid (ceil(oh * ow / 256), planes), planes = n * c walked with the grid's y stride
__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ x, int planes, int h, int w, float* __restrict__ out, int oh, int ow,
                                                       int flip_lr, int flip_ud) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= oh * ow) return;
    const int Y = o / ow, X = o - Y * ow;
    const int dy = flip_ud ? oh - 1 - Y : Y, dx = flip_lr ? ow - 1 - X : X;
    const bool same = oh == h && ow == w;
    int y0 = Y, y1 = Y, x0 = X, x1 = X;
    float wy = 0.f, wx = 0.f;
    if (!same) {
        view_coef(Y, (double)h / oh, h, &y0, &y1, &wy);
        view_coef(X, (double)w / ow, w, &x0, &x1, &wx);
    }
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        const float* src = x + (size_t)p * h * w;
        float v;
        if (same) {
            v = src[(size_t)Y * w + X];
        } else {
            const float p00 = src[(size_t)y0 * w + x0], p01 = src[(size_t)y0 * w + x1];
            const float p10 = src[(size_t)y1 * w + x0], p11 = src[(size_t)y1 * w + x1];
            const float top = (1.0f - wx) * p00 + wx * p01;
            const float bot = (1.0f - wx) * p10 + wx * p11;
            v = (1.0f - wy) * top + wy * bot;
        }
        out[(size_t)p * oh * ow + (size_t)dy * ow + dx] = v;
    }
}

// grid (ceil(rows / 256), B)
__global__ __launch_bounds__(256) void boxes_unflip_kernel(float* __restrict__ boxes, int n_total, int row_offset, int rows, int flip_lr, int flip_ud) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float* p = boxes + ((size_t)blockIdx.y * n_total + row_offset + r) * 6;
    if (flip_lr) p[0] = 1.0f - p[0];
    if (flip_ud) p[1] = 1.0f - p[1];
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_tta_view(const float* x_nchw, int n, int c, int h, int w, float* out_nchw, int oh, int ow, int flip_lr, int flip_ud, void* stream) {
    if (!x_nchw || !out_nchw || x_nchw == out_nchw) return fail(YOLO_ERR_ARG, "tta_view: null pointer or in place");
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return fail(YOLO_ERR_ARG, "tta_view: bad sizes");
    if ((long long)n * c > 0x7fffffffll || (long long)h * w > 0x7fffffffll || (long long)oh * ow > 0x7fffffffll)
        return fail(YOLO_ERR_UNSUPPORTED, "tta_view: too large");
    const int planes = n * c;
    const dim3 grid(ceil_div(oh * ow, 256), planes < 65535 ? planes : 65535);
    hipLaunchKernelGGL(tta_view_kernel, grid, dim3(256), 0, (hipStream_t)stream, x_nchw, planes, h, w, out_nchw, oh, ow, flip_lr ? 1 : 0,
                       flip_ud ? 1 : 0);
    return check_launch("tta_view");
}

int yolo_boxes_unflip(float* boxes, int b, int n_total, int row_offset, int rows, int flip_lr, int flip_ud, void* stream) {
    if (b <= 0 || n_total < 0 || row_offset < 0 || rows < 0 || (long long)row_offset + rows > n_total)
        return fail(YOLO_ERR_ARG, "boxes_unflip: rows [%d, %d + %d) of %d", row_offset, row_offset, rows, n_total);
    if (b > 65535) return fail(YOLO_ERR_UNSUPPORTED, "boxes_unflip: b = %d too large", b);
    if (rows == 0 || (!flip_lr && !flip_ud)) return YOLO_OK;
    if (!boxes) return fail(YOLO_ERR_ARG, "boxes_unflip: null pointer");
    hipLaunchKernelGGL(boxes_unflip_kernel, dim3(ceil_div(rows, 256), b), dim3(256), 0, (hipStream_t)stream, boxes, n_total, row_offset, rows,
                       flip_lr ? 1 : 0, flip_ud ? 1 : 0);
    return check_launch("boxes_unflip");
}

}  // extern "C"
