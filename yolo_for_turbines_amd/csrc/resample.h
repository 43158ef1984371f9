// resample.h — OpenCV's uint8 INTER_LINEAR resize in fixed point, shared by the letterbox (preprocess.hip) and the training
// augmentation (augment.hip). Both must produce the same bits for the same resize, so there is one copy of the arithmetic.
// Build the including objects with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace yolo {

__device__ __forceinline__ int cv_round(double v) { return (int)rint(v); }          // round half to even, like cvRound

__device__ __forceinline__ void lin_coef(int d, double scale, int src_n, int* s0, int* s1, int* c0, int* c1) {
    double f = (d + 0.5) * scale - 0.5;
    int s = (int)floor(f);
    f -= s;
    if (s < 0) { s = 0; f = 0; }
    if (s >= src_n - 1) { s = src_n - 1; f = 0; }
    *s0 = s;
    *s1 = s + 1 < src_n ? s + 1 : s;
    const float ff = (float)f;
    int a1 = cv_round((double)(ff * 2048.f));
    int a0 = cv_round((double)((1.f - ff) * 2048.f));
    a0 = a0 > 32767 ? 32767 : a0;
    a1 = a1 > 32767 ? 32767 : a1;
    *c0 = a0; *c1 = a1;
}

// pixel (y, x) of the (h, w, 3) uint8 image img resized to (nh, nw); 0 <= y < nh, 0 <= x < nw
__device__ __forceinline__ void resize_px(const unsigned char* __restrict__ img, int h, int w, int nh, int nw, int y, int x,
                                          unsigned char px[3]) {
    if (nh == h && nw == w) {
        for (int c = 0; c < 3; ++c) px[c] = img[((size_t)y * w + x) * 3 + c];
        return;
    }
    const double sx = (double)w / nw, sy = (double)h / nh;
    int x0, x1, a0, a1, y0, y1, b0, b1;
    lin_coef(x, sx, w, &x0, &x1, &a0, &a1);
    lin_coef(y, sy, h, &y0, &y1, &b0, &b1);
    for (int c = 0; c < 3; ++c) {
        const int r0 = img[((size_t)y0 * w + x0) * 3 + c] * a0 + img[((size_t)y0 * w + x1) * 3 + c] * a1;
        const int r1 = img[((size_t)y1 * w + x0) * 3 + c] * a0 + img[((size_t)y1 * w + x1) * 3 + c] * a1;
        const int t = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
        px[c] = (unsigned char)(t < 0 ? 0 : (t > 255 ? 255 : t));
    }
}

// albumentations LongestMaxSize: the size an (h, w) image is resized to (banker's rounding of dim * scale)
__host__ __device__ inline void resized_hw(int h, int w, int size, int* nh_out, int* nw_out) {
    const double scale = (double)size / (double)(h > w ? h : w);
    int nh = h, nw = w;
    if (scale != 1.0) { nh = (int)rint(h * scale); nw = (int)rint(w * scale); }   // albumentations.py3round: half to even
    *nh_out = nh < 1 ? 1 : nh;
    *nw_out = nw < 1 ? 1 : nw;
}

}  // namespace yolo
