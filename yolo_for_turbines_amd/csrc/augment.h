// augment.h — the arithmetic that the training transform chain (augment.hip) and the training crops (crops.hip) share: the
// albumentations box rules, the ShiftScaleRotate matrix, the OpenCV uint8 HSV shift and the fixed-point warp + normalise of one
// output pixel. Both units must produce the same bits for the same canvas, so there is one copy, as resample.h is for the resize.
// Build the including objects with -ffp-contract=off.
#pragma once
#include "common.h"
#include "resample.h"

namespace yolo {

// ---------------------------------------------------------------------------------------------------- boxes
// getRotationMatrix2D((W/2, H/2), 0, scale) with (dx W, dy H) added to the translation column (albumentations
// shift_scale_rotate); m = [m00 m01 m02; m10 m11 m12]
__device__ __forceinline__ void ssr_matrix(const double* p, int H, int W, double m[6]) {
    const double alpha = p[YOLO_AUG_SCALE], beta = 0.0 * p[YOLO_AUG_SCALE];
    const double cx = 0.5 * W, cy = 0.5 * H;
    m[0] = alpha; m[1] = beta; m[2] = (1.0 - alpha) * cx - beta * cy;
    m[3] = -beta; m[4] = alpha; m[5] = beta * cx + (1.0 - alpha) * cy;
    m[2] += p[YOLO_AUG_DX] * W;
    m[5] += p[YOLO_AUG_DY] * H;
}

__device__ __forceinline__ double clip01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// albumentations calculate_bbox_area != 0 on a (H, W) image
__device__ __forceinline__ bool area_nz(const double b[4], int H, int W) {
    return (b[2] * W - b[0] * W) * (b[3] * H - b[1] * H) != 0.0;
}

// yolo (cx, cy, w, h) -> albumentations (x_min, y_min, x_max, y_max), clipped to the unit square (BboxParams(clip=True))
__device__ __forceinline__ void yolo_to_albu(double cx, double cy, double w, double h, double b[4]) {
    const double x0 = cx - w / 2, y0 = cy - h / 2;
    b[0] = clip01(x0); b[1] = clip01(y0); b[2] = clip01(x0 + w); b[3] = clip01(y0 + h);
}

// (x_min, y_min, x_max, y_max) -> yolo, rounded to fp32 at the store (the convention of targets.hip)
__device__ __forceinline__ void store_box(const double b[4], double cls, float* out) {
    out[0] = (float)((b[0] + b[2]) / 2.0);
    out[1] = (float)((b[1] + b[3]) / 2.0);
    out[2] = (float)(b[2] - b[0]);
    out[3] = (float)(b[3] - b[1]);
    out[4] = (float)cls;
}

// the part of the chain every path shares: ShiftScaleRotate + clip + min_visibility 0.4, HorizontalFlip, store (yolo, fp32)
__device__ __forceinline__ bool finish_box(double b[4], double cls, const double* p, int H, int W, float* out) {
    if (p[YOLO_AUG_DO_SSR] != 0.0) {
        double m[6];
        ssr_matrix(p, H, W, m);
        double t[4] = {(m[0] * (b[0] * W) + m[2]) / W, (m[4] * (b[1] * H) + m[5]) / H, (m[0] * (b[2] * W) + m[2]) / W,
                       (m[4] * (b[3] * H) + m[5]) / H};
        const double ta = (t[2] * W - t[0] * W) * (t[3] * H - t[1] * H);
        for (int k = 0; k < 4; ++k) b[k] = clip01(t[k]);
        const double ca = (b[2] * W - b[0] * W) * (b[3] * H - b[1] * H);
        if (!(ca != 0.0 && ca / ta >= 0.4)) return false;
    }
    if (p[YOLO_AUG_DO_FLIP] != 0.0) {
        const double x0 = 1.0 - b[2], x1 = 1.0 - b[0];
        b[0] = x0; b[2] = x1;
    }
    store_box(b, cls, out);
    return true;
}

// ---------------------------------------------------------------------------------------------------- pixels
// the row's HueSaturationValue is on and moves something (albumentations returns the image itself for three zero shifts)
__device__ __forceinline__ bool hsv_on(const double* p) {
    return p[YOLO_AUG_DO_HSV] != 0.0 && !(p[YOLO_AUG_HUE] == 0.0 && p[YOLO_AUG_SAT] == 0.0 && p[YOLO_AUG_VAL] == 0.0);
}

// OpenCV RGB2HSV_b (hsv_shift 12, hrange 180), the albumentations LUTs, OpenCV HSV2RGB_b (fp32)
__device__ __forceinline__ void hsv_shift(unsigned char px[3], double hue, double sat, double val) {
    const int r = px[0], g = px[1], bl = px[2];
    int v = bl, vmin = bl;
    v = max(v, g); v = max(v, r);
    vmin = min(vmin, g); vmin = min(vmin, r);
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    const int sdiv = v ? (int)rint(1044480.0 / (double)v) : 0;                // (255 << 12) / v
    const int hdiv = diff ? (int)rint(737280.0 / (6.0 * diff)) : 0;          // (180 << 12) / (6 diff)
    const int s = (diff * sdiv + (1 << 11)) >> 12;
    int h = (vr & (g - bl)) + (~vr & ((vg & (bl - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * hdiv + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    // LUTs: hue trunc(mod(i + hue, 180)), sat / val trunc(clip(i + shift, 0, 255))
    double hm = fmod((double)h + hue, 180.0);
    if (hm != 0.0 && hm < 0.0) hm += 180.0;
    const int H2 = (int)hm;
    const int S2 = (int)fmin(fmax((double)s + sat, 0.0), 255.0);
    const int V2 = (int)fmin(fmax((double)v + val, 0.0), 255.0);
    const float fs = (float)S2 * (1.f / 255.f), fv = (float)V2 * (1.f / 255.f);
    float rf, gf, bf;
    if (fs == 0.f) {
        rf = gf = bf = fv;
    } else {
        const int sector_data[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
        float hh = (float)H2 * (6.f / 180.f);
        hh = fmodf(hh, 6.f);
        int sector = (int)floorf(hh);
        hh -= (float)sector;
        if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
        float tab[4];
        tab[0] = fv;
        tab[1] = fv * (1.f - fs);
        tab[2] = fv * (1.f - fs * hh);
        tab[3] = fv * (1.f - fs * (1.f - hh));
        bf = tab[sector_data[sector][0]];
        gf = tab[sector_data[sector][1]];
        rf = tab[sector_data[sector][2]];
    }
    const float o[3] = {rf * 255.f, gf * 255.f, bf * 255.f};
    for (int c = 0; c < 3; ++c) {
        const int t = (int)rintf(o[c]);
        px[c] = (unsigned char)(t < 0 ? 0 : (t > 255 ? 255 : t));
    }
}

// Output pixel idx of one (H, W) canvas: fixed-point warpAffine sample of its uint8 HWC staging canvas st (or a copy), flip,
// x (1/255), stored to the three planes behind o. aug: the row's ShiftScaleRotate and flip apply.
__device__ __forceinline__ void warp_normalize_px(const unsigned char* __restrict__ st, const double* p, bool aug, int H, int W, int idx,
                                                  float* __restrict__ o) {
    const int y = idx / W;
    const int x = (aug && p[YOLO_AUG_DO_FLIP] != 0.0) ? W - 1 - (idx - y * W) : idx - y * W;   // flip of the warped image
    unsigned char px[3];
    if (aug && p[YOLO_AUG_DO_SSR] != 0.0) {
        // warpAffine: inverse matrix, AB_BITS 10 / INTER_BITS 5 fixed point, 32 x 32 bilinear table of 15-bit weights,
        // constant border 0 per tap
        double m[6];
        ssr_matrix(p, H, W, m);
        double D = m[0] * m[4] - m[1] * m[3];
        D = D != 0.0 ? 1.0 / D : 0.0;
        const double A11 = m[4] * D, A22 = m[0] * D;
        m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22;
        const double b1 = -m[0] * m[2] - m[1] * m[5], b2 = -m[3] * m[2] - m[4] * m[5];
        m[2] = b1; m[5] = b2;
        const int X0 = cv_round((m[1] * y + m[2]) * 1024) + 16, Y0 = cv_round((m[4] * y + m[5]) * 1024) + 16;
        const int X = (X0 + cv_round(m[0] * x * 1024)) >> 5, Y = (Y0 + cv_round(m[3] * x * 1024)) >> 5;
        const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
        const int wt[4] = {(32 - ay) * (32 - ax) * 32, (32 - ay) * ax * 32, ay * (32 - ax) * 32, ay * ax * 32};
        int acc[3] = {0, 0, 0};
        for (int t = 0; t < 4; ++t) {
            const int ty = sy + (t >> 1), tx = sx + (t & 1);
            if ((unsigned)ty < (unsigned)H && (unsigned)tx < (unsigned)W) {
                const unsigned char* s = st + ((size_t)ty * W + tx) * 3;
                for (int c = 0; c < 3; ++c) acc[c] += s[c] * wt[t];
            }
        }
        for (int c = 0; c < 3; ++c) {
            const int v = (acc[c] + (1 << 14)) >> 15;
            px[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    } else {
        const unsigned char* s = st + ((size_t)y * W + x) * 3;
        px[0] = s[0]; px[1] = s[1]; px[2] = s[2];
    }
    const float inv = 1.0f / 255.0f;
    for (int c = 0; c < 3; ++c) o[(size_t)c * H * W] = (float)px[c] * inv;
}

}  // namespace yolo
