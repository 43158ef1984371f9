// augment.h — the arithmetic that the training transform chain (augment.hip) and the training crops (crops.hip) share: the
// albumentations box rules, the ShiftScaleRotate matrix, the OpenCV uint8 HSV shift, the fixed-point warp + normalise of one
// output pixel, and the extras (rotation, vertical flip, MixUp, Cutout). Both units must produce the same bits for the same
// canvas, so there is one copy, as resample.h is for the resize.
// Build the including objects with -ffp-contract=off.
#pragma once
#include "common.h"
#include "resample.h"

namespace yolo {

// ---------------------------------------------------------------------------------------------------- boxes
// getRotationMatrix2D((W/2, H/2), theta, scale) from alpha = scale cos, beta = scale sin, with (dx W, dy H) added to the
// translation column (albumentations shift_scale_rotate); m = [m00 m01 m02; m10 m11 m12]
__device__ __forceinline__ void ssr_matrix_ab(double alpha, double beta, const double* p, int H, int W, double m[6]) {
    const double cx = 0.5 * W, cy = 0.5 * H;
    m[0] = alpha; m[1] = beta; m[2] = (1.0 - alpha) * cx - beta * cy;
    m[3] = -beta; m[4] = alpha; m[5] = beta * cx + (1.0 - alpha) * cy;
    m[2] += p[YOLO_AUG_DX] * W;
    m[5] += p[YOLO_AUG_DY] * H;
}
// the chain without the extras: rotation 0 (the reference's rotate_limit)
__device__ __forceinline__ void ssr_matrix(const double* p, int H, int W, double m[6]) {
    ssr_matrix_ab(p[YOLO_AUG_SCALE], 0.0 * p[YOLO_AUG_SCALE], p, H, W, m);
}
// with the rotation of the extras row e; cos 1, sin 0 gives ssr_matrix's bits
__device__ __forceinline__ void ssr_matrix_rot(const double* p, const double* e, int H, int W, double m[6]) {
    ssr_matrix_ab(p[YOLO_AUG_SCALE] * e[YOLO_AUGX_ROT_COS], p[YOLO_AUG_SCALE] * e[YOLO_AUGX_ROT_SIN], p, H, W, m);
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

// Pixel (y, x) of warpAffine(canvas st, forward matrix m): inverse matrix, AB_BITS 10 / INTER_BITS 5 fixed point, 32 x 32
// bilinear table of 15-bit weights, constant border 0 per tap. m is overwritten.
__device__ __forceinline__ void warp_px(const unsigned char* __restrict__ st, double m[6], int H, int W, int y, int x, unsigned char px[3]) {
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
}

// Output pixel idx of one (H, W) canvas: fixed-point warpAffine sample of its uint8 HWC staging canvas st (or a copy), flip,
// x (1/255), stored to the three planes behind o. aug: the row's ShiftScaleRotate and flip apply.
__device__ __forceinline__ void warp_normalize_px(const unsigned char* __restrict__ st, const double* p, bool aug, int H, int W, int idx,
                                                  float* __restrict__ o) {
    const int y = idx / W;
    const int x = (aug && p[YOLO_AUG_DO_FLIP] != 0.0) ? W - 1 - (idx - y * W) : idx - y * W;   // flip of the warped image
    unsigned char px[3];
    if (aug && p[YOLO_AUG_DO_SSR] != 0.0) {
        double m[6];
        ssr_matrix(p, H, W, m);
        warp_px(st, m, H, W, y, x, px);
    } else {
        const unsigned char* s = st + ((size_t)y * W + x) * 3;
        px[0] = s[0]; px[1] = s[1]; px[2] = s[2];
    }
    const float inv = 1.0f / 255.0f;
    for (int c = 0; c < 3; ++c) o[(size_t)c * H * W] = (float)px[c] * inv;
}

// ---------------------------------------------------------------------------------------------------- extras
// (YOLO_AUGX_* in the header: rotation, vertical flip, MixUp, Cutout). e is the row's extras; the kernels evaluate no sin or cos.
// the row mixed into row b of B, or -1: an integer value in [0, B) other than b
__device__ __forceinline__ int mix_partner(const double* e, int b, int B) {
    const double v = e[YOLO_AUGX_MIX_PARTNER];
    if (!(v >= 0.0 && v < (double)B) || v != floor(v)) return -1;             // NaN too
    return (int)v == b ? -1 : (int)v;
}

__device__ __forceinline__ int cut_count(const double* e) {
    const double v = e[YOLO_AUGX_CUT_N];
    return v >= 1.0 ? (v >= 4.0 ? 4 : (int)v) : 0;                             // NaN -> 0
}

// erase rectangle k in pixels of the (H, W) output canvas: X0 <= x < X1, Y0 <= y < Y1
__device__ __forceinline__ void cut_rect(const double* e, int k, int H, int W, int r[4]) {
    const double* q = e + YOLO_AUGX_CUT_RECT + 4 * k;
    r[0] = (int)(clip01(q[0]) * W); r[1] = (int)(clip01(q[1]) * H);
    r[2] = (int)(clip01(q[2]) * W); r[3] = (int)(clip01(q[3]) * H);
}

// the box chain of row (p, e) without Cutout: ShiftScaleRotate with the rotation (largest_box: the envelope of the four rotated
// corners; the two-corner code of finish_box when cos = 1 and sin = 0) + clip + min_visibility 0.4, both flips. b stays albumentations.
__device__ __forceinline__ bool chain_box(double b[4], const double* p, const double* e, int H, int W) {
    if (p[YOLO_AUG_DO_SSR] != 0.0) {
        double m[6], t[4];
        ssr_matrix_rot(p, e, H, W, m);
        if (e[YOLO_AUGX_ROT_COS] == 1.0 && e[YOLO_AUGX_ROT_SIN] == 0.0) {
            t[0] = (m[0] * (b[0] * W) + m[2]) / W; t[1] = (m[4] * (b[1] * H) + m[5]) / H;
            t[2] = (m[0] * (b[2] * W) + m[2]) / W; t[3] = (m[4] * (b[3] * H) + m[5]) / H;
        } else {
            for (int c = 0; c < 4; ++c) {
                const double px = b[2 * (c & 1)] * W, py = b[1 + (c & 2)] * H;
                const double tx = (m[0] * px + m[1] * py + m[2]) / W, ty = (m[3] * px + m[4] * py + m[5]) / H;
                t[0] = c ? fmin(t[0], tx) : tx; t[1] = c ? fmin(t[1], ty) : ty;
                t[2] = c ? fmax(t[2], tx) : tx; t[3] = c ? fmax(t[3], ty) : ty;
            }
        }
        const double ta = (t[2] * W - t[0] * W) * (t[3] * H - t[1] * H);
        for (int k = 0; k < 4; ++k) b[k] = clip01(t[k]);
        const double ca = (b[2] * W - b[0] * W) * (b[3] * H - b[1] * H);
        if (!(ca != 0.0 && ca / ta >= 0.4)) return false;
    }
    if (p[YOLO_AUG_DO_FLIP] != 0.0) {
        const double x0 = 1.0 - b[2], x1 = 1.0 - b[0];
        b[0] = x0; b[2] = x1;
    }
    if (e[YOLO_AUGX_DO_VFLIP] != 0.0) {
        const double y0 = 1.0 - b[3], y1 = 1.0 - b[1];
        b[1] = y0; b[3] = y1;
    }
    return true;
}

// Cutout's box rule with the rectangles of ec (the OUTPUT row's extras): dropped iff more than CUT_COVER of the box lies inside one
__device__ __forceinline__ bool cut_drops(const double b[4], const double* ec, int H, int W) {
    const int n = cut_count(ec);
    const double lim = ec[YOLO_AUGX_CUT_COVER] * ((b[2] - b[0]) * (b[3] - b[1]));
    for (int k = 0; k < n; ++k) {
        int r[4];
        cut_rect(ec, k, H, W, r);
        if (r[2] <= r[0] || r[3] <= r[1]) continue;                            // an empty rectangle drops nothing
        const double R[4] = {(double)r[0] / W, (double)r[1] / H, (double)r[2] / W, (double)r[3] / H};
        const double inter = fmax(0.0, fmin(b[2], R[2]) - fmax(b[0], R[0])) * fmax(0.0, fmin(b[3], R[3]) - fmax(b[1], R[1]));
        if (inter > lim) return true;
    }
    return false;
}

// finish_box for a kernel built with (EX) or without the extras: e the chain's own row, ec the output row whose rectangles apply
template <bool EX>
__device__ __forceinline__ bool finish_box_x(double b[4], double cls, const double* p, const double* e, const double* ec, int H, int W,
                                             float* out) {
    if constexpr (!EX) {
        return finish_box(b, cls, p, H, W, out);
    } else {
        if (!chain_box(b, p, e, H, W) || cut_drops(b, ec, H, W)) return false;
        store_box(b, cls, out);
        return true;
    }
}

// chain(r) at output pixel (y, x): the uint8 pixel of row r's staging canvas st after its warp (with the rotation) and both flips
__device__ __forceinline__ void chain_px(const unsigned char* __restrict__ st, const double* p, const double* e, bool aug, int H, int W,
                                         int y, int x, unsigned char px[3]) {
    if (aug && p[YOLO_AUG_DO_FLIP] != 0.0) x = W - 1 - x;
    if (aug && e[YOLO_AUGX_DO_VFLIP] != 0.0) y = H - 1 - y;
    if (aug && p[YOLO_AUG_DO_SSR] != 0.0) {
        double m[6];
        ssr_matrix_rot(p, e, H, W, m);
        warp_px(st, m, H, W, y, x, px);
    } else {
        const unsigned char* s = st + ((size_t)y * W + x) * 3;
        px[0] = s[0]; px[1] = s[1]; px[2] = s[2];
    }
}

// Output pixel idx of row b with the extras: chain(b), mixed with chain(pt) when pt >= 0, then erased. staging / params / extra are
// the whole batch's; aug_b / aug_p as aug of warp_normalize_px for row b and its partner.
__device__ __forceinline__ void extras_px(const unsigned char* __restrict__ staging, const double* __restrict__ params,
                                          const double* __restrict__ extra, int b, int pt, bool aug_b, bool aug_p, int H, int W, int idx,
                                          float* __restrict__ o) {
    const int y = idx / W, x = idx - y * W;
    const double* e = extra + (size_t)b * YOLO_AUGX_NPARAM;
    const int n = cut_count(e);
    bool cut = false;
    for (int k = 0; k < n; ++k) {
        int r[4];
        cut_rect(e, k, H, W, r);
        cut = cut || (x >= r[0] && x < r[2] && y >= r[1] && y < r[3]);
    }
    float v[3];
    if (cut) {
        v[0] = v[1] = v[2] = (float)e[YOLO_AUGX_CUT_FILL];
    } else {
        const size_t canvas = (size_t)H * W * 3;
        const float inv = 1.0f / 255.0f;
        unsigned char pa[3];
        chain_px(staging + b * canvas, params + (size_t)b * YOLO_AUG_NPARAM, e, aug_b, H, W, y, x, pa);
        if (pt >= 0) {
            unsigned char pb[3];
            chain_px(staging + pt * canvas, params + (size_t)pt * YOLO_AUG_NPARAM, extra + (size_t)pt * YOLO_AUGX_NPARAM, aug_p, H, W, y, x,
                     pb);
            const float l = (float)e[YOLO_AUGX_MIX_LAMBDA], m = 1.0f - l;
            for (int c = 0; c < 3; ++c) v[c] = ((float)pa[c] * inv) * l + ((float)pb[c] * inv) * m;
        } else {
            for (int c = 0; c < 3; ++c) v[c] = (float)pa[c] * inv;
        }
    }
    for (int c = 0; c < 3; ++c) o[(size_t)c * H * W] = v[c];
}

}  // namespace yolo
