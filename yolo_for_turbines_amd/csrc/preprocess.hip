// preprocess.hip — letterbox of one uint8 HWC image into the network's normalised CHW float input
// (the step in front of the forward in demo.predict: config.py:101-113 = albumentations LongestMaxSize -> centred
// PadIfNeeded(value 0) -> Normalize(mean 0, std 1, max 255) -> ToTensorV2; reference: code/config.py:84-113,
// code/demo.py:37-39).
//
// PARITY UNPINNED: cv2 / albumentations are not installed where this was built, so the reference transform could
// not be run to produce golden vectors. The kernel follows OpenCV's published uint8 INTER_LINEAR algorithm
// (resize.cpp: source coordinate (d + 0.5) * scale - 0.5, 11-bit fixed-point coefficients rounded to nearest even,
// horizontal pass in int32, vertical pass ((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2 >> 2) and
// albumentations' size / padding rules (banker's rounding of dim * scale, top/left pad = floor(diff / 2)); it is tested
// bit for bit against oracle/preprocess.py, which restates the same published rules — not against cv2 itself.
#include "common.h"
#include "resample.h"

namespace yolo {

// out: (3, SH, SW) fp32; one thread per output pixel
__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ img, int h, int w, int nh, int nw,
                                                        int pad_top, int pad_left, int SH, int SW, float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= SH * SW) return;
    const int oy = idx / SW, ox = idx - oy * SW;
    const int y = oy - pad_top, x = ox - pad_left;
    float v[3] = {0.f, 0.f, 0.f};
    if ((unsigned)y < (unsigned)nh && (unsigned)x < (unsigned)nw) {
        unsigned char px[3];
        resize_px(img, h, w, nh, nw, y, x, px);
        const float inv = 1.0f / 255.0f;                     // albumentations multiplies by the fp32 reciprocal
        for (int c = 0; c < 3; ++c) v[c] = (float)px[c] * inv;
    }
    for (int c = 0; c < 3; ++c) out[(size_t)c * SH * SW + idx] = v[c];
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_letterbox_canvas(const int32_t* hw, int n, int size, int rect, int32_t* canvas_hw) {
    if (!canvas_hw || size <= 0 || n < 0 || (rect && (n == 0 || !hw))) return fail(YOLO_ERR_ARG, "letterbox_canvas: bad arguments");
    if (!rect) { canvas_hw[0] = canvas_hw[1] = size; return YOLO_OK; }
    int ch = 0, cw = 0;
    for (int i = 0; i < n; ++i) {
        if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0) return fail(YOLO_ERR_ARG, "letterbox_canvas: image %d has no pixels", i);
        int nh, nw;
        resized_hw(hw[2 * i], hw[2 * i + 1], size, &nh, &nw);
        ch = nh > ch ? nh : ch;
        cw = nw > cw ? nw : cw;
    }
    canvas_hw[0] = (ch + 31) / 32 * 32;
    canvas_hw[1] = (cw + 31) / 32 * 32;
    return YOLO_OK;
}

/* new_hw[2] (host, out): resized size before padding; pad_tl[2] (host, out): top / left padding */
int yolo_letterbox(const unsigned char* img_hwc, int h, int w, int size, float* out_chw, int* new_hw, int* pad_tl, void* stream) {
    return yolo_letterbox_hw(img_hwc, h, w, size, size, size, out_chw, new_hw, pad_tl, stream);
}

int yolo_letterbox_hw(const unsigned char* img_hwc, int h, int w, int size, int canvas_h, int canvas_w, float* out_chw, int* new_hw,
                      int* pad_tl, void* stream) {
    if (!img_hwc || !out_chw || h <= 0 || w <= 0 || size <= 0 || canvas_h <= 0 || canvas_w <= 0)
        return fail(YOLO_ERR_ARG, "letterbox: bad arguments");
    int nh, nw;
    resized_hw(h, w, size, &nh, &nw);
    if (nh > canvas_h || nw > canvas_w) return fail(YOLO_ERR_ARG, "letterbox: resized image exceeds the target");
    const int pad_top = (canvas_h - nh) / 2, pad_left = (canvas_w - nw) / 2;
    if (new_hw) { new_hw[0] = nh; new_hw[1] = nw; }
    if (pad_tl) { pad_tl[0] = pad_top; pad_tl[1] = pad_left; }
    hipLaunchKernelGGL(letterbox_kernel, dim3(ceil_div(canvas_h * canvas_w, 256)), dim3(256), 0, (hipStream_t)stream, img_hwc, h, w, nh,
                       nw, pad_top, pad_left, canvas_h, canvas_w, out_chw);
    return check_launch("letterbox");
}

}  // extern "C"
