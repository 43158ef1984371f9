// targets.hip — ground-truth tensor builder for the loss (one of the steps next to the hot path).
//
// Replaces the per-sample Python loop of YOLODataset.__getitem__ (reference: code/dataset.py:119-161) for a whole
// batch: for every ground-truth box (x, y, w, h, class; normalised), rank the 9 anchors by width/height IoU
// (utils.py:22-36), give the box to the best FREE anchor of each scale —
//     target[scale][anchor, i, j] = [g x - j, g y - i, w g, h g, 1, class],  i = int(g y), j = int(g x)
// (per axis on an H x W canvas: gw for x and w, gh for y and h; see yolo_build_targets_hw)
// — and mark the scale's other free anchors with IoU > 0.5 as ignored (objectness -1). Reference behaviours kept:
// "free" is tested on element 0 of the cell (x offset, dataset.py:141), so a cell whose stored x offset is exactly
// 0 still looks free; boxes are processed in list order; grid arithmetic is done in double like the Python floats
// and rounded to fp32 at the store; IoU and its ranking are fp32 (torch tensors).
// The assignment is sequential per image (every box sees the cells written by the previous ones) and independent
// across images: one thread per image; the data is a few KB per image, so this is latency-, not bandwidth-bound.
#include "common.h"

namespace yolo {

__global__ void build_targets_kernel(const float* __restrict__ boxes, const int* __restrict__ counts, int max_boxes,
                                     const float* __restrict__ anchors, int B, int H, int W, float ignore_thr,
                                     float* __restrict__ t0, float* __restrict__ t1, float* __restrict__ t2) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int gh[3] = {H / 32, H / 16, H / 8}, gw[3] = {W / 32, W / 16, W / 8};
    float* T[3] = {t0 + (size_t)b * 3 * gh[0] * gw[0] * 6, t1 + (size_t)b * 3 * gh[1] * gw[1] * 6, t2 + (size_t)b * 3 * gh[2] * gw[2] * 6};
    // an H x W canvas is the square canvas of side L = max(H, W) with its padding cropped away: box sizes normalised to the
    // canvas are compared with the (L-normalised) anchors as w W/L, h H/L. Square: both factors are exactly 1.0f.
    const int Lc = H > W ? H : W;
    const float rw = (float)((double)W / Lc), rh = (float)((double)H / Lc);
    float aw[9], ah[9];
    for (int a = 0; a < 9; ++a) { aw[a] = anchors[2 * a]; ah[a] = anchors[2 * a + 1]; }
    int n = counts[b];
    if (n > max_boxes) n = max_boxes;
    for (int q = 0; q < n; ++q) {
        const float* bx = boxes + ((size_t)b * max_boxes + q) * 5;
        const float x = bx[0], y = bx[1], w = bx[2], h = bx[3];
        const float wl = w * rw, hl = h * rh;
        const int cls = (int)bx[4];
        float iou[9];
        int order[9];
        for (int a = 0; a < 9; ++a) {
            const float inter = fminf(wl, aw[a]) * fminf(hl, ah[a]);
            iou[a] = inter / (wl * hl + aw[a] * ah[a] - inter);
            int pos = a;                                        // stable insertion: descending IoU, ties keep anchor order
            while (pos > 0 && iou[order[pos - 1]] < iou[a]) { order[pos] = order[pos - 1]; --pos; }
            order[pos] = a;
        }
        bool has[3] = {false, false, false};
        for (int r = 0; r < 9; ++r) {
            const int ai = order[r], s = ai / 3, k = ai - 3 * s, gy_n = gh[s], gx_n = gw[s];
            const double gx = (double)gx_n * (double)x, gy = (double)gy_n * (double)y;
            const int i = (int)gy, j = (int)gx;
            if ((unsigned)i >= (unsigned)gy_n || (unsigned)j >= (unsigned)gx_n) continue;  // x or y == 1.0: the reference would raise
            float* cell = T[s] + (((size_t)k * gy_n + i) * gx_n + j) * 6;
            const bool taken = cell[0] != 0.f;
            if (!taken && !has[s]) {
                cell[4] = 1.f;
                cell[5] = (float)cls;
                cell[0] = (float)(gx - j);
                cell[1] = (float)(gy - i);
                cell[2] = (float)((double)w * gx_n);
                cell[3] = (float)((double)h * gy_n);
                has[s] = true;
            } else if (!taken && iou[ai] > ignore_thr) {
                cell[4] = -1.f;
            }
        }
    }
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_build_targets(const float* boxes, const int32_t* counts, int max_boxes, const float* anchors_9x2, int b, int image_size,
                       float ignore_iou, float* t0, float* t1, float* t2, void* stream) {
    return yolo_build_targets_hw(boxes, counts, max_boxes, anchors_9x2, b, image_size, image_size, ignore_iou, t0, t1, t2, stream);
}

int yolo_build_targets_hw(const float* boxes, const int32_t* counts, int max_boxes, const float* anchors_9x2, int b, int image_h,
                          int image_w, float ignore_iou, float* t0, float* t1, float* t2, void* stream) {
    if (!boxes || !counts || !anchors_9x2 || !t0 || !t1 || !t2 || b <= 0 || max_boxes <= 0 || image_h < 32 || image_h % 32 ||
        image_w < 32 || image_w % 32)
        return fail(YOLO_ERR_ARG, "build_targets: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int gh[3] = {image_h / 32, image_h / 16, image_h / 8}, gw[3] = {image_w / 32, image_w / 16, image_w / 8};
    float* t[3] = {t0, t1, t2};
    for (int k = 0; k < 3; ++k)
        if (hipMemsetAsync(t[k], 0, (size_t)b * 3 * gh[k] * gw[k] * 6 * sizeof(float), s) != hipSuccess)
            return fail(YOLO_ERR_LAUNCH, "build_targets: memset");
    hipLaunchKernelGGL(build_targets_kernel, dim3(ceil_div(b, 64)), dim3(64), 0, s, boxes, counts, max_boxes, anchors_9x2, b, image_h,
                       image_w, ignore_iou, t0, t1, t2);
    return check_launch("build_targets");
}

}  // extern "C"
