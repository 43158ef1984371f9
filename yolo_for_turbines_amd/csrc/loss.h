// loss.h — what the per-scale loss units share: loss_fused.hip (the reference's terms) and loss_iou.hip (the optional terms).
#pragma once
#include "common.h"

namespace yolo {

struct LossArgs {
    const float* pred;          // (B,3,gh,gw,5+nc) through element strides
    const float* tgt;           // (B,3,gh,gw,6) contiguous
    const float* anchors;       // (3,2) in grid units
    long long sb, sa, sy, sx, sk;
    int B, gh, gw, nc;
    long long cells;
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// IoU of two cxcywh boxes, utils.py:38-84 with box_format "center"
__device__ __forceinline__ float iou_center(float ax, float ay, float aw, float ah, float bx, float by, float bw, float bh) {
    const float ax1 = ax - aw / 2, ay1 = ay - ah / 2, bx1 = bx - bw / 2, by1 = by - bh / 2;
    float iw = fminf(ax1 + aw, bx1 + bw) - fmaxf(ax1, bx1);
    float ih = fminf(ay1 + ah, by1 + bh) - fmaxf(ay1, by1);
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = iw * ih;
    return inter / (aw * ah + bw * bh - inter + 1e-6f);
}

__device__ __forceinline__ const float* cell_ptr(const LossArgs& p, long long cell, int* a_out) {
    const int x = (int)(cell % p.gw);
    const long long r1 = cell / p.gw;
    const int y = (int)(r1 % p.gh);
    const long long r2 = r1 / p.gh;
    const int a = (int)(r2 % 3);
    const long long b = r2 / 3;
    *a_out = a;
    return p.pred + b * p.sb + a * p.sa + y * p.sy + x * p.sx;
}

inline int loss_blocks(long long cells) {
    long long b = (cells + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

inline int fill_loss_args(LossArgs* a, const float* pred, const int64_t* s5, const float* target, const float* anchors, int b, int gh,
                          int gw, int nc) {
    if (!pred || !s5 || !target || !anchors || b <= 0 || gh <= 0 || gw <= 0 || nc <= 0) return fail(YOLO_ERR_ARG, "loss: bad arguments");
    a->pred = pred; a->tgt = target; a->anchors = anchors;
    a->sb = s5[0]; a->sa = s5[1]; a->sy = s5[2]; a->sx = s5[3]; a->sk = s5[4];
    a->B = b; a->gh = gh; a->gw = gw; a->nc = nc; a->cells = (long long)b * 3 * gh * gw;
    return YOLO_OK;
}

}  // namespace yolo
