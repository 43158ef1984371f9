// loss_iou.hip — the per-scale loss with terms the reference does not have (yolo_loss_fwd_opts / yolo_loss_bwd_opts):
// GIoU / DIoU / CIoU box regression, BCE objectness, a focal no-object term, label smoothing and free weights.
// Same shape as loss_fused.hip: partial sums, finalize, gradient; one thread per cell in a grid-stride loop, masks as
// predicates, sums through the fixed-order fp64 tree (deterministic), the gradient written analytically, nothing kept
// between forward and backward but counts2. Templated on the box and objectness kind: an instantiation carries only its
// own arithmetic. For one scale, with b = (sig(p0), sig(p1), exp(p2) aw, exp(p3) ah) and g = t0..3 in cell / grid units:
//   x1 = cx - w/2, x2 = x1 + w (y alike);  inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1))
//   union = bw bh + gw gh - inter + 1e-6;  IoU = inter / union   (iou_center: the objectness target of loss_fused.hip)
//   cw = max(x2) - min(x1), ch = max(y2) - min(y1)                (the enclosing box)
//   GIoU = IoU - (C - union) / C,  C = cw ch + 1e-6
//   DIoU = IoU - rho2 / c2,        rho2 = (bx - gx)^2 + (by - gy)^2,  c2 = cw^2 + ch^2 + 1e-6
//   CIoU = DIoU - alpha v,         v = 4/pi^2 (atan(gw/gh) - atan(bw/bh))^2,  alpha = v / (1 - IoU + v + 1e-6), a constant
//   box    = lambda_box * mean over object cells of (1 - XIoU)      (kind MSE: the reference's term, loss.py:71-75)
//   object = lambda_obj * mean of (p4 - IoU)^2 or of BCEWithLogits(p4, IoU), IoU detached
//   noobj  = lambda_noobj * mean over no-object cells of sig(p4)^gamma softplus(p4)
//   class  = lambda_class * mean of CrossEntropy(p5.., t5, label_smoothing = eps)
// At a tie of a min / max pair the gradient takes neither side (a measure-zero choice; identical boxes give exactly 0).
#include "loss.h"

namespace yolo {

struct LossOpts { float gamma, eps, l_box, l_obj, l_noobj, l_cls; };

__device__ __forceinline__ float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// XIoU of the decoded prediction (bx, by, bw, bh) and the target (gx, gy, gw, gh). With GRAD, d[0..3] = dXIoU / d(bx, by, bw, bh).
template <int BOX, bool GRAD>
__device__ __forceinline__ float xiou(float bx, float by, float bw, float bh, float gx, float gy, float gw, float gh, float* iou_out,
                                      float* d) {
    const float bx1 = bx - bw / 2, by1 = by - bh / 2, gx1 = gx - gw / 2, gy1 = gy - gh / 2;
    const float bx2 = bx1 + bw, by2 = by1 + bh, gx2 = gx1 + gw, gy2 = gy1 + gh;
    const float iwr = fminf(bx2, gx2) - fmaxf(bx1, gx1), ihr = fminf(by2, gy2) - fmaxf(by1, gy1);
    const float iw = iwr > 0.f ? iwr : 0.f, ih = ihr > 0.f ? ihr : 0.f;
    const float inter = iw * ih;
    const float uni = bw * bh + gw * gh - inter + 1e-6f;
    const float iou = inter / uni;
    *iou_out = iou;
    const float cw = fmaxf(bx2, gx2) - fminf(bx1, gx1), ch = fmaxf(by2, gy2) - fminf(by1, gy1);
    // dXIoU / d(inter), d(bw bh), d(cw), d(ch), and what reaches (bx, by, bw, bh) past the corners
    float k_int = (uni + inter) / (uni * uni), k_area = -inter / (uni * uni), k_cw = 0.f, k_ch = 0.f;
    float dbx = 0.f, dby = 0.f, dbw = 0.f, dbh = 0.f;
    float val = iou;
    if constexpr (BOX == YOLO_LOSS_BOX_GIOU) {
        const float C = cw * ch + 1e-6f;
        val = iou - (C - uni) / C;
        if constexpr (GRAD) {
            k_int -= 1.f / C;
            k_area += 1.f / C;
            k_cw = -uni * ch / (C * C);
            k_ch = -uni * cw / (C * C);
        }
    } else {
        const float ex = bx - gx, ey = by - gy;
        const float rho2 = ex * ex + ey * ey, c2 = cw * cw + ch * ch + 1e-6f;
        val = iou - rho2 / c2;
        if constexpr (GRAD) {
            k_cw = 2.f * rho2 * cw / (c2 * c2);
            k_ch = 2.f * rho2 * ch / (c2 * c2);
            dbx = -2.f * ex / c2;
            dby = -2.f * ey / c2;
        }
        if constexpr (BOX == YOLO_LOSS_BOX_CIOU) {
            const float kv = 0.40528473456935109f;             // 4 / pi^2
            const float da = atanf(gw / gh) - atanf(bw / bh);
            const float v = kv * da * da;
            const float alpha = v / (1.f - iou + v + 1e-6f);
            val -= alpha * v;
            if constexpr (GRAD) {                               // -alpha dv: d atan(bw/bh) = (bh dbw - bw dbh) / (bw^2 + bh^2)
                const float q = alpha * 2.f * kv * da / (bw * bw + bh * bh);
                dbw = q * bh;
                dbh = -q * bw;
            }
        }
    }
    if constexpr (GRAD) {
        const float mi = iwr > 0.f ? k_int * ih : 0.f, mj = ihr > 0.f ? k_int * iw : 0.f;     // d inter reaches a corner only where it overlaps
        const float dx2 = (bx2 < gx2 ? mi : 0.f) + (bx2 > gx2 ? k_cw : 0.f), dx1 = -(bx1 > gx1 ? mi : 0.f) - (bx1 < gx1 ? k_cw : 0.f);
        const float dy2 = (by2 < gy2 ? mj : 0.f) + (by2 > gy2 ? k_ch : 0.f), dy1 = -(by1 > gy1 ? mj : 0.f) - (by1 < gy1 ? k_ch : 0.f);
        d[0] = dx1 + dx2 + dbx;
        d[1] = dy1 + dy2 + dby;
        d[2] = 0.5f * (dx2 - dx1) + k_area * bh + dbw;
        d[3] = 0.5f * (dy2 - dy1) + k_area * bw + dbh;
    }
    return val;
}

// sums[blk][6] (double): box, obj, noobj, class, n_obj, n_noobj
template <int BOX, int OBJ>
__global__ __launch_bounds__(256) void loss_opts_partial(const LossArgs p, const LossOpts o, double* __restrict__ partial) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (long long cell = blockIdx.x * 256LL + threadIdx.x; cell < p.cells; cell += (long long)gridDim.x * 256) {
        const float* t = p.tgt + cell * 6;
        const float t4 = t[4];
        if (t4 == 0.f) {
            int a;
            const float x = cell_ptr(p, cell, &a)[4 * p.sk];
            const float sp = softplusf_(x);
            acc[2] += (double)(o.gamma > 0.f ? expf(-o.gamma * softplusf_(-x)) * sp : sp);     // sig^gamma = exp(gamma log sig)
            acc[5] += 1.0;
        } else if (t4 == 1.f) {
            int a;
            const float* q = cell_ptr(p, cell, &a);
            const float aw = p.anchors[a * 2], ah = p.anchors[a * 2 + 1];
            const float p0 = q[0], p1 = q[p.sk], p2 = q[2 * p.sk], p3 = q[3 * p.sk], p4 = q[4 * p.sk];
            float iou;
            if constexpr (BOX == YOLO_LOSS_BOX_MSE) {
                iou = iou_center(sigmoidf_(p0), sigmoidf_(p1), expf(p2) * aw, expf(p3) * ah, t[0], t[1], t[2], t[3]);
                const float e0 = p0 - t[0], e1 = sigmoidf_(p1) - t[1];
                const float e2 = sigmoidf_(p2) - logf(1e-16f + t[2] / aw), e3 = p3 - logf(1e-16f + t[3] / ah);
                acc[0] += (double)(e0 * e0) + (double)(e1 * e1) + (double)(e2 * e2) + (double)(e3 * e3);
            } else {
                const float v = xiou<BOX, false>(sigmoidf_(p0), sigmoidf_(p1), expf(p2) * aw, expf(p3) * ah, t[0], t[1], t[2], t[3], &iou,
                                                 nullptr);
                acc[0] += (double)(1.f - v);
            }
            if constexpr (OBJ == YOLO_LOSS_OBJ_MSE) {
                const float d4 = p4 - iou;
                acc[1] += (double)(d4 * d4);
            } else {
                acc[1] += (double)(softplusf_(p4) - p4 * iou);
            }
            float mx = -INFINITY;
            for (int k = 0; k < p.nc; ++k) mx = fmaxf(mx, q[(5 + k) * p.sk]);
            float se = 0.f, sx = 0.f;
            for (int k = 0; k < p.nc; ++k) {
                const float xk = q[(5 + k) * p.sk];
                se += expf(xk - mx);
                sx += xk;
            }
            const int cls = (int)t[5];
            const float lse = mx + logf(se);
            acc[3] += (double)((1.f - o.eps) * (lse - q[(5 + cls) * p.sk]) + o.eps * (lse - sx / (float)p.nc));
            acc[4] += 1.0;
        }
    }
    __shared__ double red[256];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        __syncthreads();
        red[threadIdx.x] = acc[k];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {                 // fixed tree: deterministic
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x * 6 + k] = red[0];
    }
}

// as loss_finalize of loss_fused.hip, with the weights as arguments; box_div = 4 for the MSE box term (a mean over 4 n_obj elements)
__global__ __launch_bounds__(64) void loss_opts_finalize(const double* __restrict__ partial, int nblk, const LossOpts o, double box_div,
                                                         float* __restrict__ losses4, float* __restrict__ counts2) {
    __shared__ double red[6][64];
    const int l = threadIdx.x;
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int b = l; b < nblk; b += 64)
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += partial[b * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][l] = s[k];
    __syncthreads();
    for (int st = 32; st > 0; st >>= 1) {
        if (l < st)
#pragma unroll
            for (int k = 0; k < 6; ++k) red[k][l] += red[k][l + st];
        __syncthreads();
    }
    if (l != 0) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = red[k][0];
    const double n_obj = s[4], n_noobj = s[5];
    losses4[0] = n_obj > 0 ? (float)((double)o.l_box * s[0] / (box_div * n_obj)) : 0.f;
    losses4[1] = n_obj > 0 ? (float)((double)o.l_obj * s[1] / n_obj) : 0.f;
    losses4[2] = (float)((double)o.l_noobj * s[2] / n_noobj);                 // empty mean = NaN, like torch
    losses4[3] = n_obj > 0 ? (float)((double)o.l_cls * s[3] / n_obj) : 0.f;
    counts2[0] = (float)n_obj;
    counts2[1] = (float)n_noobj;
}

// dpred (B,3,gh,gw,5+nc) contiguous = sum_k gout[k] * d loss_k / d pred
template <int BOX, int OBJ>
__global__ __launch_bounds__(256) void loss_opts_grad(const LossArgs p, const LossOpts o, const float* __restrict__ counts2,
                                                      const float* __restrict__ gout4, float* __restrict__ dpred) {
    const float n_obj = counts2[0], n_noobj = counts2[1];
    const float g_box = gout4[0] * o.l_box, g_obj = gout4[1] * o.l_obj, g_noobj = gout4[2] * o.l_noobj, g_cls = gout4[3] * o.l_cls;
    const int D = 5 + p.nc;
    for (long long cell = blockIdx.x * 256LL + threadIdx.x; cell < p.cells; cell += (long long)gridDim.x * 256) {
        const float* t = p.tgt + cell * 6;
        float* d = dpred + cell * D;
        const float t4 = t[4];
        if (t4 == 1.f) {
            int a;
            const float* q = cell_ptr(p, cell, &a);
            const float aw = p.anchors[a * 2], ah = p.anchors[a * 2 + 1];
            const float p0 = q[0], p1 = q[p.sk], p2 = q[2 * p.sk], p3 = q[3 * p.sk], p4 = q[4 * p.sk];
            const float s0 = sigmoidf_(p0), s1 = sigmoidf_(p1);
            float iou;
            if constexpr (BOX == YOLO_LOSS_BOX_MSE) {
                const float s2 = sigmoidf_(p2);
                iou = iou_center(s0, s1, expf(p2) * aw, expf(p3) * ah, t[0], t[1], t[2], t[3]);
                const float kb = g_box * 2.f / (4.f * n_obj);
                d[0] = kb * (p0 - t[0]);
                d[1] = kb * (s1 - t[1]) * s1 * (1.f - s1);
                d[2] = kb * (s2 - logf(1e-16f + t[2] / aw)) * s2 * (1.f - s2);
                d[3] = kb * (p3 - logf(1e-16f + t[3] / ah));
            } else {
                const float bw = expf(p2) * aw, bh = expf(p3) * ah;
                float dv[4];
                xiou<BOX, true>(s0, s1, bw, bh, t[0], t[1], t[2], t[3], &iou, dv);
                const float kb = -g_box / n_obj;                                   // the term is 1 - XIoU
                d[0] = kb * dv[0] * s0 * (1.f - s0);
                d[1] = kb * dv[1] * s1 * (1.f - s1);
                d[2] = kb * dv[2] * bw;
                d[3] = kb * dv[3] * bh;
            }
            if constexpr (OBJ == YOLO_LOSS_OBJ_MSE)
                d[4] = g_obj * 2.f * (p4 - iou) / n_obj;
            else
                d[4] = g_obj * (sigmoidf_(p4) - iou) / n_obj;
            float mx = -INFINITY;
            for (int k = 0; k < p.nc; ++k) mx = fmaxf(mx, q[(5 + k) * p.sk]);
            float se = 0.f;
            for (int k = 0; k < p.nc; ++k) se += expf(q[(5 + k) * p.sk] - mx);
            const int cls = (int)t[5];
            const float kc = g_cls / n_obj, off = o.eps / (float)p.nc;
            for (int k = 0; k < p.nc; ++k) d[5 + k] = kc * (expf(q[(5 + k) * p.sk] - mx) / se - ((k == cls ? 1.f - o.eps : 0.f) + off));
        } else {
            for (int k = 0; k < D; ++k) d[k] = 0.f;
            if (t4 == 0.f) {
                int a;
                const float x = cell_ptr(p, cell, &a)[4 * p.sk];
                const float sg = sigmoidf_(x);
                float g = sg;
                if (o.gamma > 0.f) g = expf(-o.gamma * softplusf_(-x)) * (o.gamma * (1.f - sg) * softplusf_(x) + sg);
                d[4] = g_noobj * g / n_noobj;
            }
        }
    }
}

// run `body` with the constants BOX and OBJ bound to the run-time kinds (validated by the caller)
#define YOLO_SWITCH_LOSS_OBJ(obj, ...)                                                                  \
    if ((obj) == YOLO_LOSS_OBJ_BCE) { constexpr int OBJ = YOLO_LOSS_OBJ_BCE; __VA_ARGS__; }             \
    else { constexpr int OBJ = YOLO_LOSS_OBJ_MSE; __VA_ARGS__; }
#define YOLO_SWITCH_LOSS_KINDS(box, obj, ...)                                                                            \
    switch (box) {                                                                                                        \
    case YOLO_LOSS_BOX_GIOU: { constexpr int BOX = YOLO_LOSS_BOX_GIOU; YOLO_SWITCH_LOSS_OBJ(obj, __VA_ARGS__) } break;    \
    case YOLO_LOSS_BOX_DIOU: { constexpr int BOX = YOLO_LOSS_BOX_DIOU; YOLO_SWITCH_LOSS_OBJ(obj, __VA_ARGS__) } break;    \
    case YOLO_LOSS_BOX_CIOU: { constexpr int BOX = YOLO_LOSS_BOX_CIOU; YOLO_SWITCH_LOSS_OBJ(obj, __VA_ARGS__) } break;    \
    default: { constexpr int BOX = YOLO_LOSS_BOX_MSE; YOLO_SWITCH_LOSS_OBJ(obj, __VA_ARGS__) } break;                     \
    }

static int check_loss_opts(const yolo_loss_opts* u, LossOpts* o) {
    if (!u) return fail(YOLO_ERR_ARG, "loss opts: null pointer");
    if (u->box_kind < YOLO_LOSS_BOX_MSE || u->box_kind > YOLO_LOSS_BOX_CIOU) return fail(YOLO_ERR_ARG, "loss opts: box_kind %d", u->box_kind);
    if (u->obj_kind < YOLO_LOSS_OBJ_MSE || u->obj_kind > YOLO_LOSS_OBJ_BCE) return fail(YOLO_ERR_ARG, "loss opts: obj_kind %d", u->obj_kind);
    if (!(u->focal_gamma >= 0.f) || !std::isfinite(u->focal_gamma))
        return fail(YOLO_ERR_ARG, "loss opts: focal_gamma %g is not a finite number >= 0", (double)u->focal_gamma);
    if (!(u->label_smoothing >= 0.f && u->label_smoothing < 1.f))
        return fail(YOLO_ERR_ARG, "loss opts: label_smoothing %g outside [0, 1)", (double)u->label_smoothing);
    if (!std::isfinite(u->lambda_box) || !std::isfinite(u->lambda_obj) || !std::isfinite(u->lambda_noobj) || !std::isfinite(u->lambda_class))
        return fail(YOLO_ERR_ARG, "loss opts: a lambda is not finite");
    o->gamma = u->focal_gamma; o->eps = u->label_smoothing;
    o->l_box = u->lambda_box; o->l_obj = u->lambda_obj; o->l_noobj = u->lambda_noobj; o->l_cls = u->lambda_class;
    return YOLO_OK;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_loss_fwd_opts(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int gh, int gw,
                       int nc, float* losses4, float* counts2, void* workspace, size_t workspace_bytes, const yolo_loss_opts* opts,
                       void* stream) {
    LossArgs a;
    LossOpts o;
    int rc = fill_loss_args(&a, pred, strides5, target, anchors_3x2, b, gh, gw, nc);
    if (rc) return rc;
    rc = check_loss_opts(opts, &o);
    if (rc) return rc;
    if (!losses4 || !counts2 || !workspace || workspace_bytes < yolo_loss_workspace_bytes_hw(b, gh, gw))
        return fail(YOLO_ERR_WORKSPACE, "loss: workspace");
    const int nblk = loss_blocks(a.cells);
    hipStream_t s = (hipStream_t)stream;
    YOLO_SWITCH_LOSS_KINDS(opts->box_kind, opts->obj_kind,
                           hipLaunchKernelGGL((loss_opts_partial<BOX, OBJ>), dim3(nblk), dim3(256), 0, s, a, o, (double*)workspace));
    rc = check_launch("loss_opts_partial");
    if (rc) return rc;
    const double box_div = opts->box_kind == YOLO_LOSS_BOX_MSE ? 4.0 : 1.0;
    hipLaunchKernelGGL(loss_opts_finalize, dim3(1), dim3(64), 0, s, (const double*)workspace, nblk, o, box_div, losses4, counts2);
    return check_launch("loss_opts_finalize");
}

int yolo_loss_bwd_opts(const float* pred, const int64_t* strides5, const float* target, const float* anchors_3x2, int b, int gh, int gw,
                       int nc, const float* counts2, const float* grad_losses4, float* dpred, const yolo_loss_opts* opts, void* stream) {
    LossArgs a;
    LossOpts o;
    int rc = fill_loss_args(&a, pred, strides5, target, anchors_3x2, b, gh, gw, nc);
    if (rc) return rc;
    rc = check_loss_opts(opts, &o);
    if (rc) return rc;
    if (!counts2 || !grad_losses4 || !dpred) return fail(YOLO_ERR_ARG, "loss_bwd: null pointer");
    const int nblk = loss_blocks(a.cells);
    hipStream_t s = (hipStream_t)stream;
    YOLO_SWITCH_LOSS_KINDS(opts->box_kind, opts->obj_kind,
                           hipLaunchKernelGGL((loss_opts_grad<BOX, OBJ>), dim3(nblk), dim3(256), 0, s, a, o, counts2, grad_losses4, dpred));
    return check_launch("loss_opts_grad");
}

}  // extern "C"
