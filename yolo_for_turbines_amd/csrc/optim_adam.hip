// optim_adam.hip — the Adam / AdamW update as two launches over every parameter: one thread per tensor for the scalars of
// this step, then one block per 4,096-element chunk for the update (the geometry and the chunk tables of optim.hip).
//
// Replaces `optimizer.step()` of `torch.optim.Adam` / `torch.optim.AdamW` in the mode PyTorch picks by default on the GPU
// (foreach=True, capturable=False, fused=False: `_multi_tensor_adam`), which walks the parameter tensors in about ten
// multi-tensor passes. Here p, g, exp_avg (m) and exp_avg_sq (v) are read once and p, m, v written once: 28 bytes per element,
// 36 with the weight average. The gradient is never written.
//
// Same bits as PyTorch. Its passes were probed one op at a time on the MI355X (PyTorch 2.10, 2^20 random elements at two
// magnitudes, every candidate formula evaluated in fp64 and rounded once; `tools/adam_probe.py`, output in
// `profiles/adam/rounding_probe.txt`). Exactly one candidate per op gave zero mismatches:
//   1  _foreach_neg (maximize)                 g = -g
//   2a _foreach_mul_(p, 1 - lr*wd)             p = p * w0                      w0 = float(1 - lr*wd), formed in fp64
//   2b _foreach_add(g, p, alpha=wd)            g = fma(float(wd), p, g)        ONE rounding (two: 1,456 of 2^20 differ)
//   3  _foreach_lerp_(m, g, w)                 diff = g - m                    rounded on its own, both branches
//        |w| <  0.5                            m = fma(w, diff, m)             ONE rounding (two: 118,507 differ)
//        |w| >= 0.5                            m = fma(-diff, 1.0f - w, g)     ONE rounding, 1 - w formed in fp32; w = 0.5 is here
//   4  _foreach_mul_(v, beta2)                 v = v * float(beta2)
//   5  _foreach_addcmul_(v, g, g, value)       v = fma(float(value), g * g, v) g * g rounded on its own, then ONE rounding
//   6  _foreach_sqrt(v)                        d = sqrt(v)                     correctly rounded
//   7  _foreach_div_(d, [bc2_sqrt])            d = d / float(bc2_sqrt)         a TRUE division (reciprocal-multiply: 146,929 differ)
//   8  _foreach_add_(d, eps)                   d = d + float(eps)
//   9  _foreach_addcdiv_(p, m, d, [step_size]) p = fma(float(step_size), m / d, p)   m / d a true division rounded on its own, then ONE
//                                                                              rounding (two: 41,508 differ; reciprocal: 22,607)
// Denormals: PyTorch's kernels keep them in every op above (1e-20 squared arrives in exp_avg_sq as 9.9e-44) and so does this
// unit, which is built without any flush-to-zero flag; sqrtf and `/` are the correctly rounded ones the compiler emits by default.
// Every line of the chain below is therefore either an explicit __builtin_fmaf or a single operation under
// `#pragma clang fp contract(off)`.
//
// The per-step scalars. PyTorch forms 1 - beta**t, lr / bc1 and bc2 ** 0.5 in Python doubles on the host, from a step count the
// host knows. Here the count is a device fact (a step the loss scaler skips must not count, and a captured replay knows nothing
// about the host), so `adam_prepare_kernel`, one thread per item in front of the step, advances the item's step word and writes
// its eight fp32 words from the group's fp64 block {lr, beta1, beta2, eps, weight_decay} with the device's fp64 pow / sqrt / div,
// each expression with its own roundings (no contraction) and one cast at the end. The fp64 pow is not promised to be correctly
// rounded; a disagreement with the host needs an fp64 error that straddles an fp32 rounding boundary, and the test of this kernel
// asks for equal bits over t in {1 .. 20000}.
//
// Under a loss scale g * inv_scale, and under clipping g * coef after it, are roundings of their own in front of the chain, as
// in optim.hip. *found_inf set: neither kernel touches anything.
#include "optim.h"

namespace yolo {

constexpr int ADAM_WORDS = 8;            // fp32 words per item, 32 bytes: two 16-byte loads
// word:  0 float(1 - lr*wd)   1 float(1 - beta1)   2 float(beta2)   3 float(1 - beta2)   4 float(eps)
//        5 float(sqrt(1 - beta2**t))   6 float((lr / (1 - beta1**t)) * -1)   7 float(wd)

__global__ __launch_bounds__(256) void adam_prepare_kernel(const SgdItem* __restrict__ items, int n_items, const double* __restrict__ hyper,
                                                           int* __restrict__ steps, float* __restrict__ words,
                                                           const float* __restrict__ found_inf) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    if (found_inf != nullptr && *found_inf != 0.f) return;
    if (items[i].g == nullptr) return;                   // no gradient this step: skipped, and its count does not move
    const int t = steps[i] + 1;
    steps[i] = t;
    const double lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], wd = hyper[4];
    const double bc1 = 1.0 - pow(beta1, (double)t);
    const double bc2 = 1.0 - pow(beta2, (double)t);
    float* __restrict__ w = words + (size_t)i * ADAM_WORDS;
    w[0] = (float)(1.0 - lr * wd);
    w[1] = (float)(1.0 - beta1);
    w[2] = (float)beta2;
    w[3] = (float)(1.0 - beta2);
    w[4] = (float)eps;
    w[5] = (float)sqrt(bc2);
    w[6] = (float)((lr / bc1) * -1.0);
    w[7] = (float)wd;
}

struct AdamWords { float decay, w, omw, beta2, value, eps, bc2_sqrt, step_size, wd; bool small; };

// EMA: ema (the shadow of p) moves towards the NEW p with the coefficients {ema_d, ema_omd}
// CLIP: g * coef directly after the unscale, a rounding of its own like it, applied whatever coef is
template <bool VEC, bool EMA, bool CLIP>
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            long long i0, int cnt, const AdamWords& k, int decoupled, int maximize, float inv_scale,
                                            float coef, float* __restrict__ ema, float ema_d, float ema_omd) {
    // The options are uniform over the launch; as selects instead of branches they leave each element a straight line, so the
    // compiler interleaves the four division / square-root chains of a float4.
    const unsigned flip = maximize ? 0x80000000u : 0u;
    const bool couple = !decoupled && k.wd != 0.f;
    const float decay = decoupled ? k.decay : 1.0f;          // times 1.0f is the identity (also for wd == 0 under AdamW)
    auto one = [&](float pv, float gv, float mv, float vv, float& pn, float& mn, float& vn) {
#pragma clang fp contract(off)
        gv = gv * inv_scale;                             // the unscale pass: a rounding of its own (times 1.0f: the identity)
        if (CLIP) gv = gv * coef;
        gv = __uint_as_float(__float_as_uint(gv) ^ flip);                    // 1
        const float coupled = __builtin_fmaf(k.wd, pv, gv);                  // 2b
        gv = couple ? coupled : gv;
        pv = pv * decay;                                                     // 2a
        const float diff = gv - mv;                                          // 3
        const float lo = __builtin_fmaf(k.w, diff, mv), hi = __builtin_fmaf(-diff, k.omw, gv);
        mn = k.small ? lo : hi;
        const float vb = vv * k.beta2;                                       // 4
        const float gg = gv * gv;
        vn = __builtin_fmaf(k.value, gg, vb);                                // 5
        float d = sqrtf(vn);                                                 // 6
        d = d / k.bc2_sqrt;                                                  // 7
        d = d + k.eps;                                                       // 8
        const float q = mn / d;
        pn = __builtin_fmaf(k.step_size, q, pv);                             // 9
    };
    if (VEC) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0), gv = *reinterpret_cast<const f32x4*>(g + i0);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(m + i0), vv = *reinterpret_cast<const f32x4*>(v + i0);
        f32x4 pn, mn, vn;
#pragma unroll
        for (int e = 0; e < 4; ++e) { float a, b, c; one(pv[e], gv[e], mv[e], vv[e], a, b, c); pn[e] = a; mn[e] = b; vn[e] = c; }
        *reinterpret_cast<f32x4*>(p + i0) = pn;
        *reinterpret_cast<f32x4*>(m + i0) = mn;
        *reinterpret_cast<f32x4*>(v + i0) = vn;
        if (EMA) {
            f32x4 ev = *reinterpret_cast<const f32x4*>(ema + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) ev[e] = ema_one(ev[e], pn[e], ema_d, ema_omd);
            *reinterpret_cast<f32x4*>(ema + i0) = ev;
        }
    } else {
        for (int e = 0; e < cnt; ++e) {
            float pn, mn, vn;
            one(p[i0 + e], g[i0 + e], m[i0 + e], v[i0 + e], pn, mn, vn);
            p[i0 + e] = pn;
            m[i0 + e] = mn;
            v[i0 + e] = vn;
            if (EMA) ema[i0 + e] = ema_one(ema[i0 + e], pn, ema_d, ema_omd);
        }
    }
}

// items: n_items SgdItem rows {p, g, exp_avg, n} (what the clip launches read), then n_items float* (exp_avg_sq of each item).
// Every option is a pointer that may be NULL: found_inf (set: nothing is touched), grad_scale (unscale in registers), clip (CLIP
// says whether it is given), shadows + state (EMA says whether they are given; a NULL entry of shadows: plain update).
template <bool EMA, bool CLIP>
__global__ __launch_bounds__(256) void adam_step_kernel(const SgdItem* __restrict__ items, int n_items, const int2* __restrict__ chunks,
                                                        const float* __restrict__ words, const float* __restrict__ grad_scale,
                                                        const float* __restrict__ found_inf, const ClipState* __restrict__ clip,
                                                        float* const* __restrict__ shadows, const EmaState* __restrict__ state,
                                                        int decoupled, int maximize) {
    if (found_inf != nullptr && *found_inf != 0.f) return;
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) return;                         // parameter without a gradient this step: skipped, like PyTorch
    float* const v = reinterpret_cast<float* const*>(items + n_items)[ck.x];
    const f32x4 wa = *reinterpret_cast<const f32x4*>(words + (size_t)ck.x * ADAM_WORDS);
    const f32x4 wb = *reinterpret_cast<const f32x4*>(words + (size_t)ck.x * ADAM_WORDS + 4);
    AdamWords k;
    k.decay = wa[0]; k.w = wa[1]; k.beta2 = wa[2]; k.value = wa[3]; k.eps = wb[0]; k.bc2_sqrt = wb[1]; k.step_size = wb[2]; k.wd = wb[3];
    k.omw = 1.0f - k.w;
    k.small = __builtin_fabsf(k.w) < 0.5f;
    const float inv_scale = grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    const float coef = CLIP ? clip->coef : 1.0f;
    const long long n = it.n < 0 ? -it.n : it.n;
    float* ema = nullptr;
    float d = 0.f, e_omd = 0.f;
    if (EMA) {
        ema = shadows[ck.x];
        ema_coeffs(state, d, e_omd);
    }
    const bool aligned = ((((size_t)it.p) | ((size_t)it.g) | ((size_t)it.buf) | ((size_t)v) | ((size_t)ema)) & 15) == 0;
    for_each_quad(ck, n, aligned, [&](long long i0, int cnt, bool vec) {
        if (EMA && ema != nullptr) {
            if (vec) adam_update<true, true, CLIP>(it.p, it.g, it.buf, v, i0, 4, k, decoupled, maximize, inv_scale, coef, ema, d, e_omd);
            else adam_update<false, true, CLIP>(it.p, it.g, it.buf, v, i0, cnt, k, decoupled, maximize, inv_scale, coef, ema, d, e_omd);
        } else {
            if (vec) adam_update<true, false, CLIP>(it.p, it.g, it.buf, v, i0, 4, k, decoupled, maximize, inv_scale, coef, nullptr, 0.f, 0.f);
            else adam_update<false, false, CLIP>(it.p, it.g, it.buf, v, i0, cnt, k, decoupled, maximize, inv_scale, coef, nullptr, 0.f, 0.f);
        }
    });
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_adam_prepare(const void* items_dev, int n_items, const double* hyper5_dev, int32_t* steps_dev, float* words_dev,
                      const float* found_inf_dev, void* stream) {
    if (n_items < 0) return fail(YOLO_ERR_ARG, "adam_prepare: bad arguments");
    if (n_items == 0) return YOLO_OK;
    if (!items_dev || !hyper5_dev || !steps_dev || !words_dev || ((size_t)hyper5_dev & 7) || ((size_t)words_dev & 15))
        return fail(YOLO_ERR_ARG, "adam_prepare: bad arguments");
    hipLaunchKernelGGL(adam_prepare_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const SgdItem*)items_dev, n_items, hyper5_dev, (int*)steps_dev, words_dev, found_inf_dev);
    return check_launch("adam_prepare");
}

int yolo_adam_step(const void* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, const float* words_dev,
                   const float* grad_scale_dev, const float* found_inf_dev, const void* clip_state_dev, const void* shadows_dev,
                   const void* ema_state_dev, int decoupled, int maximize, void* stream) {
    if (n_chunks < 0 || n_items < 0) return fail(YOLO_ERR_ARG, "adam_step: bad arguments");
    if (n_chunks == 0 || n_items == 0) return YOLO_OK;
    if (!items_dev || !chunks_dev || !words_dev || ((size_t)words_dev & 15) || ((size_t)clip_state_dev & 15) ||
        (!shadows_dev != !ema_state_dev) || ((size_t)ema_state_dev & 15))
        return fail(YOLO_ERR_ARG, "adam_step: bad arguments");
    const dim3 grid((unsigned)n_chunks), block(256);
    hipStream_t st = (hipStream_t)stream;
#define ADAM_LAUNCH(EMA, CLIP)                                                                                                          \
    hipLaunchKernelGGL((adam_step_kernel<EMA, CLIP>), grid, block, 0, st, (const SgdItem*)items_dev, n_items, (const int2*)chunks_dev, \
                       words_dev, grad_scale_dev, found_inf_dev, (const ClipState*)clip_state_dev, (float* const*)shadows_dev,        \
                       (const EmaState*)ema_state_dev, decoupled, maximize)
    if (shadows_dev) { if (clip_state_dev) ADAM_LAUNCH(true, true); else ADAM_LAUNCH(true, false); }
    else { if (clip_state_dev) ADAM_LAUNCH(false, true); else ADAM_LAUNCH(false, false); }
#undef ADAM_LAUNCH
    return check_launch("adam_step");
}

}  // extern "C"
