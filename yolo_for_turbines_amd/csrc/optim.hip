// optim.hip — the SGD update of the fine-tune step as ONE launch over every parameter.
//
// Replaces `optimizer.step()` of `torch.optim.SGD(model.parameters(), lr, momentum, weight_decay)` (reference:
// code/train.py:171-172 constructs it, :68 steps it through the GradScaler). PyTorch's default (foreach) implementation
// walks the 222 parameter tensors of the network in four multi-tensor passes (weight decay, momentum scale, momentum add,
// parameter update): ~19 launches and 0.66 ms of the 18.7 ms bf16 step at batch 32. Here a block owns a 4,096-element chunk
// of one tensor and does the whole update in registers: p, g and the momentum buffer are read once, p and the buffer written
// once (62 M parameters x 20 bytes = 1.2 GB per step).
//
// Same bits as PyTorch: each of its passes computes `a + alpha * b` with ONE rounding (a fused multiply-add in its
// elementwise functor), so the chain below is fmaf / mul in exactly that order:
//   g' = fma(wd, p, g)                     grad.add(param, alpha=weight_decay)
//   b  = first ? g' : fma(1 - dampening, g', b * momentum)      buf.mul_(momentum).add_(grad, alpha=1 - dampening)
//   g" = nesterov ? fma(momentum, b, g') : b
//   p  = fma(-lr, g", p)                   param.add_(grad, alpha=-lr)
//
// fp16 loss scaling (torch.amp.GradScaler, train.py:39,67-69) without a host wait: `sgd_check_finite_kernel` reads every
// gradient once and raises a device word; `sgd_step_kernel` reads that word and the scale, returns untouched when the
// word is set, and otherwise unscales in registers (g * inv_scale, rounded on its own like the separate unscale pass of
// `_amp_foreach_non_finite_check_and_unscale_`) in front of the chain above. The gradient is not written back.
//
// Weight average (EMA of every parameter and BatchNorm statistic; `ema.py`). The step holds the new parameter value in a
// register when it stores it, so its EMA instantiations move the average in the same launch: one more
// read and one more write per element, 28 bytes where the plain step moves 20. What the optimizer does not own (running
// statistics, parameters without a gradient, the integer counters) goes through `ema_update_kernel`, one launch over a table
// of (src, dst, n) rows. The arithmetic, with t = the number of updates applied so far (a device word, read when the
// kernel runs, so a captured launch follows the warm-up through its replays):
//   d   = warmup ? min(decay, float(1 + t) / float(10 + t)) : decay        a correctly rounded fp32 division
//   e   = fma(1 - d, p, e * d)                                             e.mul_(d).add_(p, alpha=1 - d)
// t is advanced by a one-thread launch AFTER every entry has been updated (a later block must still see the old t), and -
// like everything else - left alone when *found_inf is set: the average counts applied steps.
#include "optim.h"

namespace yolo {

struct EmaItem { const void* src; void* dst; long long n; };             // n < 0: copy -n 32-bit words (integer entries)
static_assert(sizeof(EmaItem) == 24, "matches yolo_ema_item in the header");

// EMA: ema (the shadow of p) moves towards the NEW p with the coefficients {ema_d, ema_omd}
// CLIP: g * coef directly after the unscale, a rounding of its own like it (the grad.mul_(clip_coef) pass of clip_grad_norm_),
// applied whatever coef is
template <bool VEC, bool EMA = false, bool CLIP = false>
__device__ __forceinline__ void sgd_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ b, long long i0,
                                           int cnt, bool first, float neg_lr, float momentum, float omd, float wd, int nesterov,
                                           int maximize, float inv_scale = 1.0f, float* __restrict__ ema = nullptr, float ema_d = 0.f,
                                           float ema_omd = 0.f, float coef = 1.0f) {
    auto one = [&](float pv, float gv, float bv, float& pn, float& bn) {
        if (inv_scale != 1.0f) {                         // the unscale pass: a rounding of its own, never fused into what follows
#pragma clang fp contract(off)
            gv = gv * inv_scale;
        }
        if (CLIP) {
#pragma clang fp contract(off)
            gv = gv * coef;
        }
        if (maximize) gv = -gv;
        if (wd != 0.f) gv = __builtin_fmaf(wd, pv, gv);
        if (momentum != 0.f) {
            bn = first ? gv : __builtin_fmaf(omd, gv, bv * momentum);
            gv = nesterov ? __builtin_fmaf(momentum, bn, gv) : bn;
        } else {
            bn = bv;
        }
        pn = __builtin_fmaf(neg_lr, gv, pv);
    };
    if (VEC) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0), gv = *reinterpret_cast<const f32x4*>(g + i0);
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (momentum != 0.f && !first) bv = *reinterpret_cast<const f32x4*>(b + i0);
        f32x4 pn, bn;
#pragma unroll
        for (int e = 0; e < 4; ++e) { float a, c; one(pv[e], gv[e], bv[e], a, c); pn[e] = a; bn[e] = c; }
        *reinterpret_cast<f32x4*>(p + i0) = pn;
        if (momentum != 0.f) *reinterpret_cast<f32x4*>(b + i0) = bn;
        if (EMA) {
            f32x4 ev = *reinterpret_cast<const f32x4*>(ema + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) ev[e] = ema_one(ev[e], pn[e], ema_d, ema_omd);
            *reinterpret_cast<f32x4*>(ema + i0) = ev;
        }
    } else {
        for (int e = 0; e < cnt; ++e) {
            float pn, bn;
            one(p[i0 + e], g[i0 + e], (momentum != 0.f && !first) ? b[i0 + e] : 0.f, pn, bn);
            p[i0 + e] = pn;
            if (momentum != 0.f) b[i0 + e] = bn;
            if (EMA) ema[i0 + e] = ema_one(ema[i0 + e], pn, ema_d, ema_omd);
        }
    }
}

// The step. chunks[c] = (item index, first element): built once per optimizer (sizes never change), the items every step.
// hyper: {lr, momentum, dampening, weight_decay} in device memory, read at EXECUTION time, so a captured launch follows a
// learning-rate schedule (train.py:71-74 steps a LinearLR warm-up after every batch) instead of replaying the values of the
// capture. Every option is a pointer that may be NULL:
//   found_inf   set: every block returns without touching p, the momentum buffer or the average.
//   grad_scale  the loss scale: inv_scale is `scale.double().reciprocal().float()` of GradScaler.unscale_, applied in registers;
//               NULL: inv_scale = 1.0f, and sgd_update then has no unscale rounding at all.
//   written     who decides "first step" (buf = g', which ignores dampening): written[item] == 0 says the item's momentum buffer
//               has never been written - a device fact under a loss scale, where a skipped first step leaves it unwritten;
//               sgd_mark_written_kernel sets the word after a step that was applied, in a launch of its own (a later block of
//               the same item must still read the old value). NULL: the sign of n says it.
//   shadows + state (EMA says whether they are given): shadows[item] is the average of that item's parameter, moved in the same
//               launch (NULL entry: this parameter has none, plain update). An item without a gradient is skipped here like
//               everywhere; its average is the caller's business (ema_update_kernel).
//   clip (CLIP says whether it is given): coef is the word the finalize launch left in the clip state. CLIP is a template
//               parameter because g * coef is a rounding of its own that an unclipped step must not have.
template <bool EMA, bool CLIP>
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdItem* __restrict__ items, const int2* __restrict__ chunks,
                                                       const float* __restrict__ hyper, const ClipState* __restrict__ clip,
                                                       const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                       const int* __restrict__ written, float* const* __restrict__ shadows,
                                                       const EmaState* __restrict__ state, int nesterov, int maximize) {
    if (found_inf != nullptr && *found_inf != 0.f) return;
    const f32x4 h = *reinterpret_cast<const f32x4*>(hyper);
    const float neg_lr = -h[0], momentum = h[1], omd = 1.0f - h[2], wd = h[3];
    const float inv_scale = grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    const float coef = CLIP ? clip->coef : 1.0f;
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) return;                         // parameter without a gradient this step: skipped, like PyTorch
    const bool first = written != nullptr ? written[ck.x] == 0 : it.n < 0;
    const long long n = it.n < 0 ? -it.n : it.n;
    float* ema = nullptr;
    float d = 0.f, e_omd = 0.f;
    if (EMA) {
        ema = shadows[ck.x];
        ema_coeffs(state, d, e_omd);
    }
    const bool aligned = ((((size_t)it.p) | ((size_t)it.g) | ((size_t)it.buf) | ((size_t)ema)) & 15) == 0;
    for_each_quad(ck, n, aligned, [&](long long i0, int cnt, bool vec) {
        if (EMA && ema != nullptr) {
            if (vec) sgd_update<true, true, CLIP>(it.p, it.g, it.buf, i0, 4, first, neg_lr, momentum, omd, wd, nesterov, maximize, inv_scale, ema, d, e_omd, coef);
            else sgd_update<false, true, CLIP>(it.p, it.g, it.buf, i0, cnt, first, neg_lr, momentum, omd, wd, nesterov, maximize, inv_scale, ema, d, e_omd, coef);
        } else {
            if (vec) sgd_update<true, false, CLIP>(it.p, it.g, it.buf, i0, 4, first, neg_lr, momentum, omd, wd, nesterov, maximize, inv_scale, nullptr, 0.f, 0.f, coef);
            else sgd_update<false, false, CLIP>(it.p, it.g, it.buf, i0, cnt, first, neg_lr, momentum, omd, wd, nesterov, maximize, inv_scale, nullptr, 0.f, 0.f, coef);
        }
    });
}

// One block per chunk, as in the step. A value is non-finite when its exponent bits are all ones: an integer test, which no
// floating-point folding can remove. Writes nothing but *found_inf = 1.0f (every writer writes the same value: no atomics),
// one store per block that saw something; the word is cleared by a one-thread launch in front of this one (a kernel rather
// than a 4-byte memset: a captured memset node of that size was seen to replay with a stale fill pattern).
__global__ void sgd_clear_flag_kernel(float* __restrict__ found_inf) { *found_inf = 0.f; }

__global__ __launch_bounds__(256) void sgd_check_finite_kernel(const SgdItem* __restrict__ items, const int2* __restrict__ chunks,
                                                               float* __restrict__ found_inf) {
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) return;                         // uniform over the block
    constexpr unsigned EXP = 0x7f800000u;
    int bad = 0;
    scan_grad_chunk(reinterpret_cast<const unsigned*>(it.g), ck, it.n < 0 ? -it.n : it.n, [&](unsigned bits) { bad |= (bits & EXP) == EXP; });
    if (__syncthreads_or(bad) && threadIdx.x == 0) *found_inf = 1.0f;
}

// One thread per item, after the step: the buffer of every item that had a gradient has now been written, unless the
// step was skipped.
__global__ __launch_bounds__(256) void sgd_mark_written_kernel(const SgdItem* __restrict__ items, int n_items,
                                                               const float* __restrict__ found_inf, int* __restrict__ written) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items || *found_inf != 0.f) return;
    if (items[i].g != nullptr) written[i] = 1;
}

// The average on its own: chunks[c] = (row, first element) as for the step. found_inf may be NULL (no loss scale).
__global__ __launch_bounds__(256) void ema_update_kernel(const EmaItem* __restrict__ items, const int2* __restrict__ chunks,
                                                         const EmaState* __restrict__ state, const float* __restrict__ found_inf) {
    if (found_inf != nullptr && *found_inf != 0.f) return;
    const int2 ck = chunks[blockIdx.x];
    const EmaItem it = items[ck.x];
    if (it.n < 0) {                                      // integer entry: copied word by word (a handful of words in all)
        const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(it.src);
        unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(it.dst);
        const long long n = -it.n;
        for (long long i = (long long)ck.y + threadIdx.x; i < n && i < (long long)ck.y + SGD_CHUNK; i += 256) dst[i] = src[i];
        return;
    }
    const float* __restrict__ p = reinterpret_cast<const float*>(it.src);
    float* __restrict__ e = reinterpret_cast<float*>(it.dst);
    float d, omd;
    ema_coeffs(state, d, omd);
    const bool aligned = ((((size_t)p) | ((size_t)e)) & 15) == 0;
    for_each_quad(ck, it.n, aligned, [&](long long i0, int cnt, bool vec) {
        if (vec) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i0);
            f32x4 ev = *reinterpret_cast<const f32x4*>(e + i0);
#pragma unroll
            for (int k = 0; k < 4; ++k) ev[k] = ema_one(ev[k], pv[k], d, omd);
            *reinterpret_cast<f32x4*>(e + i0) = ev;
        } else {
            for (int k = 0; k < cnt; ++k) e[i0 + k] = ema_one(e[i0 + k], p[i0 + k], d, omd);
        }
    });
}

// One thread, after every entry has been updated: an applied update counts.
__global__ void ema_advance_kernel(EmaState* __restrict__ state, const float* __restrict__ found_inf) {
    if (found_inf != nullptr && *found_inf != 0.f) return;
    state->updates += 1;
}

// ---- gradient clipping by global norm (torch.nn.utils.clip_grad_norm_ between the unscale and the step) ----
// The norm is a reduction over the chunk table, the coefficient a device word, the clip one more multiply in sgd_update.
//   partials: one block per chunk, each element unscaled in fp32 like the step does it, squared and summed in fp64 (the square of
//             3e19 overflows fp32 and the square of 1e-30 vanishes in it; 6.2e7 fp64 terms err by 7e-9 relative), per thread in
//             a fixed order, then over the block in a fixed tree: one double per chunk in a slot that chunk owns, no atomics,
//             the same bits every run. CHECK: the non-finite test of sgd_check_finite_kernel from the same registers, so a
//             loss-scaled step reads its gradients once for both. INF: the largest |g| in place of the sum, NaN-propagating.
//   finalize: one block over every group's partials in a fixed order, sqrt, one rounding to fp32, then
//             coef = min(fl(fl(1 / fl(total + 1e-6f)) * max_norm), 1): torch turns `max_norm / tensor` into reciprocal() * max_norm.
template <bool INF>
__device__ __forceinline__ double clip_combine(double a, double b) {
    if (INF) return (b != b || b > a) ? b : a;           // a NaN on either side stays
    return a + b;
}

// every thread's value -> thread 0, in the same order every run: down the wave, then the waves left to right
template <bool INF, int WAVES>
__device__ __forceinline__ double clip_block_reduce(double acc) {
    __shared__ double per_wave[WAVES];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = clip_combine<INF>(acc, __shfl_down(acc, off));
    if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    double all = per_wave[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) all = clip_combine<INF>(all, per_wave[w]);
    return all;
}

template <bool CHECK, bool INF>
__global__ __launch_bounds__(256) void clip_norm_partials_kernel(const SgdItem* __restrict__ items, const int2* __restrict__ chunks,
                                                                 const float* __restrict__ grad_scale, double* __restrict__ partials,
                                                                 float* __restrict__ found_inf) {
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) {                               // uniform over the block; the slot is still this chunk's to write
        if (threadIdx.x == 0) partials[blockIdx.x] = 0.0;
        return;
    }
    const float inv_scale = grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    constexpr unsigned EXP = 0x7f800000u;
    int bad = 0;
    double acc = 0.0;
    scan_grad_chunk(reinterpret_cast<const unsigned*>(it.g), ck, it.n < 0 ? -it.n : it.n, [&](unsigned bits) {
        if (CHECK) bad |= (bits & EXP) == EXP;           // on the value as it lies in memory, like the check launch
        float v = __uint_as_float(bits);
        if (inv_scale != 1.0f) {
#pragma clang fp contract(off)
            v = v * inv_scale;
        }
        if (INF) acc = clip_combine<true>(acc, (double)__builtin_fabsf(v));
        else { const double d = (double)v; acc = __builtin_fma(d, d, acc); }
    });
    const double sum = clip_block_reduce<INF, 4>(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
    if (CHECK) {
        if (__syncthreads_or(bad) && threadIdx.x == 0) *found_inf = 1.0f;
    }
}

// One block of FIN_THREADS. A thread takes partials t, t + FIN_THREADS, ... in that order, FIN_BATCH independent loads in flight
// at a time (one dependent load after the other made this launch cost as much as the pass over the gradients). Past the end a
// thread adds 0, the identity of both the sum of squares and the maximum of magnitudes.
constexpr int FIN_THREADS = 1024, FIN_BATCH = 8;

template <bool INF>
__global__ __launch_bounds__(FIN_THREADS) void clip_finalize_kernel(const double* __restrict__ partials, int n, ClipState* __restrict__ state) {
    double acc = 0.0;
    for (int i0 = 0; i0 < n; i0 += FIN_THREADS * FIN_BATCH) {
        double v[FIN_BATCH];
#pragma unroll
        for (int k = 0; k < FIN_BATCH; ++k) {
            const int i = i0 + k * FIN_THREADS + (int)threadIdx.x;
            v[k] = i < n ? partials[i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < FIN_BATCH; ++k) acc = clip_combine<INF>(acc, v[k]);
    }
    const double all = clip_block_reduce<INF, FIN_THREADS / 64>(acc);
    if (threadIdx.x != 0) return;
    const float total = (float)(INF ? all : __builtin_sqrt(all));
    const float max_norm = state->max_norm;              // read when the kernel runs: a captured step follows a changed value
    const float recip = 1.0f / (total + 1e-6f);          // correctly rounded; the product below is rounded on its own
    const float scaled = recip * max_norm;
    state->total_norm = total;
    state->coef = scaled > 1.0f ? 1.0f : scaled;         // clamp(max=1): a NaN stays a NaN
    state->norm_type = INF ? 1 : 0;
}

// g *= coef in place over a chunk table (clip_grad_norm_ for other optimizers): the item's p and buf are not looked at
__global__ __launch_bounds__(256) void clip_scale_grads_kernel(const SgdItem* __restrict__ items, const int2* __restrict__ chunks,
                                                               const ClipState* __restrict__ clip) {
    const float coef = clip->coef;
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) return;
    const long long n = it.n < 0 ? -it.n : it.n;
    float* __restrict__ g = const_cast<float*>(it.g);
    for_each_quad(ck, n, (((size_t)g) & 15) == 0, [&](long long i0, int cnt, bool vec) {
        if (vec) {
            f32x4 v = *reinterpret_cast<const f32x4*>(g + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] * coef;
            *reinterpret_cast<f32x4*>(g + i0) = v;
        } else {
            for (int e = 0; e < cnt; ++e) g[i0 + e] = g[i0 + e] * coef;
        }
    });
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_sgd_chunk_elems(void) { return SGD_CHUNK; }

int yolo_sgd_step(const void* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, const float* hyper4_dev,
                  const void* clip_state_dev, const float* grad_scale_dev, const float* found_inf_dev, int32_t* written_dev,
                  const void* shadows_dev, const void* ema_state_dev, int nesterov, int maximize, void* stream) {
    if (((size_t)clip_state_dev & 15) || n_chunks < 0 || n_items < 0) return fail(YOLO_ERR_ARG, "sgd_step: bad arguments");
    if (n_chunks == 0 || n_items == 0) return YOLO_OK;
    // the "written" words are advanced by a launch that reads *found_inf; the average needs its table and its state together
    if (!items_dev || !chunks_dev || !hyper4_dev || ((size_t)hyper4_dev & 15) || (written_dev && !found_inf_dev) ||
        (!shadows_dev != !ema_state_dev) || ((size_t)ema_state_dev & 15))
        return fail(YOLO_ERR_ARG, "sgd_step: bad arguments");
    const dim3 grid((unsigned)n_chunks), block(256);
    hipStream_t st = (hipStream_t)stream;
#define SGD_LAUNCH(EMA, CLIP)                                                                                                          \
    hipLaunchKernelGGL((sgd_step_kernel<EMA, CLIP>), grid, block, 0, st, (const SgdItem*)items_dev, (const int2*)chunks_dev, hyper4_dev, \
                       (const ClipState*)clip_state_dev, grad_scale_dev, found_inf_dev, (const int*)written_dev,                        \
                       (float* const*)shadows_dev, (const EmaState*)ema_state_dev, nesterov, maximize)
    if (shadows_dev) { if (clip_state_dev) SGD_LAUNCH(true, true); else SGD_LAUNCH(true, false); }
    else { if (clip_state_dev) SGD_LAUNCH(false, true); else SGD_LAUNCH(false, false); }
#undef SGD_LAUNCH
    if (written_dev)
        hipLaunchKernelGGL(sgd_mark_written_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, (const SgdItem*)items_dev, n_items,
                           found_inf_dev, (int*)written_dev);
    return check_launch("sgd_step");
}

int yolo_sgd_check_finite(const void* items_dev, const int32_t* chunks_dev, int n_chunks, float* found_inf_dev, int clear, void* stream) {
    if (!found_inf_dev || n_chunks < 0 || (n_chunks > 0 && (!items_dev || !chunks_dev))) return fail(YOLO_ERR_ARG, "sgd_check_finite: bad arguments");
    if (clear) hipLaunchKernelGGL(sgd_clear_flag_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, found_inf_dev);
    if (n_chunks == 0) return YOLO_OK;
    hipLaunchKernelGGL(sgd_check_finite_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const SgdItem*)items_dev,
                       (const int2*)chunks_dev, found_inf_dev);
    return check_launch("sgd_check_finite");
}

int yolo_ema_update(const void* items_dev, const int32_t* chunks_dev, int n_chunks, void* ema_state_dev, const float* found_inf_dev,
                    int advance, void* stream) {
    if (!ema_state_dev || ((size_t)ema_state_dev & 15) || n_chunks < 0 || (n_chunks > 0 && (!items_dev || !chunks_dev)))
        return fail(YOLO_ERR_ARG, "ema_update: bad arguments");
    if (n_chunks > 0)
        hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const EmaItem*)items_dev,
                           (const int2*)chunks_dev, (const EmaState*)ema_state_dev, found_inf_dev);
    if (advance) hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (EmaState*)ema_state_dev, found_inf_dev);
    return check_launch("ema_update");
}

static bool clip_norm_known(int norm_type) { return norm_type == YOLO_NORM_L2 || norm_type == YOLO_NORM_INF; }

int yolo_clip_norm_partials(const void* items_dev, const int32_t* chunks_dev, int n_chunks, const float* grad_scale_dev, int norm_type,
                            double* partials_dev, float* found_inf_dev, int clear, void* stream) {
    if (n_chunks < 0 || !clip_norm_known(norm_type) || (n_chunks > 0 && (!items_dev || !chunks_dev || !partials_dev)) ||
        ((size_t)partials_dev & 7))
        return fail(YOLO_ERR_ARG, "clip_norm_partials: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (found_inf_dev && clear) hipLaunchKernelGGL(sgd_clear_flag_kernel, dim3(1), dim3(1), 0, st, found_inf_dev);
    if (n_chunks == 0) return check_launch("clip_norm_partials");
    const SgdItem* items = (const SgdItem*)items_dev;
    const int2* chunks = (const int2*)chunks_dev;
    const dim3 grid((unsigned)n_chunks), block(256);
    const bool inf = norm_type == YOLO_NORM_INF;
    if (found_inf_dev) {
        if (inf) hipLaunchKernelGGL((clip_norm_partials_kernel<true, true>), grid, block, 0, st, items, chunks, grad_scale_dev, partials_dev, found_inf_dev);
        else hipLaunchKernelGGL((clip_norm_partials_kernel<true, false>), grid, block, 0, st, items, chunks, grad_scale_dev, partials_dev, found_inf_dev);
    } else {
        if (inf) hipLaunchKernelGGL((clip_norm_partials_kernel<false, true>), grid, block, 0, st, items, chunks, grad_scale_dev, partials_dev, found_inf_dev);
        else hipLaunchKernelGGL((clip_norm_partials_kernel<false, false>), grid, block, 0, st, items, chunks, grad_scale_dev, partials_dev, found_inf_dev);
    }
    return check_launch("clip_norm_partials");
}

int yolo_clip_finalize(const double* partials_dev, int n_partials, int norm_type, void* clip_state_dev, void* stream) {
    if (!clip_state_dev || ((size_t)clip_state_dev & 15) || n_partials < 0 || !clip_norm_known(norm_type) || (n_partials > 0 && !partials_dev) ||
        ((size_t)partials_dev & 7))
        return fail(YOLO_ERR_ARG, "clip_finalize: bad arguments");
    if (norm_type == YOLO_NORM_INF)
        hipLaunchKernelGGL(clip_finalize_kernel<true>, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, partials_dev, n_partials, (ClipState*)clip_state_dev);
    else
        hipLaunchKernelGGL(clip_finalize_kernel<false>, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, partials_dev, n_partials, (ClipState*)clip_state_dev);
    return check_launch("clip_finalize");
}

int yolo_clip_scale_grads(const void* items_dev, const int32_t* chunks_dev, int n_chunks, const void* clip_state_dev, void* stream) {
    if (!clip_state_dev || ((size_t)clip_state_dev & 15) || n_chunks < 0 || (n_chunks > 0 && (!items_dev || !chunks_dev)))
        return fail(YOLO_ERR_ARG, "clip_scale_grads: bad arguments");
    if (n_chunks == 0) return YOLO_OK;
    hipLaunchKernelGGL(clip_scale_grads_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const SgdItem*)items_dev,
                       (const int2*)chunks_dev, (const ClipState*)clip_state_dev);
    return check_launch("clip_scale_grads");
}

}  // extern "C"
