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
// gradient once and raises a device word; `sgd_step_amp_kernel` reads that word and the scale, returns untouched when the
// word is set, and otherwise unscales in registers (g * inv_scale, rounded on its own like the separate unscale pass of
// `_amp_foreach_non_finite_check_and_unscale_`) in front of the chain above. The gradient is not written back.
#include "common.h"

namespace yolo {

struct SgdItem { float* p; const float* g; float* buf; long long n; };   // n < 0: the momentum buffer is new (first step): buf = g'
static_assert(sizeof(SgdItem) == 32, "matches yolo_sgd_item in the header");

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int SGD_CHUNK = 4096;          // elements per block: 256 threads x 4 x float4

template <bool VEC>
__device__ __forceinline__ void sgd_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ b, long long i0,
                                           int cnt, bool first, float neg_lr, float momentum, float omd, float wd, int nesterov,
                                           int maximize, float inv_scale = 1.0f) {
    auto one = [&](float pv, float gv, float bv, float& pn, float& bn) {
        if (inv_scale != 1.0f) {                         // the unscale pass: a rounding of its own, never fused into what follows
#pragma clang fp contract(off)
            gv = gv * inv_scale;
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
    } else {
        for (int e = 0; e < cnt; ++e) {
            float pn, bn;
            one(p[i0 + e], g[i0 + e], (momentum != 0.f && !first) ? b[i0 + e] : 0.f, pn, bn);
            p[i0 + e] = pn;
            if (momentum != 0.f) b[i0 + e] = bn;
        }
    }
}

// chunks[c] = (item index, first element): built once per optimizer (sizes never change), the items every step.
// hyper != nullptr: {lr, momentum, dampening, weight_decay} are read from device memory at EXECUTION time, so a captured
// launch follows a learning-rate schedule (train.py:71-74 steps a LinearLR warm-up after every batch) instead of replaying
// the values of the capture; the by-value arguments are then ignored.
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdItem* __restrict__ items, const int2* __restrict__ chunks,
                                                       const float* __restrict__ hyper, float neg_lr, float momentum, float omd, float wd,
                                                       int nesterov, int maximize) {
    if (hyper != nullptr) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(hyper);
        neg_lr = -h[0]; momentum = h[1]; omd = 1.0f - h[2]; wd = h[3];
    }
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) return;                         // parameter without a gradient this step: skipped, like PyTorch
    const bool first = it.n < 0;
    const long long n = first ? -it.n : it.n;
    const bool aligned = ((((size_t)it.p) | ((size_t)it.g) | ((size_t)it.buf)) & 15) == 0;
#pragma unroll
    for (int r = 0; r < SGD_CHUNK / 1024; ++r) {
        const long long i0 = (long long)ck.y + r * 1024 + threadIdx.x * 4;
        if (i0 >= n) break;
        const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
        if (aligned && cnt == 4) sgd_update<true>(it.p, it.g, it.buf, i0, 4, first, neg_lr, momentum, omd, wd, nesterov, maximize);
        else sgd_update<false>(it.p, it.g, it.buf, i0, cnt, first, neg_lr, momentum, omd, wd, nesterov, maximize);
    }
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
    const long long n = it.n < 0 ? -it.n : it.n;
    const unsigned* __restrict__ g = reinterpret_cast<const unsigned*>(it.g);
    const bool aligned = (((size_t)g) & 15) == 0;
    constexpr unsigned EXP = 0x7f800000u;
    int bad = 0;
    const long long base = (long long)ck.y + threadIdx.x * 4;
    if (aligned && (long long)ck.y + SGD_CHUNK <= n) {   // full chunk: four independent 16-byte loads in flight
        u32x4 v[SGD_CHUNK / 1024];
#pragma unroll
        for (int r = 0; r < SGD_CHUNK / 1024; ++r) v[r] = *reinterpret_cast<const u32x4*>(g + base + r * 1024);
#pragma unroll
        for (int r = 0; r < SGD_CHUNK / 1024; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= (v[r][e] & EXP) == EXP;
    } else {
#pragma unroll
        for (int r = 0; r < SGD_CHUNK / 1024; ++r) {
            const long long i0 = base + r * 1024;
            if (i0 >= n) break;
            const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
            if (aligned && cnt == 4) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(g + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) bad |= (v[e] & EXP) == EXP;
            } else {
                for (int e = 0; e < cnt; ++e) bad |= (g[i0 + e] & EXP) == EXP;
            }
        }
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) *found_inf = 1.0f;
}

// The step under a loss scale. found_inf (device, never NULL): non-zero -> every block returns without touching p or the
// momentum buffer. grad_scale (device, may be NULL: the gradients are unscaled already): inv_scale is
// `scale.double().reciprocal().float()` of GradScaler.unscale_. written[item] == 0: this item's momentum buffer has never
// been written (buf = g', PyTorch's first applied step, which ignores dampening); sgd_mark_written_kernel sets it after a
// step that was applied, in a launch of its own (a later block of the same item must still read the old value).
__global__ __launch_bounds__(256) void sgd_step_amp_kernel(const SgdItem* __restrict__ items, const int2* __restrict__ chunks,
                                                           const float* __restrict__ hyper, const float* __restrict__ grad_scale,
                                                           const float* __restrict__ found_inf, const int* __restrict__ written,
                                                           int nesterov, int maximize) {
    if (*found_inf != 0.f) return;
    const f32x4 h = *reinterpret_cast<const f32x4*>(hyper);
    const float neg_lr = -h[0], momentum = h[1], omd = 1.0f - h[2], wd = h[3];
    const float inv_scale = grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.0f;
    const int2 ck = chunks[blockIdx.x];
    const SgdItem it = items[ck.x];
    if (it.g == nullptr) return;
    const bool first = written[ck.x] == 0;
    const long long n = it.n < 0 ? -it.n : it.n;
    const bool aligned = ((((size_t)it.p) | ((size_t)it.g) | ((size_t)it.buf)) & 15) == 0;
#pragma unroll
    for (int r = 0; r < SGD_CHUNK / 1024; ++r) {
        const long long i0 = (long long)ck.y + r * 1024 + threadIdx.x * 4;
        if (i0 >= n) break;
        const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
        if (aligned && cnt == 4) sgd_update<true>(it.p, it.g, it.buf, i0, 4, first, neg_lr, momentum, omd, wd, nesterov, maximize, inv_scale);
        else sgd_update<false>(it.p, it.g, it.buf, i0, cnt, first, neg_lr, momentum, omd, wd, nesterov, maximize, inv_scale);
    }
}

// One thread per item, after the step: the buffer of every item that had a gradient has now been written, unless the
// step was skipped.
__global__ __launch_bounds__(256) void sgd_mark_written_kernel(const SgdItem* __restrict__ items, int n_items,
                                                               const float* __restrict__ found_inf, int* __restrict__ written) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items || *found_inf != 0.f) return;
    if (items[i].g != nullptr) written[i] = 1;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_sgd_chunk_elems(void) { return SGD_CHUNK; }

int yolo_sgd_step(const void* items_dev, const int32_t* chunks_dev, int n_chunks, float lr, float momentum, float dampening,
                  float weight_decay, int nesterov, int maximize, void* stream) {
    if (n_chunks == 0) return YOLO_OK;
    if (!items_dev || !chunks_dev || n_chunks < 0) return fail(YOLO_ERR_ARG, "sgd_step: bad arguments");
    if (nesterov && (momentum <= 0.f || dampening != 0.f)) return fail(YOLO_ERR_ARG, "sgd_step: nesterov needs momentum > 0 and dampening = 0");
    hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const SgdItem*)items_dev,
                       (const int2*)chunks_dev, (const float*)nullptr, -lr, momentum, 1.0f - dampening, weight_decay, nesterov, maximize);
    return check_launch("sgd_step");
}

int yolo_sgd_step_hp(const void* items_dev, const int32_t* chunks_dev, int n_chunks, const float* hyper4_dev, int nesterov, int maximize,
                     void* stream) {
    if (n_chunks == 0) return YOLO_OK;
    if (!items_dev || !chunks_dev || !hyper4_dev || n_chunks < 0 || ((size_t)hyper4_dev & 15)) return fail(YOLO_ERR_ARG, "sgd_step_hp: bad arguments");
    hipLaunchKernelGGL(sgd_step_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const SgdItem*)items_dev,
                       (const int2*)chunks_dev, hyper4_dev, 0.f, 0.f, 1.f, 0.f, nesterov, maximize);
    return check_launch("sgd_step_hp");
}

int yolo_sgd_check_finite(const void* items_dev, const int32_t* chunks_dev, int n_chunks, float* found_inf_dev, int clear, void* stream) {
    if (!found_inf_dev || n_chunks < 0 || (n_chunks > 0 && (!items_dev || !chunks_dev))) return fail(YOLO_ERR_ARG, "sgd_check_finite: bad arguments");
    if (clear) hipLaunchKernelGGL(sgd_clear_flag_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, found_inf_dev);
    if (n_chunks == 0) return YOLO_OK;
    hipLaunchKernelGGL(sgd_check_finite_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const SgdItem*)items_dev,
                       (const int2*)chunks_dev, found_inf_dev);
    return check_launch("sgd_check_finite");
}

int yolo_sgd_step_amp(const void* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, const float* hyper4_dev,
                      const float* grad_scale_dev, const float* found_inf_dev, int32_t* written_dev, int nesterov, int maximize, void* stream) {
    if (n_chunks == 0 || n_items == 0) return YOLO_OK;
    if (!items_dev || !chunks_dev || !hyper4_dev || !found_inf_dev || !written_dev || n_chunks < 0 || n_items < 0 || ((size_t)hyper4_dev & 15))
        return fail(YOLO_ERR_ARG, "sgd_step_amp: bad arguments");
    hipLaunchKernelGGL(sgd_step_amp_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const SgdItem*)items_dev,
                       (const int2*)chunks_dev, hyper4_dev, grad_scale_dev, found_inf_dev, (const int*)written_dev, nesterov, maximize);
    hipLaunchKernelGGL(sgd_mark_written_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const SgdItem*)items_dev, n_items, found_inf_dev, (int*)written_dev);
    return check_launch("sgd_step_amp");
}

}  // extern "C"
