// anchors.hip — the anchors of a dataset: k-means++ seeding and Lloyd steps under the distance 1 - IoU(w, h), several restarts side by
// side, and the fitness of any anchor set (next to the hot path: the anchors rank every box in targets.hip, scale the decode and the
// loss). The contract (arithmetic, seeding rule, stop rule) is stated in include/yolo_mi355x.h; this file is written from it.
//
// Work split. A block owns kChunk = 2048 consecutive boxes; the grid is (blocks over boxes, restarts) and every restart has its
// own done-flag in the workspace, so a converged restart costs early-exit launches only. No floating-point atomics: a block
// reduces in a fixed order (lanes by xor butterfly or shuffle scan, waves through LDS in wave order) and writes its partial row to
// the workspace; one block per restart adds the rows in ascending block order (ordered_sum). Results are the same bits run to run.
//   seeding step j:  anchor_seed_sums (sum of d^2 per block)  ->  anchor_seed_pick (prefix over blocks, then over the boxes of the
//                    one block the draw falls into; d^2 is recomputed from the j chosen seeds, nothing of size n is stored)
//   Lloyd step:      anchor_assign (label, then sum w, sum h, count per cluster and block)  ->  anchor_update (new centroids, stop test)
//   fitness:         anchor_score (sum of best IoU per block, optionally wins / labels)  ->  anchor_*_final
// Built with -ffp-contract=off: the IoU is the expression of build_targets_kernel (targets.hip), every fp32 operation rounded once.
#include "common.h"

#include <climits>
#include <cstdint>

namespace yolo {

constexpr int kThreads = 256;
constexpr int kItems = 8;                        // boxes per thread
constexpr int kChunk = kThreads * kItems;        // boxes per block
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 16, kMaxRestarts = 64;
constexpr int kStage = 1536;                     // doubles of LDS that ordered_sum stages per round (32 rows of 3 * kMaxK)

__device__ __forceinline__ float wh_iou(float bw, float bh, float cw, float ch) {
    const float inter = fminf(bw, cw) * fminf(bh, ch);
    return inter / (bw * bh + cw * ch - inter);
}

// argmax_j IoU(b, c_j), the first maximum; c: k x 2 (wave-uniform address)
__device__ __forceinline__ int best_match(float w, float h, const float* __restrict__ c, int k, float& best) {
    int lab = 0;
    best = wh_iou(w, h, c[0], c[1]);
    for (int j = 1; j < k; ++j) {
        const float v = wh_iou(w, h, c[2 * j], c[2 * j + 1]);
        if (v > best) { best = v; lab = j; }
    }
    return lab;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// sum of v over the block, the same bits in every thread; s_w: kWaves doubles
__device__ __forceinline__ double block_sum(double v, double* s_w) {
    v = wave_sum(v);
    __syncthreads();                                       // s_w may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// prefix of v over the block's threads in thread order (inclusive, exclusive) and the block total (== incl of the last thread)
__device__ __forceinline__ void block_scan(double v, double* s_w, double& incl, double& excl, double& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double x = v;
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    double e = __shfl_up(x, 1);
    if (lane == 0) e = 0.0;
    __syncthreads();
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    double pre = 0.0;
    for (int q = 0; q < wave; ++q) pre += s_w[q];
    total = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    incl = pre + x;
    excl = pre + e;
}

// Thread t < width gets the sum over rows of tab[row][t], rows added in ascending order; tab: [rows][width] doubles, width <= 3 * kMaxK.
// The rows are staged through LDS (s_buf: kStage doubles) so that the sequential adds do not each wait for a global load.
__device__ __forceinline__ double ordered_sum(const double* __restrict__ tab, int rows, int width, double* s_buf) {
    const int per = kStage / width;
    double acc = 0.0;
    for (int r0 = 0; r0 < rows; r0 += per) {
        const int cnt = rows - r0 < per ? rows - r0 : per;
        for (int e = threadIdx.x; e < cnt * width; e += kThreads) s_buf[e] = tab[(size_t)r0 * width + e];
        __syncthreads();
        if ((int)threadIdx.x < width)
            for (int q = 0; q < cnt; ++q) acc += s_buf[q * width + threadIdx.x];
        __syncthreads();
    }
    return acc;
}

__device__ __forceinline__ long long draw_index(double u, int n) {
    if (!(u > 0.0)) return 0;                                            // a draw outside [0, 1) must not index outside the boxes
    if (u >= 1.0) return n - 1;
    const long long i = (long long)(u * (double)n);
    return i < n - 1 ? i : n - 1;
}

// ------------------------------------------------------------------------------------------------ seeding
// seed 0 of every restart, and the per-restart state: one thread per restart
__global__ __launch_bounds__(64) void anchor_init_kernel(const float2* __restrict__ wh, int n, int k, int restarts,
                                                         const double* __restrict__ draws, float* __restrict__ centroids,
                                                         int* __restrict__ picks, int* __restrict__ iterations, int* __restrict__ converged,
                                                         int* __restrict__ done) {
    const int r = threadIdx.x;
    if (r >= restarts) return;
    const long long p = draw_index(draws[(size_t)r * k], n);
    const float2 b = wh[p];
    centroids[(size_t)r * k * 2] = b.x;
    centroids[(size_t)r * k * 2 + 1] = b.y;
    if (picks) picks[(size_t)r * k] = (int)p;
    iterations[r] = 0;
    converged[r] = 0;
    done[r] = 0;
}

// running sum of d^2 over the thread's kItems consecutive boxes (d = 1 - the best IoU with the j chosen seeds); boxes past n add 0
__device__ __forceinline__ void thread_weights(const float2* __restrict__ wh, int n, long long i0, const float* __restrict__ c, int j,
                                               double (&cum)[kItems]) {
    double run = 0.0;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const long long idx = i0 + i;
        if (idx < n) {
            const float2 b = wh[idx];
            float best = wh_iou(b.x, b.y, c[0], c[1]);
            for (int s = 1; s < j; ++s) best = fmaxf(best, wh_iou(b.x, b.y, c[2 * s], c[2 * s + 1]));
            const double d = (double)(1.0f - best);
            run += d * d;
        }
        cum[i] = run;
    }
}

// bsum[restart][block] = sum of d^2 over the block's boxes
__global__ __launch_bounds__(kThreads) void anchor_seed_sums_kernel(const float2* __restrict__ wh, int n, int k, int j,
                                                                    const float* __restrict__ centroids, double* __restrict__ bsum) {
    __shared__ double s_w[kWaves];
    const int r = blockIdx.y;
    double cum[kItems], incl, excl, total;
    thread_weights(wh, n, (long long)blockIdx.x * kChunk + threadIdx.x * kItems, centroids + (size_t)r * k * 2, j, cum);
    block_scan(cum[kItems - 1], s_w, incl, excl, total);
    if (threadIdx.x == 0) bsum[(size_t)r * gridDim.x + blockIdx.x] = total;
}

// seed j of restart blockIdx.x: the first box whose running sum of d^2 exceeds draws[r][j] * T
__global__ __launch_bounds__(kThreads) void anchor_seed_pick_kernel(const float2* __restrict__ wh, int n, int k, int j,
                                                                    const double* __restrict__ draws, const double* __restrict__ bsum, int nb,
                                                                    float* centroids, int* __restrict__ picks) {
    __shared__ double s_w[kWaves];
    __shared__ double s_base;
    __shared__ int s_min;
    const int r = blockIdx.x, t = threadIdx.x;
    const double u = draws[(size_t)r * k + j];
    const double* bs = bsum + (size_t)r * nb;
    double incl, excl, total, carry = 0.0;
    for (int b0 = 0; b0 < nb; b0 += kThreads) {                          // T, by the association the search below uses
        block_scan(b0 + t < nb ? bs[b0 + t] : 0.0, s_w, incl, excl, total);
        carry += total;
    }
    const double T = carry;
    long long pick;
    if (!(T > 0.0)) {
        pick = draw_index(u, n);
    } else {
        const double target = u * T;
        int blk = -1;
        double base = 0.0;
        if (t == 0) s_min = INT_MAX;
        carry = 0.0;
        for (int b0 = 0; b0 < nb; b0 += kThreads) {                      // the first block whose inclusive prefix exceeds the target
            const int b = b0 + t;
            block_scan(b < nb ? bs[b] : 0.0, s_w, incl, excl, total);
            if (b < nb && carry + incl > target) atomicMin(&s_min, b);
            __syncthreads();
            const int m = s_min;
            if (m != INT_MAX) {
                if (b == m) s_base = carry + excl;
                __syncthreads();
                blk = m;
                base = s_base;
                break;
            }
            carry += total;
        }
        if (blk < 0) {
            pick = n - 1;                                                // u T rounded up to T: no running sum exceeds it
        } else {
            if (t == 0) s_min = INT_MAX;
            double cum[kItems];
            const long long i0 = (long long)blk * kChunk + t * kItems;
            thread_weights(wh, n, i0, centroids + (size_t)r * k * 2, j, cum);
            block_scan(cum[kItems - 1], s_w, incl, excl, total);
            const double start = base + excl;
            int first = INT_MAX;
#pragma unroll
            for (int i = kItems - 1; i >= 0; --i)
                if (i0 + i < n && start + cum[i] > target) first = t * kItems + i;
            if (first != INT_MAX) atomicMin(&s_min, first);
            __syncthreads();
            const int m = s_min;
            const long long last = (long long)blk * kChunk + kChunk - 1;   // the block's sum said yes, its own prefix says no: a last-bit matter
            pick = m != INT_MAX ? (long long)blk * kChunk + m : (last < n - 1 ? last : n - 1);
        }
    }
    if (t == 0) {
        const float2 b = wh[pick];
        centroids[((size_t)r * k + j) * 2] = b.x;
        centroids[((size_t)r * k + j) * 2 + 1] = b.y;
        if (picks) picks[(size_t)r * k + j] = (int)pick;
    }
}

// ------------------------------------------------------------------------------------------------ Lloyd step
// part[restart][block][cluster][3] = {sum w, sum h, count} over the block's boxes (thread t takes boxes base + i * kThreads + t)
__global__ __launch_bounds__(kThreads) void anchor_assign_kernel(const float2* __restrict__ wh, int n, int k, const float* __restrict__ centroids,
                                                                 const int* __restrict__ done, double* __restrict__ part) {
    __shared__ double s_part[kWaves][3 * kMaxK];
    const int r = blockIdx.y, t = threadIdx.x;
    if (done[r]) return;
    const float* c = centroids + (size_t)r * k * 2;
    float w[kItems], h[kItems];
    int lab[kItems];
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const long long idx = (long long)blockIdx.x * kChunk + i * kThreads + t;
        lab[i] = -1;
        w[i] = h[i] = 0.f;
        if (idx < n) {
            const float2 b = wh[idx];
            float best;
            w[i] = b.x;
            h[i] = b.y;
            lab[i] = best_match(b.x, b.y, c, k, best);
        }
    }
    for (int j = 0; j < k; ++j) {
        double sw = 0.0, sh = 0.0, cnt = 0.0;
#pragma unroll
        for (int i = 0; i < kItems; ++i)
            if (lab[i] == j) { sw += (double)w[i]; sh += (double)h[i]; cnt += 1.0; }
        sw = wave_sum(sw);
        sh = wave_sum(sh);
        cnt = wave_sum(cnt);
        if ((t & 63) == 0) { s_part[t >> 6][3 * j] = sw; s_part[t >> 6][3 * j + 1] = sh; s_part[t >> 6][3 * j + 2] = cnt; }
    }
    __syncthreads();
    if (t < 3 * k) part[((size_t)r * gridDim.x + blockIdx.x) * 3 * k + t] = ((s_part[0][t] + s_part[1][t]) + s_part[2][t]) + s_part[3][t];
}

// one block per restart: the block rows in ascending order, the new centroids, the stop test
__global__ __launch_bounds__(kThreads) void anchor_update_kernel(int k, int step, const double* __restrict__ part, int nb, float* centroids,
                                                                 int* done, int* __restrict__ iterations, int* __restrict__ converged) {
    __shared__ double s_buf[kStage];
    __shared__ double s_acc[3 * kMaxK];
    const int r = blockIdx.x, t = threadIdx.x;
    if (done[r]) return;
    const double acc = ordered_sum(part + (size_t)r * nb * 3 * k, nb, 3 * k, s_buf);
    if (t < 3 * k) s_acc[t] = acc;
    __syncthreads();
    int changed = 0;
    if (t < k && s_acc[3 * t + 2] > 0.0) {                               // a cluster with no box keeps its centroid
        float* c = centroids + ((size_t)r * k + t) * 2;
        const float nw = (float)(s_acc[3 * t] / s_acc[3 * t + 2]), nh = (float)(s_acc[3 * t + 1] / s_acc[3 * t + 2]);
        changed = __float_as_uint(nw) != __float_as_uint(c[0]) || __float_as_uint(nh) != __float_as_uint(c[1]);
        c[0] = nw;
        c[1] = nh;
    }
    changed = __syncthreads_or(changed);
    if (t == 0) {
        iterations[r] = step;
        if (!changed) { converged[r] = 1; done[r] = 1; }
    }
}

// ------------------------------------------------------------------------------------------------ fitness
// row[restart][block] of `width` doubles: {sum of the best IoU} or, with wins, {sum, boxes whose best IoU > thr, wins of anchor 0 .. k-1}
__global__ __launch_bounds__(kThreads) void anchor_score_kernel(const float2* __restrict__ wh, int n, int k, const float* __restrict__ anchors,
                                                                float thr, int wins, int* __restrict__ labels, double* __restrict__ part) {
    __shared__ double s_w[kWaves];
    const int r = blockIdx.y, t = threadIdx.x;
    const float* c = anchors + (size_t)r * k * 2;
    int lab[kItems];
    double s = 0.0, above = 0.0;
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
        const long long idx = (long long)blockIdx.x * kChunk + i * kThreads + t;
        lab[i] = -1;
        if (idx < n) {
            const float2 b = wh[idx];
            float best;
            lab[i] = best_match(b.x, b.y, c, k, best);
            s += (double)best;
            if (best > thr) above += 1.0;
            if (labels) labels[idx] = lab[i];
        }
    }
    const int width = wins ? 2 + k : 1;
    double* row = part + ((size_t)r * gridDim.x + blockIdx.x) * width;
    s = block_sum(s, s_w);
    if (t == 0) row[0] = s;
    if (!wins) return;
    above = block_sum(above, s_w);
    if (t == 0) row[1] = above;
    for (int j = 0; j < k; ++j) {
        double cnt = 0.0;
#pragma unroll
        for (int i = 0; i < kItems; ++i) cnt += lab[i] == j ? 1.0 : 0.0;
        cnt = block_sum(cnt, s_w);
        if (t == 0) row[2 + j] = cnt;
    }
}

__global__ __launch_bounds__(kThreads) void anchor_kmeans_final_kernel(const double* __restrict__ part, int nb, int n, double* __restrict__ fitness) {
    __shared__ double s_buf[kStage];
    const double acc = ordered_sum(part + (size_t)blockIdx.x * nb, nb, 1, s_buf);
    if (threadIdx.x == 0) fitness[blockIdx.x] = acc / (double)n;
}

__global__ __launch_bounds__(kThreads) void anchor_fitness_final_kernel(const double* __restrict__ part, int nb, int n, int k,
                                                                        double* __restrict__ out2, int* __restrict__ counts) {
    __shared__ double s_buf[kStage];
    const int t = threadIdx.x;
    const double acc = ordered_sum(part, nb, 2 + k, s_buf);
    if (t < 2) out2[t] = acc / (double)n;
    else if (t < 2 + k) counts[t - 2] = (int)acc;
}

static inline int n_blocks(int n) { return (int)(((long long)n + kChunk - 1) / kChunk); }
static inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline bool kmeans_shape_ok(int n, int k, int restarts) {
    return k >= 1 && k <= kMaxK && n >= k && restarts >= 1 && restarts <= kMaxRestarts;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

size_t yolo_anchor_kmeans_workspace_bytes(int n, int k, int restarts) {
    if (!kmeans_shape_ok(n, k, restarts)) return 0;
    return align16((size_t)restarts * sizeof(int32_t)) + (size_t)restarts * n_blocks(n) * 3 * k * sizeof(double);
}

int yolo_anchor_kmeans(const float* wh, int n, int k, int restarts, const double* draws, int max_iter, float* centroids, double* fitness,
                       int32_t* iterations, int32_t* converged, int32_t* picks, void* workspace, size_t workspace_bytes, void* stream) {
    if (!kmeans_shape_ok(n, k, restarts) || max_iter < 1)
        return fail(YOLO_ERR_ARG, "anchor_kmeans: need 1 <= k <= %d, k <= n, 1 <= restarts <= %d, max_iter >= 1 (n %d, k %d, restarts %d, max_iter %d)",
                    kMaxK, kMaxRestarts, n, k, restarts, max_iter);
    if (!wh || !draws || !centroids || !fitness || !iterations || !converged) return fail(YOLO_ERR_ARG, "anchor_kmeans: null pointer");
    if (((uintptr_t)wh & 7) || ((uintptr_t)draws & 7) || ((uintptr_t)fitness & 7)) return fail(YOLO_ERR_ARG, "anchor_kmeans: wh, draws and fitness must be 8-byte aligned");
    const size_t need = yolo_anchor_kmeans_workspace_bytes(n, k, restarts);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))
        return fail(YOLO_ERR_WORKSPACE, "anchor_kmeans: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    hipStream_t s = (hipStream_t)stream;
    const float2* b = reinterpret_cast<const float2*>(wh);
    const int nb = n_blocks(n);
    int* done = static_cast<int*>(workspace);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + align16((size_t)restarts * sizeof(int32_t)));
    const dim3 grid(nb, restarts);
    int rc;
    hipLaunchKernelGGL(anchor_init_kernel, dim3(1), dim3(64), 0, s, b, n, k, restarts, draws, centroids, picks, iterations, converged, done);
    if ((rc = check_launch("anchor_init"))) return rc;
    for (int j = 1; j < k; ++j) {
        hipLaunchKernelGGL(anchor_seed_sums_kernel, grid, dim3(kThreads), 0, s, b, n, k, j, centroids, part);
        hipLaunchKernelGGL(anchor_seed_pick_kernel, dim3(restarts), dim3(kThreads), 0, s, b, n, k, j, draws, part, nb, centroids, picks);
        if ((rc = check_launch("anchor_seed"))) return rc;
    }
    for (int step = 1; step <= max_iter; ++step) {
        hipLaunchKernelGGL(anchor_assign_kernel, grid, dim3(kThreads), 0, s, b, n, k, centroids, done, part);
        hipLaunchKernelGGL(anchor_update_kernel, dim3(restarts), dim3(kThreads), 0, s, k, step, part, nb, centroids, done, iterations, converged);
        if ((rc = check_launch("anchor_lloyd"))) return rc;
    }
    hipLaunchKernelGGL(anchor_score_kernel, grid, dim3(kThreads), 0, s, b, n, k, centroids, 0.f, 0, (int*)nullptr, part);
    hipLaunchKernelGGL(anchor_kmeans_final_kernel, dim3(restarts), dim3(kThreads), 0, s, part, nb, n, fitness);
    return check_launch("anchor_kmeans_fitness");
}

size_t yolo_anchor_fitness_workspace_bytes(int n, int k) {
    if (n < 1 || k < 1 || k > kMaxK) return 0;
    return (size_t)n_blocks(n) * (2 + k) * sizeof(double);
}

int yolo_anchor_fitness(const float* wh, int n, const float* anchors, int k, float iou_threshold, double* mean_iou_and_recall,
                        int32_t* counts, int32_t* labels, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 1 || k < 1 || k > kMaxK || iou_threshold != iou_threshold)
        return fail(YOLO_ERR_ARG, "anchor_fitness: need n >= 1, 1 <= k <= %d and a threshold that is a number (n %d, k %d)", kMaxK, n, k);
    if (!wh || !anchors || !mean_iou_and_recall || !counts) return fail(YOLO_ERR_ARG, "anchor_fitness: null pointer");
    if (((uintptr_t)wh & 7) || ((uintptr_t)mean_iou_and_recall & 7)) return fail(YOLO_ERR_ARG, "anchor_fitness: wh and the result must be 8-byte aligned");
    const size_t need = yolo_anchor_fitness_workspace_bytes(n, k);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(YOLO_ERR_WORKSPACE, "anchor_fitness: workspace of %zu bytes (8-byte aligned) needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    hipStream_t s = (hipStream_t)stream;
    const int nb = n_blocks(n);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(anchor_score_kernel, dim3(nb), dim3(kThreads), 0, s, reinterpret_cast<const float2*>(wh), n, k, anchors, iou_threshold, 1,
                       labels, part);
    hipLaunchKernelGGL(anchor_fitness_final_kernel, dim3(1), dim3(kThreads), 0, s, part, nb, n, k, mean_iou_and_recall, counts);
    return check_launch("anchor_fitness");
}

}  // extern "C"
