// nms_order.hip — NMS stage 1: the candidates (objectness above the threshold) of every image in the reference's order, a
// stable descending sort of the scores (Python sorted(reverse=True)).   BUILD WITH -ffp-contract=off.
//
// Every ordering is a sort of UNIQUE 64-bit keys (make_key: ~orderable(score) << 32 | index), done one of three ways
// (nms_host.hip has the routing table):
//   counting rank   every candidate counts the keys smaller than its own; O(n^2), exactly parallel: small n
//   chunk sort      2,048-key chunks sorted in LDS + a rank merge, run twice: score order, then class-major rows for the
//                   class-sorted mask and scan. The same two kernels, without the NMS framing, are yolo_sort_u64 (mAP).
//   library sort    one rocPRIM radix sort of the batch + a key builder and a gather: sizes beyond the class scan's LDS.
// This is the only unit that includes rocPRIM.
#include "nms.h"
#include <rocprim/rocprim.hpp>
#include <type_traits>

namespace yolo {

// grid (ceil(n/256), B). rank = #keys smaller than mine.
__global__ __launch_bounds__(256) void nms_rank_kernel(const float* __restrict__ boxes, int n, double obj_thr, int center,
                                                       int* __restrict__ order, SBox* __restrict__ sbox,
                                                       int* __restrict__ nvalid) {
    __shared__ unsigned long long keys[256];
    const int b = blockIdx.y;
    const float* bx = boxes + (size_t)b * n * 6;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < n ? make_key(bx[(size_t)i * 6 + 4], i, obj_thr) : ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        __syncthreads();
        keys[threadIdx.x] = j < n ? make_key(bx[(size_t)j * 6 + 4], j, obj_thr) : ~0ull;
        __syncthreads();
        const int lim = n - j0 < 256 ? n - j0 : 256;
        for (int t = 0; t < lim; ++t) rank += keys[t] < mine;
    }
    const bool valid = mine != ~0ull;
    if (valid) {
        sbox[(size_t)b * n + rank] = make_sbox(bx + (size_t)i * 6, center);
        order[(size_t)b * n + rank] = i;
    }
    const unsigned long long bal = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(nvalid + b, __popcll(bal));
}

// ---- ordering by ONE radix sort of the whole batch (image id in the top key bits) ----------------------------------
// The counting rank above is O(n^2) (1e8 key compares per image at n = 10,000, 5e8 at the 22,743 boxes of a 608x608
// image); the keys are unique for valid boxes (the index is part of the key), so sorting them gives the identical
// order: rocPRIM's device radix sort (the plain library piece of this file) + a key builder and a gather.
// (rocPRIM's SEGMENTED sort was tried first: with 16 segments of 10,000 keys it was slower than the counting rank.)
// Today this orders only what the chunk sort below does not take: n > 163,456, where the class scan's LDS ends.

__global__ __launch_bounds__(256) void nms_keys_kernel(const float* __restrict__ boxes, int n, double obj_thr,
                                                       unsigned long long* __restrict__ keys) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = make_key(boxes[((size_t)b * n + i) * 6 + 4], i, obj_thr);
    // image (12 bits) | descending-score field (32 bits; all ones = filtered) | index (20 bits): ONE radix sort of the
    // whole batch leaves image b's boxes in [b n, (b + 1) n), valid ones first, in the reference's stable order
    const unsigned long long sc = k != ~0ull ? (k >> 32) : 0xffffffffull;
    keys[(size_t)b * n + i] = ((unsigned long long)b << 52) | (sc << 20) | (unsigned long long)i;
}

__global__ __launch_bounds__(256) void nms_gather_kernel(const float* __restrict__ boxes, const unsigned long long* __restrict__ sorted,
                                                         int* __restrict__ nvalid, int n, int center, int* __restrict__ order,
                                                         SBox* __restrict__ sbox) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const unsigned long long key = sorted[(size_t)b * n + r];
    if (!key_valid(key)) return;
    if (r == n - 1 || !key_valid(sorted[(size_t)b * n + r + 1])) nvalid[b] = r + 1;
    const int i = (int)(unsigned)(key & 0xfffffull);
    sbox[(size_t)b * n + r] = make_sbox(boxes + ((size_t)b * n + i) * 6, center);
    order[(size_t)b * n + r] = i;
}

// ---- hand-written ordering for every size of the class-sorted path (2,048 <= n <= 163,456: 1 .. 80 chunks per image). It
// replaced two rocPRIM sorts, whose ~16 merge launches were more than half of the batched NMS. Both orders are full sorts of
// UNIQUE 64-bit keys (the index / rank is part of the key):
//   order 1: make_key (score descending, index ascending)            -> global rank r of every valid box
//   order 2: class bucket | rank r | index                            -> class-major rows (a stable partition by class)
// Each is done by two launches that use the whole chip: (A) 2,048-key chunks sorted in LDS by a bitonic network, four
// keys per thread and two strides per LDS round trip; (B) one thread per key adds up, over the other chunks of its
// image, how many keys are smaller (binary searches, all chunks of a step in flight together) — that sum plus its
// position in its own chunk IS its final position, so the merge is a scatter. No atomics; deterministic.
__device__ __forceinline__ int sc_addr(int i) { return (i >> 3) * SC_ROW + (i & 7) * 8; }

template <int LG>            // 2^LG keys per thread, SC >> LG threads, LG strides per LDS round trip
__device__ __forceinline__ void chunk_sort_lds(char* lds, int tid) {
    constexpr int KPT = 1 << LG;
    // fully unrolled: every shift, mask and LDS offset below is an immediate
#pragma unroll
    for (int m = 1; m <= 11; ++m) {                       // bitonic merges of length 2^m; the last one ascending
#pragma unroll
        for (int p = m - 1; p >= 0; p -= LG) {            // strides 2^p .. 2^(p-LG+1) in ONE round trip
            const int lo = p >= LG - 1 ? p - (LG - 1) : 0;   // the thread's keys differ in bits lo .. lo+LG-1
            const int base = ((tid >> lo) << (lo + LG)) | (tid & ((1 << lo) - 1));
            unsigned long long r[KPT];
#pragma unroll
            for (int a = 0; a < KPT; ++a) r[a] = *reinterpret_cast<const unsigned long long*>(lds + sc_addr(base | (a << lo)));
#pragma unroll
            for (int sb = LG - 1; sb >= 0; --sb) {
                if (sb > p - lo) continue;
#pragma unroll
                for (int a = 0; a < KPT; ++a) {
                    if (a & (1 << sb)) continue;
                    const unsigned long long x = r[a], y = r[a | (1 << sb)];
                    const bool up = (((base | (a << lo)) >> m) & 1) == 0;      // direction of the length-2^m run this pair sits in
                    const bool sw = (x > y) == up;
                    r[a] = sw ? y : x;
                    r[a | (1 << sb)] = sw ? x : y;
                }
            }
#pragma unroll
            for (int a = 0; a < KPT; ++a) *reinterpret_cast<unsigned long long*>(lds + sc_addr(base | (a << lo))) = r[a];
            __syncthreads();
        }
    }
}

// (A) grid (nch, B), SC_THREADS threads. PHASE 1: keys from the boxes. PHASE 2: keys from order 1 (sorted1[b][r], r < nvalid[b]).
constexpr int SC_LG = 2;                 // chunk sort: 4 keys per thread, 512 threads (two waves per SIMD cover each other's LDS latency)
constexpr int SC_THREADS = SC >> SC_LG;
template <int PHASE>
__global__ __launch_bounds__(SC_THREADS) void nms_chunksort_kernel(const float* __restrict__ boxes, const unsigned long long* __restrict__ sorted1,
                                                            const int* __restrict__ nvalid, int n, double obj_thr,
                                                            unsigned long long* __restrict__ chunked, int* __restrict__ chunk_valid) {
    __shared__ __attribute__((aligned(16))) char lds[(SC / 8) * SC_ROW];
    const int b = blockIdx.y, c = blockIdx.x, nch = gridDim.x, tid = threadIdx.x;
    const int nv = PHASE == 2 ? nvalid[b] : 0;
#pragma unroll
    for (int e = 0; e < (1 << SC_LG); ++e) {
        const int loc = e * SC_THREADS + tid, i = c * SC + loc;
        unsigned long long key = ~0ull;
        if (PHASE == 1) {
            if (i < n) key = make_key(boxes[((size_t)b * n + i) * 6 + 4], i, obj_thr);
        } else {
            // class bucket (12 bits; 0xfff = not a candidate) | global rank (20) | original index (20): unique for every r
            key = (0xfffull << 40) | ((unsigned long long)(unsigned)i << 20);
            if (i < nv) {
                const unsigned long long idx = sorted1[(size_t)b * n + i] & 0xffffffffull;
                key = ((unsigned long long)class_bucket(boxes[((size_t)b * n + idx) * 6 + 5]) << 40) | ((unsigned long long)(unsigned)i << 20) | idx;
            }
        }
        *reinterpret_cast<unsigned long long*>(lds + sc_addr(loc)) = key;
    }
    __syncthreads();
    chunk_sort_lds<SC_LG>(lds, tid);
    unsigned long long* out = chunked + ((size_t)b * nch + c) * SC;
#pragma unroll
    for (int e = 0; e < (1 << SC_LG); ++e) {
        const int loc = e * SC_THREADS + tid;
        const unsigned long long key = *reinterpret_cast<const unsigned long long*>(lds + sc_addr(loc));
        out[loc] = key;
        if (PHASE == 1 && key != ~0ull) {                 // candidates sort first: the last one reports the count ...
            const unsigned long long nxt = loc + 1 < SC ? *reinterpret_cast<const unsigned long long*>(lds + sc_addr(loc + 1)) : ~0ull;
            if (nxt == ~0ull) chunk_valid[b * SC_MAXCH + c] = loc + 1;
        } else if (PHASE == 1 && loc == 0) {
            chunk_valid[b * SC_MAXCH + c] = 0;            // ... or the first key says there is none (no memset before the call)
        }
    }
}

// number of keys of the OTHER sorted chunks that are smaller than `key`: MAXC chunks at once (one load per chunk and step in
// flight), in rounds when there are more than MAXC + 1 chunks (MAXC = SC_GROUP: more than 32,768 keys)
template <int MAXC>       // slot k of a round is the (first + k)-th other chunk: chunk first + k, or the one after it from the thread's own chunk on
__device__ __forceinline__ int rank_in_other_chunks(const unsigned long long* __restrict__ img, int nch, int c, unsigned long long key) {
    int total = 0;
#pragma unroll 1
    for (int first = 0; first < nch - 1; first += MAXC) {
        int pos[MAXC];
        const unsigned long long* base[MAXC];
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            pos[k] = 0;
            const int ck = first + k + (first + k >= c ? 1 : 0);
            base[k] = img + (size_t)(ck < nch ? ck : 0) * SC;       // clamped: unconditional loads
        }
#pragma unroll 1
        for (int step = SC / 2; step >= 1; step >>= 1) {
            unsigned long long v[MAXC];
#pragma unroll
            for (int k = 0; k < MAXC; ++k) v[k] = base[k][pos[k] + step - 1];
#pragma unroll
            for (int k = 0; k < MAXC; ++k) pos[k] += v[k] < key ? step : 0;
        }
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            // positions are in [0, SC - 1]: the last element needs its own test
            const bool live = first + k + (first + k >= c ? 1 : 0) < nch;
            const int full = pos[k] + ((live && pos[k] == SC - 1 && base[k][SC - 1] < key) ? 1 : 0);
            total += live ? full : 0;
        }
    }
    return total;
}

// (B, order 1) grid (nch * 8, B), 256 threads: one key per thread. Writes sorted1[b][rank] for the candidates and nvalid[b].
template <int MAXC>
__global__ __launch_bounds__(256) void nms_merge1_kernel(const unsigned long long* __restrict__ chunked, const int* __restrict__ chunk_valid,
                                                         int nch, int n, unsigned long long* __restrict__ sorted1, int* __restrict__ nvalid,
                                                         unsigned long long* __restrict__ row_any, int W) {
    const int b = blockIdx.y, c = blockIdx.x >> 3, ploc = (blockIdx.x & 7) * 256 + threadIdx.x;
    const unsigned long long* img = chunked + (size_t)b * nch * SC;
    if (c * SC + ploc < W) row_any[(size_t)b * W + c * SC + ploc] = 0ull;       // the mask kernel ORs into it (nch SC >= n >= W)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int nv = 0;
        for (int k = 0; k < nch; ++k) nv += chunk_valid[b * SC_MAXCH + k];
        nvalid[b] = nv;
    }
    const unsigned long long key = img[(size_t)c * SC + ploc];
    if (key == ~0ull) return;
    const int rank = ploc + rank_in_other_chunks<MAXC>(img, nch, c, key);
    sorted1[(size_t)b * n + rank] = key;
}

// (B, order 2) same geometry; the destination row q also receives its box, its global rank and, at the ends of a 64-row block,
// the block's class range (the original index is not stored again: the scan takes it from order 1)
template <int MAXC>
__global__ __launch_bounds__(256) void nms_merge2_kernel(const float* __restrict__ boxes, const unsigned long long* __restrict__ chunked,
                                                         const int* __restrict__ nvalid, int nch, int n, int W, int center,
                                                         unsigned long long* __restrict__ sorted2, int* __restrict__ grank, SBox* __restrict__ sbox, int* __restrict__ blk_lo,
                                                         int* __restrict__ blk_hi) {
    const int b = blockIdx.y, c = blockIdx.x >> 3, ploc = (blockIdx.x & 7) * 256 + threadIdx.x;
    const unsigned long long* img = chunked + (size_t)b * nch * SC;
    const unsigned long long k = img[(size_t)c * SC + ploc];
    const int cls = (int)(unsigned)((k >> 40) & 0xfffull);
    if (cls == 0xfff) return;                                   // not a candidate (they all sort behind the candidates)
    const int q = ploc + rank_in_other_chunks<MAXC>(img, nch, c, k);
    const int nv = nvalid[b];
    const int i = (int)(unsigned)(k & 0xfffffull);
    sorted2[(size_t)b * n + q] = ((unsigned long long)b << 52) | k;
    sbox[(size_t)b * n + q] = make_sbox(boxes + ((size_t)b * n + i) * 6, center);
    grank[(size_t)b * n + q] = (int)(unsigned)((k >> 20) & 0xfffffull);
    if ((q & 63) == 0) blk_lo[(size_t)b * W + (q >> 6)] = cls;
    if ((q & 63) == 63 || q == nv - 1) blk_hi[(size_t)b * W + (q >> 6)] = cls;
}

// ---- segments: seg[b][bucket] = {first row, one past the last row} of the bucket's run in order 2 (zeroed before: empty)
__global__ __launch_bounds__(256) void nms_segments_kernel(const unsigned long long* __restrict__ sorted2, const int* __restrict__ nvalid, int n,
                                                            int agnostic, int* __restrict__ seg) {
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const int nv = nvalid[b];
    if (q >= nv) return;
    int* sg = seg + (size_t)b * CLASS_BUCKETS * 2;
    if (agnostic) {
        if (q == 0) { sg[0] = 0; sg[1] = nv; }
        return;
    }
    const unsigned long long* s = sorted2 + (size_t)b * n;
    const unsigned bucket = (unsigned)((s[q] >> 40) & 0xfffull);
    if (q == 0 || (unsigned)((s[q - 1] >> 40) & 0xfffull) != bucket) sg[bucket * 2] = q;
    if (q == nv - 1 || (unsigned)((s[q + 1] >> 40) & 0xfffull) != bucket) sg[bucket * 2 + 1] = q + 1;
}

// ---- the same two launches as a stand-alone ascending sort of UNIQUE 64-bit keys (none equal to ~0): the orderings of
// calc_mAP (utils.py:206,232: detections by class and descending objectness, ground truths by class and image - Python's
// stable sorts become one sort of (major | minor | original index) keys)
// (The load / sort / store frame is nms_chunksort_kernel's, written out a second time: through one shared helper the compiler
// emitted different code for both kernels.)
__global__ __launch_bounds__(SC_THREADS) void sort_chunks_kernel(const unsigned long long* __restrict__ in, int n, unsigned long long* __restrict__ chunked) {
    __shared__ __attribute__((aligned(16))) char lds[(SC / 8) * SC_ROW];
    const int c = blockIdx.x, tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < (1 << SC_LG); ++e) {
        const int loc = e * SC_THREADS + tid, i = c * SC + loc;
        *reinterpret_cast<unsigned long long*>(lds + sc_addr(loc)) = i < n ? in[i] : ~0ull;
    }
    __syncthreads();
    chunk_sort_lds<SC_LG>(lds, tid);
#pragma unroll
    for (int e = 0; e < (1 << SC_LG); ++e) {
        const int loc = e * SC_THREADS + tid;
        chunked[(size_t)c * SC + loc] = *reinterpret_cast<const unsigned long long*>(lds + sc_addr(loc));
    }
}
template <int MAXC>
__global__ __launch_bounds__(256) void sort_merge_kernel(const unsigned long long* __restrict__ chunked, int nch, unsigned long long* __restrict__ out) {
    const int c = blockIdx.x >> 3, ploc = (blockIdx.x & 7) * 256 + threadIdx.x;
    const unsigned long long key = chunked[(size_t)c * SC + ploc];
    if (key == ~0ull) return;                                   // padding of the last chunk
    out[ploc + rank_in_other_chunks<MAXC>(chunked, nch, c, key)] = key;
}

// ---- host side
// call f with the rank merges' MAXC for nch chunks as a compile-time constant: the smallest of 2, (4,) 8 that takes the nch - 1
// other chunks in one round, else SC_GROUP. WITH4 = false for a merge that has no 4-chunk instantiation.
template <bool WITH4, typename F>
static void with_merge_maxc(int nch, F f) {
    if (nch <= 3) return f(std::integral_constant<int, 2>());
    if constexpr (WITH4)
        if (nch <= 5) return f(std::integral_constant<int, 4>());
    if (nch <= 9) return f(std::integral_constant<int, 8>());
    f(std::integral_constant<int, SC_GROUP>());
}

int nms_order_rank(const float* boxes, int b, int n, double obj_thr, int center, int* order, SBox* sbox, int* nvalid, hipStream_t st) {
    hipLaunchKernelGGL(nms_rank_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, boxes, n, obj_thr, center, order, sbox, nvalid);
    return check_launch("nms_rank");
}

size_t nms_library_sort_tmp_bytes(int b, int n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)b * n, 0, 64,
                                   (hipStream_t)0);
    return bytes;
}

int nms_order_library_sort(const float* boxes, int b, int n, double obj_thr, int center, unsigned long long* keys_in, unsigned long long* keys_out,
                           void* sort_tmp, size_t sort_tmp_bytes, int* order, SBox* sbox, int* nvalid, hipStream_t st) {
    const dim3 gn(ceil_div(n, 256), b);
    hipLaunchKernelGGL(nms_keys_kernel, gn, dim3(256), 0, st, boxes, n, obj_thr, keys_in);
    if (int rc = check_launch("nms_keys")) return rc;
    size_t tb = sort_tmp_bytes;
    if (rocprim::radix_sort_keys(sort_tmp, tb, keys_in, keys_out, (size_t)b * n, 0, 64, st) != hipSuccess)
        return fail(YOLO_ERR_LAUNCH, "nms: radix sort");
    hipLaunchKernelGGL(nms_gather_kernel, gn, dim3(256), 0, st, boxes, keys_out, nvalid, n, center, order, sbox);
    return check_launch("nms_gather");
}

int nms_order_class_sorted(const float* boxes, int b, int n, int W, double obj_thr, int center, unsigned long long* chunked, int* chunk_valid,
                           unsigned long long* sorted1, unsigned long long* sorted2, int* nvalid, unsigned long long* row_any, int* grank,
                           SBox* sbox, int* blk_lo, int* blk_hi, hipStream_t st) {
    const int nch = ceil_div(n, SC);
    const dim3 ga(nch, b), gb(nch * 8, b);
    hipLaunchKernelGGL(nms_chunksort_kernel<1>, ga, dim3(SC_THREADS), 0, st, boxes, (const unsigned long long*)nullptr, (const int*)nullptr, n,
                       obj_thr, chunked, chunk_valid);
    with_merge_maxc<true>(nch, [&](auto maxc) {
        hipLaunchKernelGGL(nms_merge1_kernel<decltype(maxc)::value>, gb, dim3(256), 0, st, chunked, chunk_valid, nch, n, sorted1, nvalid, row_any, W);
    });
    if (int rc = check_launch("nms order 1")) return rc;
    // order 2 lands in a second array: order 1 is still being read by this chunk sort, and the scan reads it again
    hipLaunchKernelGGL(nms_chunksort_kernel<2>, ga, dim3(SC_THREADS), 0, st, boxes, sorted1, nvalid, n, obj_thr, chunked, chunk_valid);
    with_merge_maxc<true>(nch, [&](auto maxc) {
        hipLaunchKernelGGL(nms_merge2_kernel<decltype(maxc)::value>, gb, dim3(256), 0, st, boxes, chunked, nvalid, nch, n, W, center, sorted2, grank,
                           sbox, blk_lo, blk_hi);
    });
    return check_launch("nms order 2");
}

int nms_class_segments(const unsigned long long* sorted2, const int* nvalid, int b, int n, int agnostic, int* seg, hipStream_t st) {
    hipLaunchKernelGGL(nms_segments_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, sorted2, nvalid, n, agnostic, seg);
    return check_launch("nms class segments");
}

}  // namespace yolo

using namespace yolo;

extern "C" {

size_t yolo_sort_u64_workspace_bytes(int n) { return n > 0 ? (size_t)ceil_div(n, SC) * SC * sizeof(unsigned long long) : 8; }

int yolo_sort_u64(const uint64_t* keys, uint64_t* sorted, int n, void* workspace, size_t workspace_bytes, void* stream) {
    if (n <= 0) return YOLO_OK;
    if (!keys || !sorted || !workspace) return fail(YOLO_ERR_ARG, "sort_u64: null pointer");
    if (n > SC * SC_MAXCH) return fail(YOLO_ERR_UNSUPPORTED, "sort_u64: n = %d exceeds %d keys", n, SC * SC_MAXCH);
    if (workspace_bytes < yolo_sort_u64_workspace_bytes(n)) return fail(YOLO_ERR_WORKSPACE, "sort_u64: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nch = ceil_div(n, SC);
    unsigned long long* chunked = (unsigned long long*)workspace;
    hipLaunchKernelGGL(sort_chunks_kernel, dim3(nch), dim3(SC_THREADS), 0, st, (const unsigned long long*)keys, n, chunked);
    if (int rc = check_launch("sort_chunks")) return rc;
    const dim3 gb(nch * 8);
    with_merge_maxc<false>(nch, [&](auto maxc) {
        hipLaunchKernelGGL(sort_merge_kernel<decltype(maxc)::value>, gb, dim3(256), 0, st, chunked, nch, (unsigned long long*)sorted);
    });
    return check_launch("sort_merge");
}

}  // extern "C"
