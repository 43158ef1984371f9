// fuse.hip — weighted box fusion (WBF): the candidates of an image are merged into clusters whose box is the score-weighted
// mean of its members' corners.   BUILD WITH -ffp-contract=off.
//
// Nothing of the reference: the arithmetic is defined in DESIGN.md 7.20 and include/yolo_mi355x.h, fp32 with one rounding per
// operation, and tests/fuse_ref.py restates it in numpy. The walk is sequential by definition (a cluster's box moves when a member
// joins and the next candidate is matched against the moved box), so it cannot go through the NMS mask / scan kernels.
//
//   order     nms_order_class_sorted (nms_order.hip): the candidates' score order g (order 1) and the class-major rows (order 2)
//   segments  class-aware: clusters of different classes never interact, so every run of one class bucket in order 2 is an
//             independent walk (inside a run the rows are still in score order); class-agnostic: one walk per image over order 1
//   walk      ONE WAVE per segment, no barrier and no atomic: serial over the candidates, lanes across the clusters. Cluster k
//             lives in lane k & 63, slot k >> 6; the first FUSE_ONCHIP clusters of a segment in LDS, the rest in the workspace
//             (same code, other address space). A chunk of FUSE_CHUNK candidates is in registers, one per lane, the next one
//             is being loaded while this one is walked; the walked candidate is broadcast by v_readlane. The best match is a
//             wave maximum of (orderable IoU << 32 | ~k): largest IoU, ties to the cluster created first; it is taken by reading
//             the few lanes that matched into scalars (walking their ballot), not by cross-lane exchange steps. The IEEE division
//             is skipped for a cluster the candidate does not intersect (its IoU is exactly 0, which never passes a threshold
//             >= 0): in clustered data that is almost every cluster.
//   rank      the clusters of an image by (final score descending, founder rank ascending): a counting rank over their unique
//             64-bit keys - empty tiles of the key array are skipped - which IS the output row; the same launch writes the rows
//   assign    input row -> output row
// Everything is stream-ordered; the outputs are fully written by the call (memsets + scatters).
#include "nms.h"

namespace yolo {

constexpr int FUSE_ONCHIP = 1024;        // clusters of one segment held in LDS (52 bytes each: 52 KiB per wave, three waves per CU)
constexpr int FUSE_CHUNK = 64;           // candidates per prefetch chunk: one per lane
constexpr int FUSE_BUCKETS = CLASS_BUCKETS;
constexpr int FUSE_WAVES = 128;          // walk waves per image (class-aware): wave x takes buckets x, x + 128, ...
constexpr int FUSE_MAX_N = 163456;       // the n up to which yolo_nms orders class-sorted (nms_host.hip): at most 80 chunks of SC keys
static_assert(FUSE_MAX_N <= SC * 80 && FUSE_MAX_N < (1 << 20), "the ordering's chunk count and the 20-bit index fields");

struct FuseCand { float x1, y1, x2, y2, a, cls, s; int g; };

// bare v_max / v_min: fmaxf() makes the compiler canonicalise both operands first (nms_mask.hip)
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

__device__ __forceinline__ float bcast(float v, int t) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t)); }

__device__ __forceinline__ unsigned orderable(float f) {          // ascending-orderable bits, -0 as +0
    const unsigned u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the cluster arrays of one image in the workspace: the spill of the walk (position = segment start + k)
struct FuseSpill { float4* F; float4* A; float4* M; int* G; };   // M = {S, founder score, class, n as bits}

// grid (FUSE_WAVES or 1, B), 64 threads
__global__ __launch_bounds__(64) void fuse_walk_kernel(const float* __restrict__ boxes, const unsigned long long* __restrict__ order,
                                                       const int* __restrict__ seg, int n, int center, int agnostic, float thr, int n_views,
                                                       int conf_type, FuseSpill sp, float4* __restrict__ crec, unsigned long long* __restrict__ ckey,
                                                       int* __restrict__ joined) {
    __shared__ float4 sF[FUSE_ONCHIP], sA[FUSE_ONCHIP];
    __shared__ float sS[FUSE_ONCHIP], sFs[FUSE_ONCHIP], sCls[FUSE_ONCHIP];
    __shared__ int sN[FUSE_ONCHIP], sG[FUSE_ONCHIP];
    const int b = blockIdx.y, lane = threadIdx.x;
    const size_t img = (size_t)b * n;
    const float* bx = boxes + img * 6;
    const bool pretest = thr >= 0.0f;                     // a cluster without intersection has IoU +-0: it cannot pass
    const int nbuckets = agnostic ? 1 : FUSE_BUCKETS;

    // the wave's buckets x, x + gridDim.x, ...: lane l fetches the l-th of them (at most 32), one load instead of a chain of them
    int seg0 = 0, seg1 = 0;
    {
        const int mb = blockIdx.x + lane * gridDim.x;
        if (mb < nbuckets) {
            const int2 se = *reinterpret_cast<const int2*>(seg + ((size_t)b * FUSE_BUCKETS + mb) * 2);
            seg0 = se.x; seg1 = se.y;
        }
    }
    for (int it = 0; blockIdx.x + it * gridDim.x < nbuckets && it < 64; ++it) {
        const int s0 = __builtin_amdgcn_readlane(seg0, it), s1 = __builtin_amdgcn_readlane(seg1, it);
        if (s1 <= s0) continue;
        const int len = s1 - s0;
        float4* gF = sp.F + img + s0;                     // cluster k >= FUSE_ONCHIP of this segment: index k (k < len)
        float4* gA = sp.A + img + s0;
        float4* gM = sp.M + img + s0;
        int* gG = sp.G + img + s0;

        auto load = [&](int c) {                          // candidate c * 64 + lane of the segment
            FuseCand v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0};
            const int p = s0 + c * FUSE_CHUNK + lane;
            if (p < s1) {
                const unsigned long long key = order[img + p];
                const int i = agnostic ? (int)(unsigned)(key & 0xffffffffull) : (int)(unsigned)(key & 0xfffffull);
                const float* row = bx + (size_t)i * 6;
                const SBox sb = make_sbox(row, center);
                v.x1 = sb.x1; v.y1 = sb.y1; v.x2 = sb.x2; v.y2 = sb.y2; v.a = sb.area; v.cls = sb.cls; v.s = row[4];
                v.g = agnostic ? p : (int)(unsigned)((key >> 20) & 0xfffffull);
            }
            return v;
        };

        int K = 0;                                        // clusters so far (wave-uniform)
        FuseCand cur = load(0);
        const int nchunks = (len + FUSE_CHUNK - 1) / FUSE_CHUNK;
        for (int c = 0; c < nchunks; ++c) {
            FuseCand nxt = cur;
            if (c + 1 < nchunks) nxt = load(c + 1);       // in flight while this chunk is walked
            const int cnt = len - c * FUSE_CHUNK < FUSE_CHUNK ? len - c * FUSE_CHUNK : FUSE_CHUNK;
            int mine = 0;                                 // the cluster this lane's candidate joined
            for (int t = 0; t < cnt; ++t) {
                const float x1 = bcast(cur.x1, t), y1 = bcast(cur.y1, t), x2 = bcast(cur.x2, t), y2 = bcast(cur.y2, t);
                const float a = bcast(cur.a, t), cls = bcast(cur.cls, t), s = bcast(cur.s, t);
                const int g = __builtin_amdgcn_readlane(cur.g, t);

                unsigned long long best = 0ull;           // (orderable IoU << 32) | ~k; 0 = no match
                // `live`: the slot holds an eligible cluster. The intersection is computed for every slot (branch-free, a dead
                // slot's value is ignored); only a cluster the candidate intersects pays the IEEE division.
                auto eval = [&](const float4 F, const bool live, const int k) {
                    const float xa = vmax(x1, F.x), ya = vmax(y1, F.y), xb = vmin(x2, F.z), yb = vmin(y2, F.w);
                    const float inter = vmax(xb - xa, 0.f) * vmax(yb - ya, 0.f);
                    if (live && (inter > 0.f || !pretest)) {
                        const float ak = (F.z - F.x) * (F.w - F.y);
                        const float iou = inter / (((a + ak) - inter) + 1e-6f);
                        if (iou > thr) {
                            const unsigned long long key = ((unsigned long long)orderable(iou) << 32) | (0xffffffffu - (unsigned)k);
                            best = key > best ? key : best;
                        }
                    }
                };
                const int nslots = (K + 63) >> 6;
                const int nlds = nslots < FUSE_ONCHIP / 64 ? nslots : FUSE_ONCHIP / 64;
                for (int j0 = 0; j0 < nlds; j0 += 4) {    // four slots per LDS round trip (a slot past K reads a stale cluster, unused)
                    float4 Fv[4];
                    float cv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = ((j0 + u) & (FUSE_ONCHIP / 64 - 1)) * 64 + lane;
                        Fv[u] = sF[k];
                        cv[u] = sCls[k];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)           // all eight reads issued before the first use: keeps them out of the branches
                        asm volatile("" : "+v"(Fv[u].x), "+v"(Fv[u].y), "+v"(Fv[u].z), "+v"(Fv[u].w), "+v"(cv[u]));
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = (j0 + u) * 64 + lane;
                        eval(Fv[u], k < K && (agnostic || cv[u] == cls), k);
                    }
                }
                for (int j = FUSE_ONCHIP / 64; j < nslots; ++j) {
                    const int k = j * 64 + lane;
                    if (k < K) eval(gF[k], agnostic || gM[k].z == cls, k);
                }
                // wave maximum of the keys: the lanes that matched are few (the clusters the candidate overlaps), so they are
                // read one by one into scalars instead of six cross-lane exchange steps
                int kb = K;
                unsigned long long m = __ballot(best != 0ull);
                if (m) {
                    unsigned hi = 0u, lo = 0u;
                    do {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const unsigned h = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(best >> 32), l);
                        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(best & 0xffffffffull), l);
                        const bool up = h > hi || (h == hi && w > lo);
                        hi = up ? h : hi;
                        lo = up ? w : lo;
                    } while (m);
                    kb = (int)(0xffffffffu - lo);
                }
                if (lane == (kb & 63)) {
                    if (kb < K) {                         // joins cluster kb: sums, then the fused corners
                        float4 A; float S; int cn;
                        if (kb < FUSE_ONCHIP) { A = sA[kb]; S = sS[kb]; cn = sN[kb]; }
                        else { A = gA[kb]; const float4 M = gM[kb]; S = M.x; cn = __float_as_int(M.w); }
                        cn += 1;
                        S = S + s;
                        A.x = A.x + s * x1; A.y = A.y + s * y1; A.z = A.z + s * x2; A.w = A.w + s * y2;
                        const float4 F = make_float4(A.x / S, A.y / S, A.z / S, A.w / S);
                        if (kb < FUSE_ONCHIP) { sA[kb] = A; sF[kb] = F; sS[kb] = S; sN[kb] = cn; }
                        else { float4 M = gM[kb]; M.x = S; M.w = __int_as_float(cn); gA[kb] = A; gF[kb] = F; gM[kb] = M; }
                    } else {                              // founds cluster K: its own corners, not A / S
                        const float4 A = make_float4(s * x1, s * y1, s * x2, s * y2);
                        const float4 F = make_float4(x1, y1, x2, y2);
                        if (kb < FUSE_ONCHIP) { sA[kb] = A; sF[kb] = F; sS[kb] = s; sN[kb] = 1; sCls[kb] = cls; sFs[kb] = s; sG[kb] = g; }
                        else { gA[kb] = A; gF[kb] = F; gM[kb] = make_float4(s, s, cls, __int_as_float(1)); gG[kb] = g; }
                    }
                }
                if (kb >= FUSE_ONCHIP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the spilled cluster is read again by other lanes
                if (lane == t) mine = kb;
                K += kb == K ? 1 : 0;
            }
            if (lane < cnt) joined[img + s0 + c * FUSE_CHUNK + lane] = s0 + mine;
            cur = nxt;
        }

        // the segment's clusters: output record and ordering key at position s0 + k
        for (int k = lane; k < K; k += 64) {
            float4 F; float S, fs, cls; int cn, g;
            if (k < FUSE_ONCHIP) { F = sF[k]; S = sS[k]; fs = sFs[k]; cls = sCls[k]; cn = sN[k]; g = sG[k]; }
            else { F = gF[k]; const float4 M = gM[k]; S = M.x; fs = M.y; cls = M.z; cn = __float_as_int(M.w); g = gG[k]; }
            float score = conf_type == 0 ? S / (float)cn : fs;
            if (n_views > 0) score = score * ((float)(cn < n_views ? cn : n_views) / (float)n_views);
            const float w = F.z - F.x, h = F.w - F.y;
            const float x = center ? F.x + w / 2.0f : F.x, y = center ? F.y + h / 2.0f : F.y;
            crec[(img + s0 + k) * 2] = make_float4(x, y, w, h);
            crec[(img + s0 + k) * 2 + 1] = make_float4(score, cls, __int_as_float(cn), 0.f);
            ckey[img + s0 + k] = ((unsigned long long)(~orderable(score)) << 32) | (unsigned)g;
        }
    }
}

// ---- output rows. grid (ceil(n / 256), B): row = number of the image's cluster keys that are smaller (they are unique: the founder
// rank is part of the key). ckey is ~0 where there is no cluster; tiles of it without a cluster cost one load and a barrier.
__global__ __launch_bounds__(256) void fuse_rank_kernel(const unsigned long long* __restrict__ ckey, const float4* __restrict__ crec, int n,
                                                        float* __restrict__ fused, int* __restrict__ members, int* __restrict__ count,
                                                        int* __restrict__ rowof) {
    __shared__ unsigned long long keys[256];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const size_t img = (size_t)b * n;
    const unsigned long long mine = i < n ? ckey[img + i] : ~0ull;
    if (!__syncthreads_or(mine != ~0ull)) return;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + threadIdx.x;
        const unsigned long long kj = j < n ? ckey[img + j] : ~0ull;
        __syncthreads();
        keys[threadIdx.x] = kj;
        if (!__syncthreads_or(kj != ~0ull)) continue;
        for (int t = 0; t < 256; ++t) rank += keys[t] < mine;
    }
    const bool valid = mine != ~0ull;
    if (valid) {
        const float4 r0 = crec[(img + i) * 2], r1 = crec[(img + i) * 2 + 1];
        float2* o = reinterpret_cast<float2*>(fused + (img + rank) * 6);
        o[0] = make_float2(r0.x, r0.y);
        o[1] = make_float2(r0.z, r0.w);
        o[2] = make_float2(r1.x, r1.y);
        members[img + rank] = __float_as_int(r1.z);
        rowof[img + i] = rank;
    }
    const unsigned long long bal = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count + b, __popcll(bal));
}

// assign[b][input row] = output row of the cluster its candidate joined (-1 before: filtered rows)
__global__ __launch_bounds__(256) void fuse_assign_kernel(const unsigned long long* __restrict__ order, const int* __restrict__ nvalid, int n,
                                                          int agnostic, const int* __restrict__ joined, const int* __restrict__ rowof,
                                                          int* __restrict__ assign) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nvalid[b]) return;
    const size_t img = (size_t)b * n;
    const unsigned long long key = order[img + p];
    const int i = agnostic ? (int)(unsigned)(key & 0xffffffffull) : (int)(unsigned)(key & 0xfffffull);
    assign[img + i] = rowof[img + joined[img + p]];
}

struct FuseWs { int* nvalid; unsigned long long* row_any; int* chunk_valid; unsigned long long* chunked; unsigned long long* sorted1;
                unsigned long long* sorted2; int* grank; SBox* sbox; int* blk_lo; int* blk_hi; int* seg; FuseSpill sp; float4* crec;
                unsigned long long* ckey; int* joined; int* rowof; size_t total; };

static FuseWs fuse_carve(void* base, int b, int n) {
    const int W = ceil_div(n > 0 ? n : 1, 64);
    const size_t bn = (size_t)b * (n > 0 ? n : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return (char*)base + o; };
    FuseWs w;
    w.nvalid = (int*)take(sizeof(int) * (size_t)b);
    w.row_any = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * W);
    w.chunk_valid = (int*)take(sizeof(int) * (size_t)b * SC_MAXCH);
    w.chunked = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * ceil_div(n > 0 ? n : 1, SC) * SC);
    w.sorted1 = (unsigned long long*)take(sizeof(unsigned long long) * bn);
    w.sorted2 = (unsigned long long*)take(sizeof(unsigned long long) * bn);
    w.grank = (int*)take(sizeof(int) * bn);
    w.sbox = (SBox*)take(sizeof(SBox) * bn);
    w.blk_lo = (int*)take(sizeof(int) * (size_t)b * W);
    w.blk_hi = (int*)take(sizeof(int) * (size_t)b * W);
    w.seg = (int*)take(sizeof(int) * (size_t)b * FUSE_BUCKETS * 2);
    w.sp.F = (float4*)take(sizeof(float4) * bn);
    w.sp.A = (float4*)take(sizeof(float4) * bn);
    w.sp.M = (float4*)take(sizeof(float4) * bn);
    w.sp.G = (int*)take(sizeof(int) * bn);
    w.crec = (float4*)take(sizeof(float4) * 2 * bn);
    w.ckey = (unsigned long long*)take(sizeof(unsigned long long) * bn);
    w.joined = (int*)take(sizeof(int) * bn);
    w.rowof = (int*)take(sizeof(int) * bn);
    w.total = off;
    return w;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_fuse_onchip_clusters(void) { return FUSE_ONCHIP; }
int yolo_fuse_chunk_candidates(void) { return FUSE_CHUNK; }

size_t yolo_fuse_workspace_bytes(int b, int n) {
    if (b <= 0 || n < 0 || b > 2047 || n > FUSE_MAX_N) return 0;
    return fuse_carve(nullptr, b, n).total;
}

int yolo_fuse_boxes(const float* boxes, int b, int n, double iou_threshold, double obj_threshold, int center, int class_agnostic, int n_views,
                    int conf_type, float* fused, int32_t* members, int32_t* count, int32_t* assign, void* workspace, size_t workspace_bytes,
                    void* stream) {
    if (b <= 0 || n < 0 || !count) return fail(YOLO_ERR_ARG, "fuse_boxes: bad arguments");
    if (n_views < 0 || (conf_type != 0 && conf_type != 1) || iou_threshold != iou_threshold)
        return fail(YOLO_ERR_ARG, "fuse_boxes: n_views %d, conf_type %d or a NaN threshold", n_views, conf_type);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(int) * (size_t)b, st) != hipSuccess) return fail(YOLO_ERR_LAUNCH, "fuse_boxes: memset");
    if (n == 0) return YOLO_OK;
    if (!boxes || !fused || !members) return fail(YOLO_ERR_ARG, "fuse_boxes: null pointer");
    if (n > FUSE_MAX_N || b > 2047) return fail(YOLO_ERR_UNSUPPORTED, "fuse_boxes: n = %d (max %d) or b = %d (max 2047) too large", n, FUSE_MAX_N, b);
    if (!workspace || ((uintptr_t)workspace & 15)) return fail(YOLO_ERR_WORKSPACE, "fuse_boxes: workspace missing or not 16-byte aligned");
    const FuseWs w = fuse_carve(workspace, b, n);
    if (workspace_bytes < w.total) return fail(YOLO_ERR_WORKSPACE, "fuse_boxes: workspace %zu < %zu bytes", workspace_bytes, w.total);
    const size_t bn = (size_t)b * n;
    const int W = ceil_div(n, 64), agnostic = class_agnostic ? 1 : 0;
    bool ok = hipMemsetAsync(fused, 0, sizeof(float) * 6 * bn, st) == hipSuccess;
    ok = ok && hipMemsetAsync(members, 0, sizeof(int) * bn, st) == hipSuccess;
    ok = ok && (!assign || hipMemsetAsync(assign, 0xff, sizeof(int) * bn, st) == hipSuccess);
    ok = ok && hipMemsetAsync(w.seg, 0, sizeof(int) * (size_t)b * FUSE_BUCKETS * 2, st) == hipSuccess;
    ok = ok && hipMemsetAsync(w.ckey, 0xff, sizeof(unsigned long long) * bn, st) == hipSuccess;
    if (!ok) return fail(YOLO_ERR_LAUNCH, "fuse_boxes: memset");
    if (int rc = nms_order_class_sorted(boxes, b, n, W, obj_threshold, center, w.chunked, w.chunk_valid, w.sorted1, w.sorted2, w.nvalid,
                                        w.row_any, w.grank, w.sbox, w.blk_lo, w.blk_hi, st))
        return rc;
    const unsigned long long* order = agnostic ? w.sorted1 : w.sorted2;
    const dim3 gn(ceil_div(n, 256), b);
    if (int rc = nms_class_segments(w.sorted2, w.nvalid, b, n, agnostic, w.seg, st)) return rc;
    hipLaunchKernelGGL(fuse_walk_kernel, dim3(agnostic ? 1 : FUSE_WAVES, b), dim3(64), 0, st, boxes, order, w.seg, n, center ? 1 : 0, agnostic,
                       (float)iou_threshold, n_views, conf_type, w.sp, w.crec, w.ckey, w.joined);
    if (int rc = check_launch("fuse walk")) return rc;
    hipLaunchKernelGGL(fuse_rank_kernel, gn, dim3(256), 0, st, w.ckey, w.crec, n, fused, members, count, w.rowof);
    if (assign) hipLaunchKernelGGL(fuse_assign_kernel, gn, dim3(256), 0, st, order, w.nvalid, n, agnostic, w.joined, w.rowof, assign);
    return check_launch("fuse rank");
}

}  // extern "C"
