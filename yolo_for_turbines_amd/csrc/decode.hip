// decode.hip — box decode: the (5 + nc) values of every grid cell to [x, y, w, h, obj, cls] rows.   BUILD WITH -ffp-contract=off.
//
// Replaces (reference file:line): cells_to_boxes code/utils.py:86-148. One scale per launch (yolo_decode, yolo_decode_hw) or
// the three scales of a forward in one (yolo_decode3, yolo_decode3_ex, yolo_decode3_hw). The kernels are bound by VALU issue
// and wave slots, not by HBM.
#include "common.h"

namespace yolo {

// ------------------------------------------------------------------------------ decode
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// x / d for 0 <= x < 2^31 with m = ceil(2^32 / d) (d >= 2) or 0 (d == 1)
struct DecodeMagic { unsigned mg, mgg, m3gg; };
__device__ __forceinline__ int pp_fdiv(int x, unsigned m, int d) {
    if (!m) return x;
    const unsigned q = __umulhi((unsigned)x, m);
    return (int)(q * (unsigned)d > (unsigned)x ? q - 1 : q);
}
static unsigned pp_magic(long long d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned long long)d - 1) / (unsigned long long)d); }
static DecodeMagic decode_magic(int gh, int gw) { return DecodeMagic{pp_magic(gw), pp_magic((long long)gh * gw), pp_magic(3LL * gh * gw)}; }

// one cell's box from its (5 + nc) values at src (LDS tile or global memory): called by the four lanes q of the cell together
__device__ __forceinline__ void decode_cell(float* __restrict__ pred, long long sb, long long sa, long long sy, long long sx, long long sk,
                                            const float* __restrict__ anchors, int gh, int gw, int nc, int is_pred, float* __restrict__ boxes,
                                            int n_total, int box_offset, long long cell, const float* src, long long kstride, bool staged, int q,
                                            const DecodeMagic mg) {
    // cell -> (b, a, row, col) by multiply-high (cells < 2^31, checked on the host): as four 64-bit divisions per lane this index
    // arithmetic was most of the kernel's issue time (~4.6 us per 64-cell tile)
    const int c32 = (int)cell, gg = gh * gw;
    const int b = pp_fdiv(c32, mg.m3gg, 3 * gg), r1 = c32 - b * 3 * gg;
    const int a = pp_fdiv(r1, mg.mgg, gg), r2 = r1 - a * gg;
    const int row = pp_fdiv(r2, mg.mg, gw), col = r2 - row * gw;
    float* gp = pred + b * sb + a * sa + row * sy + col * sx;
    if (!staged) src = gp;
    float cls;
    if (is_pred) {
        const int per = (nc + 3) >> 2;
        const int k0 = q * per, k1 = k0 + per < nc ? k0 + per : nc;
        bool have = k0 < k1;
        int best = k0;
        float bv = have ? src[(5 + k0) * kstride] : 0.f;
        int k = k0 + 1;
        for (; k + 8 <= k1; k += 8) {                    // 8 scores in flight: one LDS round trip per 8 instead of per score
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[(5 + k + u) * kstride];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (v[u] > bv || (v[u] != v[u] && bv == bv)) { bv = v[u]; best = k + u; }
        }
        for (; k < k1; ++k) {
            const float v = src[(5 + k) * kstride];
            if (v > bv || (v != v && bv == bv)) { bv = v; best = k; }
        }
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1) {      // lanes q and q + step: the later quarter wins only by the same rule
            const float ov = __shfl_down(bv, step, 4);
            const int ob = __shfl_down(best, step, 4);
            const int oh = __shfl_down((int)have, step, 4);
            if (oh && (!have || ov > bv || (ov != ov && bv == bv))) { bv = ov; best = ob; have = true; }
        }
        cls = (float)best;
    } else {
        cls = 0.f;
    }
    // `1 / grid_size` is a Python float, cast to fp32 by the multiply; per axis: x and w by 1/gw, y and h by 1/gh
    const float inv_w = (float)(1.0 / (double)gw), inv_h = (float)(1.0 / (double)gh);
    float* o = boxes + ((size_t)b * n_total + box_offset + (size_t)a * gg + (size_t)row * gw + col) * 6;
    if (is_pred) {
        // The four box values of a cell go to its four lanes (x, y: sigmoid; w, h: exp * anchor): the kernel is bound by VALU
        // issue (an expf is ~50 instructions for the whole wave however few lanes are active), and with lane 0 doing all five
        // transcendentals the other 48 lanes of the wave waited through them. Same operations per value as before.
        const float x = src[q * kstride];
        const float e = expf(q < 2 ? -x : x);
        const float v = q < 2 ? 1.f / (1.f + e) : e * anchors[2 * a + (q & 1)];
        // in-place side effect (utils.py:106-110): what cells_to_boxes does to its argument. is_pred == 2 (detect paths, where
        // the caller cannot observe the prediction tensor afterwards) leaves it alone: 16 bytes into every (5+nc)*4-byte cell
        // are a partial-line write per cell, 1.7x the algorithmic 24 bytes per box of this kernel's writes
        if (is_pred == 1) gp[q * sk] = v;
        const float add = q == 0 ? (float)col : (float)row;
        o[q] = ((q & 1) ? inv_h : inv_w) * (q < 2 ? v + add : v);
        if (q == 0) {
            o[4] = sigmoid_f(src[4 * kstride]);
            o[5] = cls;
        }
    } else if (q == 0) {
        o[0] = inv_w * (src[0] + (float)col);
        o[1] = inv_h * (src[kstride] + (float)row);
        o[2] = inv_w * src[2 * kstride];
        o[3] = inv_h * src[3 * kstride];
        o[4] = src[4 * kstride];
        o[5] = src[5 * kstride];
    }
}

// 256 threads per 64 cells (b, a, row, col): FOUR lanes per cell. For this library's contiguous head layout (stride 1
// along k) the 64 x (5 + nc) floats of the block are staged through LDS with full-line 16-byte loads by all 256 threads;
// each of a cell's four lanes then finds the first maximum of a quarter of the class scores and the partial results are
// combined in class order with the same rule, which is exactly the sequential first-maximum (torch.argmax; NaN counts as
// the maximum). Lane 0 of the cell finishes it. (One lane per cell and 64-thread blocks left 6-7 waves per CU, each
// waiting on its own loads and then on 80 dependent LDS reads: 2.5 TB/s.)
__device__ __forceinline__ void decode_block(float* __restrict__ pred, long long sb, long long sa, long long sy, long long sx, long long sk,
                                             const float* __restrict__ anchors, int B, int gh, int gw, int nc, int is_pred,
                                             float* __restrict__ boxes, int n_total, int box_offset, long long blk, const DecodeMagic mg) {
    extern __shared__ __attribute__((aligned(16))) float tile[];           // [64][D] when sk == 1 && cells contiguous, else unused
    const int D = 5 + nc;
    const int q = threadIdx.x & 3, cl = threadIdx.x >> 2;
    const long long cells = (long long)B * 3 * gh * gw;
    const long long cell0 = blk * 64;
    const long long cell = cell0 + cl;
    const bool contiguous = (sk == 1 && sx == D && sy == (long long)gw * D && sa == (long long)gh * gw * D &&
                             sb == 3LL * gh * gw * D);
    const float* src;
    long long kstride;
    if (contiguous) {
        const long long first = cell0 * D;
        const long long count = (cells - cell0 < 64 ? cells - cell0 : 64) * D;
        const float* gsrc = pred + first;
        if (count == 64LL * D && ((reinterpret_cast<size_t>(gsrc) & 15) == 0)) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            const int n4 = (int)(count >> 2);                                // 1,360 at 80 classes: <= 6 per thread, all in flight
            for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * 6) {
                f4 r[6];
#pragma unroll
                for (int u = 0; u < 6; ++u)
                    if (i0 + u * 256 < n4) r[u] = reinterpret_cast<const f4*>(gsrc)[i0 + u * 256];
#pragma unroll
                for (int u = 0; u < 6; ++u)
                    if (i0 + u * 256 < n4) reinterpret_cast<f4*>(tile)[i0 + u * 256] = r[u];
            }
        } else {
            for (long long i = threadIdx.x; i < count; i += 256) tile[i] = gsrc[i];
        }
        __syncthreads();
        src = tile + (long long)cl * D;
        kstride = 1;
    } else {
        src = nullptr;
        kstride = sk;
    }
    if (cell >= cells) return;                                               // the four lanes of a cell leave together
    decode_cell(pred, sb, sa, sy, sx, sk, anchors, gh, gw, nc, is_pred, boxes, n_total, box_offset, cell, src, kstride, contiguous, q, mg);
}

__global__ void decode_kernel(float* __restrict__ pred, long long sb, long long sa, long long sy, long long sx, long long sk,
                              const float* __restrict__ anchors, int B, int gh, int gw, int nc, int is_pred,
                              float* __restrict__ boxes, int n_total, int box_offset, const DecodeMagic mg) {
    decode_block(pred, sb, sa, sy, sx, sk, anchors, B, gh, gw, nc, is_pred, boxes, n_total, box_offset, blockIdx.x, mg);
}

// the three scales of one forward in ONE launch (demo.py:44-51 / utils.py:300-309 order): at batch 32 the three separate
// launches were launch-latency-bound (3 x ~25 us for 129 MB)
struct DecodeScale { float* pred; long long sb, sa, sy, sx, sk; const float* anchors; int gh, gw, box_offset; long long first_block; DecodeMagic mg; };
struct Decode3Args { DecodeScale sc[3]; int B, nc, n_total, is_pred; float* boxes; };

__global__ void decode3_kernel(const Decode3Args a) {
    const int k = (long long)blockIdx.x >= a.sc[2].first_block ? 2 : ((long long)blockIdx.x >= a.sc[1].first_block ? 1 : 0);
    const DecodeScale& d = a.sc[k];
    decode_block(d.pred, d.sb, d.sa, d.sy, d.sx, d.sk, d.anchors, a.B, d.gh, d.gw, a.nc, a.is_pred, a.boxes, a.n_total, d.box_offset,
                 (long long)blockIdx.x - d.first_block, d.mg);
}

// (Round 3 tried this launch as a STREAM: persistent workgroups, 2-4 LDS tiles, the next tiles requested by LDS-DMA while the
// current one is decoded, one barrier per tile. Slower at every depth: 3 workgroups/CU x 2 tiles 3.9 TB/s, 2 x 3 tiles 3.2,
// 1 x 4 tiles 1.9, against 4.4 TB/s for this kernel's ~7 independent workgroups per CU - a tile's decode is ~3 us of dependent
// LDS reads, compares and transcendentals per wave, so what the kernel needs is wave slots, not a deeper queue. DESIGN.md 7.4.)

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_decode(void* pred, const int64_t* s, const float* anchors, int b, int g, int nc, int is_pred, float* boxes,
                int n_total, int box_offset, void* stream) {
    return yolo_decode_hw(pred, s, anchors, b, g, g, nc, is_pred, boxes, n_total, box_offset, stream);
}

int yolo_decode_hw(void* pred, const int64_t* s, const float* anchors, int b, int gh, int gw, int nc, int is_pred, float* boxes,
                   int n_total, int box_offset, void* stream) {
    if (!pred || !s || !boxes || b <= 0 || gh <= 0 || gw <= 0 || nc < 1) return fail(YOLO_ERR_ARG, "decode: bad arguments");
    if (is_pred && !anchors) return fail(YOLO_ERR_ARG, "decode: anchors required");
    if (!is_pred && nc != 1) return fail(YOLO_ERR_ARG, "decode: targets must have last dim 6");
    if (box_offset < 0 || (long long)box_offset + 3LL * gh * gw > n_total) return fail(YOLO_ERR_ARG, "decode: box range outside n_total");
    const long long cells = (long long)b * 3 * gh * gw;
    if (cells > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "decode: too many cells");
    const int D = 5 + nc;
    const size_t lds = (size_t)64 * D * sizeof(float);
    if (lds > 64 * 1024) return fail(YOLO_ERR_UNSUPPORTED, "decode: %d classes exceed the staging tile", nc);
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((cells + 63) / 64)), dim3(256), lds, (hipStream_t)stream, (float*)pred,
                       (long long)s[0], (long long)s[1], (long long)s[2], (long long)s[3], (long long)s[4], anchors, b, gh, gw, nc,
                       is_pred, boxes, n_total, box_offset, decode_magic(gh, gw));
    return check_launch("decode");
}

int yolo_decode3(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids3, int b, int nc,
                 float* boxes, int n_total, void* stream) {
    return yolo_decode3_ex(preds3, strides15, anchors3, grids3, b, nc, 1, boxes, n_total, stream);
}

int yolo_decode3_ex(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids3, int b, int nc,
                    int write_back, float* boxes, int n_total, void* stream) {
    if (!grids3) return fail(YOLO_ERR_ARG, "decode3: bad arguments");
    const int hw6[6] = {grids3[0], grids3[0], grids3[1], grids3[1], grids3[2], grids3[2]};
    return yolo_decode3_hw(preds3, strides15, anchors3, hw6, b, nc, write_back, boxes, n_total, stream);
}

// the three scales into rows [first, first + sum 3 gh gw) of every image; `whole`: that must be the whole buffer
static int decode3_launch(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids_hw6, int b, int nc,
                          int write_back, float* boxes, int n_total, long long first, bool whole, void* stream) {
    if (!preds3 || !strides15 || !anchors3 || !grids_hw6 || !boxes || b <= 0 || nc < 1) return fail(YOLO_ERR_ARG, "decode3: bad arguments");
    Decode3Args a;
    a.B = b; a.nc = nc; a.n_total = n_total; a.boxes = boxes; a.is_pred = write_back ? 1 : 2;
    long long blocks = 0;
    long long off = first;
    for (int k = 0; k < 3; ++k) {
        const int gh = grids_hw6[2 * k], gw = grids_hw6[2 * k + 1];
        if (!preds3[k] || !anchors3[k] || gh <= 0 || gw <= 0) return fail(YOLO_ERR_ARG, "decode3: bad scale %d", k);
        if ((long long)b * 3 * gh * gw > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "decode3: too many cells");
        DecodeScale& d = a.sc[k];
        d.pred = (float*)preds3[k]; d.anchors = anchors3[k]; d.gh = gh; d.gw = gw; d.box_offset = (int)off; d.first_block = blocks;
        d.mg = decode_magic(gh, gw);
        d.sb = strides15[5 * k]; d.sa = strides15[5 * k + 1]; d.sy = strides15[5 * k + 2]; d.sx = strides15[5 * k + 3]; d.sk = strides15[5 * k + 4];
        off += 3LL * gh * gw;
        blocks += ((long long)b * 3 * gh * gw + 63) / 64;
    }
    if (whole && off != n_total) return fail(YOLO_ERR_ARG, "decode3: n_total %d != sum of 3 gh gw = %lld", n_total, off);
    if (off > n_total) return fail(YOLO_ERR_ARG, "decode3: rows [%lld, %lld) outside n_total %d", first, off, n_total);
    if (blocks > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "decode3: too many cells");
    const size_t lds = (size_t)64 * (5 + nc) * sizeof(float);
    if (lds > 64 * 1024) return fail(YOLO_ERR_UNSUPPORTED, "decode: %d classes exceed the staging tile", nc);
    hipLaunchKernelGGL(decode3_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch("decode3");
}

int yolo_decode3_hw(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids_hw6, int b, int nc,
                    int write_back, float* boxes, int n_total, void* stream) {
    return decode3_launch(preds3, strides15, anchors3, grids_hw6, b, nc, write_back, boxes, n_total, 0, true, stream);
}

int yolo_decode3_hw_at(void* const* preds3, const int64_t* strides15, const float* const* anchors3, const int* grids_hw6, int b, int nc,
                       int write_back, float* boxes, int n_total, int box_offset, void* stream) {
    if (box_offset < 0) return fail(YOLO_ERR_ARG, "decode3: box_offset %d", box_offset);
    return decode3_launch(preds3, strides15, anchors3, grids_hw6, b, nc, write_back, boxes, n_total, box_offset, false, stream);
}

}  // extern "C"
