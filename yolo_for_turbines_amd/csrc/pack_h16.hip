// pack_h16.hip — fp32 OIHW weights -> the 16-bit MFMA-fragment streams of the bf16 / fp16 convolution kernels: forward and
// stride-1 input-gradient layouts (one layer or a batch of layers per launch), the four tap-subset streams of the stride-2
// input gradient and its fused form.
#include "h16.h"

namespace yolo {

// fragment-order 16-bit weights: [n_tile32][kt][s(2)][lane(64)][e(8)], n = nt*32 + (lane&31),
// ci = chunk*32 + s*16 + 8*(lane>>5) + e, (chunk, tap) = divmod(kt, ks*ks)
template <typename T>
__global__ void pack_weights_frag_h16(const float* __restrict__ w, unsigned short* __restrict__ wf, int cout, int cin, int ks,
                                      int KT, long long total) {
    const int taps = ks * ks;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        const int s = (int)((i >> 9) & 1);
        const long long rest = i >> 10;
        const int kt = (int)(rest % KT);
        const int nt = (int)(rest / KT);
        const int n = nt * 32 + (lane & 31);
        const int chunk = kt / taps, tap = kt - chunk * taps;
        const int ci = chunk * 32 + s * 16 + 8 * (lane >> 5) + e;
        const float v = (n < cout && ci < cin) ? w[((size_t)n * cin + ci) * taps + tap] : 0.f;
        wf[i] = HTraits<T>::from_f32(v);
    }
}

// same fragment order for the stride-1 input-gradient convolution dx = conv(dz, W'):
// n = ci, k channel = co, W'[ci][co][tap] = W[co][ci][taps-1-tap]  (see dgrad_f32.hip)
template <typename T>
__global__ void pack_dgrad_frag_h16(const float* __restrict__ w, unsigned short* __restrict__ wf, int cout, int cin, int ks,
                                    int KT, long long total) {
    const int taps = ks * ks;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        const int s = (int)((i >> 9) & 1);
        const long long rest = i >> 10;
        const int kt = (int)(rest % KT);
        const int nt = (int)(rest / KT);
        const int ci = nt * 32 + (lane & 31);
        const int chunk = kt / taps, tap = kt - chunk * taps;
        const int co = chunk * 32 + s * 16 + 8 * (lane >> 5) + e;
        const float v = (ci < cin && co < cout) ? w[((size_t)co * cin + ci) * taps + (taps - 1 - tap)] : 0.f;
        wf[i] = HTraits<T>::from_f32(v);
    }
}

// ---- many layers in ONE launch: an optimizer step changes every weight tensor, and 75 + 70 separate ~6 us pack launches
// per fine-tune step were 3 % of the bf16 step (the conversion itself is 0.1 ms of HBM time). Items ride in the kernel
// argument; a block finds its item by a scan of the (<= 48) first-block numbers.
constexpr int H_PACK_BATCH = 48;
struct PackItemH { const float* w; unsigned short* wf; int cout, cin, ks, KT; long long total; int first_block, nblocks; };
struct PackBatchH { PackItemH it[H_PACK_BATCH]; int n; };

template <typename T, bool DGRAD>
__global__ void pack_batch_h16(const PackBatchH b) {
    int k = 0;
    while (k + 1 < b.n && (int)blockIdx.x >= b.it[k + 1].first_block) ++k;
    const PackItemH& q = b.it[k];
    const int taps = q.ks * q.ks;
    const long long start = ((long long)blockIdx.x - q.first_block) * blockDim.x + threadIdx.x;
    for (long long i = start; i < q.total; i += (long long)q.nblocks * blockDim.x) {
        const int e = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        const int s = (int)((i >> 9) & 1);
        const long long rest = i >> 10;
        const int kt = (int)(rest % q.KT);
        const int nt = (int)(rest / q.KT);
        const int chunk = kt / taps, tap = kt - chunk * taps;
        const int a = nt * 32 + (lane & 31);                      // GEMM n: output channel (forward) / input channel (dgrad)
        const int c = chunk * 32 + s * 16 + 8 * (lane >> 5) + e;  // GEMM k channel
        float v = 0.f;
        if (DGRAD) { if (a < q.cin && c < q.cout) v = q.w[((size_t)c * q.cin + a) * taps + (taps - 1 - tap)]; }
        else       { if (a < q.cout && c < q.cin) v = q.w[((size_t)a * q.cin + c) * taps + tap]; }
        q.wf[i] = HTraits<T>::from_f32(v);
    }
}

// The same conversion one 32 x 32 x taps CELL per block: the rows of a cell are contiguous runs of 32 * taps floats in the
// OIHW tensor (forward: one output channel's 32 input channels; dgrad: one output channel's 32 input channels read as the
// GEMM's n), so they are read with 16-byte loads, rounded once, parked in LDS and written out in fragment order with one
// 16-byte store per (tap, half, lane). The element-wise kernel above reads 4 bytes at a stride of taps * 4 (and a 64-bit
// divide) per element: 2 x ~100 us per fine-tune step for the forward layouts and as much again for the gradient layouts.
// Needs cin % 32 == 0 (row alignment); other items keep the element-wise kernel.
template <typename T, bool DGRAD>
__global__ __launch_bounds__(256) void pack_batch_tiled_h16(const PackBatchH b) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[32][32 * 9 + 8];
    int k = 0;
    while (k + 1 < b.n && (int)blockIdx.x >= b.it[k + 1].first_block) ++k;
    const PackItemH& q = b.it[k];
    const int taps = q.ks * q.ks;
    const int chunks = q.KT / taps;
    const int cell = (int)blockIdx.x - q.first_block;
    const int nt = cell / chunks, chunk = cell - nt * chunks;
    const int run = 32 * taps;                                       // floats per row of the cell
    const int tid = threadIdx.x;
    // rows: forward = output channel a (n of the GEMM), columns (ci_local, tap); dgrad = output channel c (k of the GEMM),
    // columns (ci_local = n of the GEMM, source tap)
    {
        const int r = tid >> 3, part = tid & 7;                      // 8 threads per row
        const int row_ch = (DGRAD ? chunk : nt) * 32 + r;            // output channel of this row
        const int col0 = (DGRAD ? nt : chunk) * 32;                  // first input channel of the run
        const bool row_ok = row_ch < q.cout && col0 < q.cin;
        const float* src = q.w + ((size_t)row_ch * q.cin + col0) * taps;
        const int avail = row_ok ? ((q.cin - col0 < 32 ? q.cin - col0 : 32) * taps) : 0;   // floats of the run that exist
        for (int f = part * 4; f < run; f += 32) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (f + 3 < avail) v = *reinterpret_cast<const f32x4*>(src + f);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (f + e < avail) v[e] = src[f + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[r][f + e] = HTraits<T>::from_f32(v[e]);
        }
    }
    __syncthreads();
    for (int w = tid; w < taps * 128; w += 256) {                    // (tap, s, lane): one 16-byte store each
        const int lane = w & 63, s2 = (w >> 6) & 1, tap = w >> 7;
        const int al = lane & 31, cl = s2 * 16 + 8 * (lane >> 5);
        unsigned short h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = DGRAD ? tile[cl + e][al * taps + (taps - 1 - tap)] : tile[al][(cl + e) * taps + tap];
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (unsigned)h[2 * e] | ((unsigned)h[2 * e + 1] << 16);
        const size_t idx = (((size_t)nt * q.KT + (size_t)chunk * taps + tap) * 2 + s2) * 512 + (size_t)lane * 8;
        *reinterpret_cast<u32x4*>(q.wf + idx) = o;
    }
}

size_t h16_frag_elems(int cout, int cin, int ks) {
    const int cinp = round_up(cin, 32);
    return (size_t)(round_up(cout, 128) / 32) * (cinp / 32) * ks * ks * 1024;
}

int h16_pack(const float* w_oihw, void* wf, int cout, int cin, int ks, int dtype, hipStream_t s) {
    const long long total = (long long)h16_frag_elems(cout, cin, ks);
    const int KT = (round_up(cin, 32) / 32) * ks * ks;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    YOLO_SWITCH_H16(dtype, hipLaunchKernelGGL(pack_weights_frag_h16<T>, dim3(grid), dim3(256), 0, s, w_oihw, (unsigned short*)wf, cout, cin, ks, KT, total));
    return check_launch("pack_weights_frag_h16");
}

int h16_pack_dgrad(const float* w_oihw, void* wf, int cout, int cin, int ks, int dtype, hipStream_t s) {
    const int coutp = round_up(cout, 32);
    const long long total = (long long)h16_frag_elems(cin, coutp, ks);
    const int KT = (coutp / 32) * ks * ks;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    YOLO_SWITCH_H16(dtype, hipLaunchKernelGGL(pack_dgrad_frag_h16<T>, dim3(grid), dim3(256), 0, s, w_oihw, (unsigned short*)wf, cout, cin, ks, KT, total));
    return check_launch("pack_dgrad_frag_h16");
}

// items: host array. dgrad = 1: the flipped / transposed stride-1 input-gradient weights (h16_pack_dgrad layout)
int h16_pack_batch(const float* const* w, void* const* wf, const int* cout, const int* cin, const int* ks, int n, int dgrad, int dtype,
                   hipStream_t s) {
    // two passes over the items: those whose rows are 16-byte aligned runs (cin % 32 == 0) go to the tiled kernel, one cell
    // per block; the rest (the 3-channel stem) to the element-wise one
    for (int tiled = 1; tiled >= 0; --tiled) {
        int base = 0;
        while (base < n) {
            PackBatchH b;
            b.n = 0;
            int blocks = 0;
            for (; base < n && b.n < H_PACK_BATCH; ++base) {
                const int i = base;
                const bool can_tile = cin[i] % 32 == 0 && ks[i] * ks[i] <= 9;
                if (can_tile != (tiled == 1)) continue;
                PackItemH& q = b.it[b.n++];
                q.w = w[i]; q.wf = (unsigned short*)wf[i]; q.cout = cout[i]; q.cin = cin[i]; q.ks = ks[i];
                if (dgrad) {
                    const int coutp = round_up(cout[i], 32);
                    q.total = (long long)h16_frag_elems(cin[i], coutp, ks[i]);
                    q.KT = (coutp / 32) * ks[i] * ks[i];
                } else {
                    q.total = (long long)h16_frag_elems(cout[i], cin[i], ks[i]);
                    q.KT = (round_up(cin[i], 32) / 32) * ks[i] * ks[i];
                }
                if (tiled) {
                    q.nblocks = (int)(q.total / 1024 / (ks[i] * ks[i]));          // cells: n-tiles x 32-channel chunks
                } else {
                    const long long nb = (q.total + 255) / 256;
                    q.nblocks = (int)(nb < 1024 ? nb : 1024);
                }
                q.first_block = blocks;
                blocks += q.nblocks;
            }
            if (b.n == 0) continue;
            YOLO_SWITCH_H16(dtype,
                void (*const kern[2][2])(const PackBatchH) = {{pack_batch_h16<T, false>, pack_batch_h16<T, true>},
                                                              {pack_batch_tiled_h16<T, false>, pack_batch_tiled_h16<T, true>}};
                hipLaunchKernelGGL(kern[tiled][dgrad != 0], dim3(blocks), dim3(256), 0, s, b));
            const int rc = check_launch("pack_batch_h16");
            if (rc) return rc;
        }
    }
    return YOLO_OK;
}


// all four parity classes of one layer in ONE launch (they were four ~6 us launches per layer and step): the classes'
// fragment streams lie back to back in `wf`; `end[cls]` = end of class cls in that concatenation
struct S2ClsEnds { long long end[4]; };
template <typename T>
__global__ void pack_dgrad_s2_cls_h16(const float* __restrict__ w, unsigned short* __restrict__ wf, int cout, int cin, S2ClsEnds ends) {
    const long long total = ends.end[3];
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int cls = g < ends.end[0] ? 0 : (g < ends.end[1] ? 1 : (g < ends.end[2] ? 2 : 3));
        const long long i = g - (cls ? ends.end[cls - 1] : 0);
        const int ph = cls >> 1, pw = cls & 1;
        const int NT = (ph + 1) * (pw + 1);                       // taps of the class: 1, 2, 2, 4
        const int KT = (cout / 32) * NT;
        const int e = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        const int s = (int)((i >> 9) & 1);
        const long long rest = i >> 10;
        const int kt = (int)(rest % KT);
        const int nt = (int)(rest / KT);
        const int ci = nt * 32 + (lane & 31);
        const int chunk = kt / NT, t = kt - chunk * NT;
        const int dh = pw ? t / 2 : t, dw = pw ? t % 2 : 0;       // taps in window order: dh-major, dw-minor
        const int kh = ph + 1 - 2 * dh, kw = pw + 1 - 2 * dw;
        const int co = chunk * 32 + s * 16 + 8 * (lane >> 5) + e;
        const float v = (ci < cin && co < cout) ? w[((size_t)co * cin + ci) * 9 + kh * 3 + kw] : 0.f;
        wf[g] = HTraits<T>::from_f32(v);
    }
}

// ---- the same gradient as ONE launch for the layers with few dx channels (C = cin <= 64, multiple of 32): the four classes
// are the column blocks of one GEMM over the dz pixels, K = 4 neighbours x cout, N = 4 classes x C:
//   dx[n, 2r+ph, 2c+pw, :] = sum over neighbours (dr <= ph, dc <= pw) of dz[n, r+dr, c+dc, :] . W[:, :, ph+1-2dr, pw+1-2dc]
// 7 of the 16 (neighbour, class) blocks are zeros (1.78 x the matrix work), which these layers can afford: the four tap-subset
// launches each read all of dz and write a quarter of dx in half-line pieces, HBM-bound at 2.5 TB/s (4 x ~97 us for the
// 64-channel layers); here dz is read once and dx written once in full 16-byte rows.
bool s2g_ok(int cout, int cin) {
    return !switches().no_s2g && (cin == 32 || cin == 64) && cout % 32 == 0 && cout >= 32;
}
static size_t s2g_frag_elems(int cout, int cin) { return s2g_ok(cout, cin) ? (size_t)(4 * cin / 32) * (4 * cout / 32) * 1024 : 0; }

// [n_tile32][kt][s][lane][e]: n = class * cin + c, kt = chunk * 4 + neighbour, k = dz channel chunk * 32 + s * 16 + 8 (lane >> 5) + e
template <typename T>
__global__ void pack_dgrad_s2g_h16(const float* __restrict__ w, unsigned short* __restrict__ wf, int cout, int cin, long long total) {
    const int KT = 4 * (cout / 32);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        const int s = (int)((i >> 9) & 1);
        const long long rest = i >> 10;
        const int kt = (int)(rest % KT);
        const int nt = (int)(rest / KT);
        const int n = nt * 32 + (lane & 31);
        const int cls = n / cin, c = n - cls * cin;
        const int ph = cls >> 1, pw = cls & 1;
        const int chunk = kt >> 2, nb = kt & 3;
        const int dr = nb >> 1, dc = nb & 1;
        const int co = chunk * 32 + s * 16 + 8 * (lane >> 5) + e;
        float v = 0.f;
        if (dr <= ph && dc <= pw && co < cout) v = w[((size_t)co * cin + c) * 9 + (ph + 1 - 2 * dr) * 3 + (pw + 1 - 2 * dc)];
        wf[i] = HTraits<T>::from_f32(v);
    }
}

size_t h16_dgrad_s2_elems(int cout, int cin) {
    size_t n = 0;
    for (int cls = 0; cls < 4; ++cls) n += cls_frag_elems(cin, cout, cls);
    return n + s2g_frag_elems(cout, cin);                   // the fused layout follows the four class streams
}

int h16_pack_dgrad_s2(const float* w_oihw, void* wf, int cout, int cin, int dtype, hipStream_t s) {
    S2ClsEnds ends;
    long long acc = 0;
    for (int cls = 0; cls < 4; ++cls) {
        if (mask_count(cls_mask(cls >> 1, cls & 1)) != ((cls >> 1) + 1) * ((cls & 1) + 1)) return fail(YOLO_ERR_ARG, "dgrad_s2: class taps");
        acc += (long long)cls_frag_elems(cin, cout, cls);
        ends.end[cls] = acc;
    }
    const int grid = (int)((acc + 255) / 256 < 8192 ? (acc + 255) / 256 : 8192);
    YOLO_SWITCH_H16(dtype, hipLaunchKernelGGL(pack_dgrad_s2_cls_h16<T>, dim3(grid), dim3(256), 0, s, w_oihw, (unsigned short*)wf, cout, cin, ends));
    if (int rc = check_launch("pack_dgrad_s2_cls_h16")) return rc;
    const long long tg = (long long)s2g_frag_elems(cout, cin);
    if (tg) {
        unsigned short* wg = (unsigned short*)wf + acc;
        const int g2 = (int)((tg + 255) / 256 < 8192 ? (tg + 255) / 256 : 8192);
        YOLO_SWITCH_H16(dtype, hipLaunchKernelGGL(pack_dgrad_s2g_h16<T>, dim3(g2), dim3(256), 0, s, w_oihw, wg, cout, cin, tg));
        return check_launch("pack_dgrad_s2g_h16");
    }
    return YOLO_OK;
}

}  // namespace yolo
