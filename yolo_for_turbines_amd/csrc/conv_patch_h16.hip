// conv_patch_h16.hip — the register-staged bf16 / fp16 convolution block (fp32 accumulation): every shape the DMA kernels do
// not take (see conv_h16.hip), and the tap-subset variants of the stride-2 input gradient.
//
// Same fused block as the fp32 kernels (reference: CNNBlock.forward code/model.py:80-86, residual add
// :115-121, upsample+concat :189-191, head permute :145-148) and the same "patch + fragment stream"
// data movement as conv_f32_v2.hip, on v_mfma_f32_32x32x16_{bf16,f16}:
//  * activations NHWC 16-bit; a block owns TH x TW <= 128 output pixels (global rows) and stages, per
//    32-channel chunk, the input patch with halo in LDS once for all taps — stride 1 AND stride 2
//    (patch (S*(TH-1)+3 [+2 per image crossed]) x (S*(TW-1)+3)), 1x1 as the degenerate linear case;
//  * weights in MFMA-fragment order [n_tile32][kstep][2][64 lanes][8 halfs]: one contiguous 1 KiB load
//    per wave per 16 k-values, in a 3-deep register ring (a K step is only 8 MFMAs = 256 cycles, so the
//    loads are issued two K steps ahead); every in-loop load unconditional, taps compile-time,
//    sched_barrier after the prefetch group (see conv_f32_v2.hip for why);
//  * accumulators and the whole epilogue (scale/shift = folded BatchNorm, LeakyReLU/Mish, residual)
//    in fp32; one rounding to 16-bit at the store; detection heads are written in fp32.
// The matrix rate is 16x the fp32 path, so this kernel is bound by operand delivery (weight fragments
// through L1/L2) and, for 1x1 layers, by HBM; see DESIGN.md for the measured numbers.
#include "h16.h"

namespace yolo {

template <typename T, int TN>
struct HCtx {
    const unsigned short* wfrag[TN];
    int a_off[2];               // LDS byte offset of this lane's pixel for m-tile 0/1 (+16*h)
    int pix[H_NI];
    int KT;
};

// one K step = 32 channels of one tap = 2 MFMA k16-steps per 32x32 tile
template <typename T, int KS, int TN, int TAP>
__device__ __forceinline__ void h_kstep(const ConvHArgs& p, const HCtx<T, TN>& c, int chunk, char* patch,
                                        u32x4 (&ring)[3][2][TN], u32x4 (&stage)[H_NI], u32x4 (&af)[2][2],
                                        f32x16 (&acc)[2][TN], int tid) {
    typedef typename HTraits<T>::vec vec;
    constexpr int TAPS = KS * KS;
    constexpr int PF_TAP = TAPS > 2 ? TAPS - 2 : 0;
    constexpr int CUR = TAP % 3, NXT2 = (TAP + 2) % 3;
    const int kt = chunk * TAPS + TAP;
    const int kta = kt + 2 < c.KT ? kt + 2 : c.KT - 1;      // clamped: unconditional loads
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            ring[NXT2][s][j] = *reinterpret_cast<const u32x4*>(c.wfrag[j] + ((size_t)kta * 2 + s) * 512);
    if (TAP == PF_TAP) {
        const int cn = chunk + 1 < p.nchunks ? chunk + 1 : chunk;
        const int coff = p.x_off + cn * 32 + (tid & 3) * 8;
#pragma unroll
        for (int i = 0; i < H_NI; ++i) {
            const int px = c.pix[i] < 0 ? 0 : c.pix[i];
            stage[i] = *reinterpret_cast<const u32x4*>(p.x + (size_t)px * p.x_ld + coff);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int kh = TAP / KS, kw = TAP % KS;
    constexpr int nkh = (TAP + 1) / KS, nkw = (TAP + 1) % KS;
    const char* Ab_next = patch + (chunk & p.bufmask) * (p.patch_cap * H_PIX_BYTES) + (nkh * p.PC + nkw) * H_PIX_BYTES;
    (void)kh; (void)kw;
    // A fragments of this step were read during the previous one (af); read the next step's now
    u32x4 an[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) an[i][s] = af[i][s];
    if (TAP + 1 < TAPS) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) an[i][s] = *reinterpret_cast<const u32x4*>(Ab_next + c.a_off[i] + s * 32);
    }
    // keep the next step's A reads HERE, ahead of this step's 8 MFMAs: left free, the scheduler sinks them to just
    // before their first use and every K step starts with an exposed LDS round trip (seen in the ISA)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const vec b = __builtin_bit_cast(vec, ring[CUR][s][j]);
            acc[0][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, af[0][s]), b, acc[0][j]);
            acc[1][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, af[1][s]), b, acc[1][j]);
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) af[i][s] = an[i][s];
    if (TAP == TAPS - 1) {
        if (!p.bufmask) __syncthreads();             // one buffer: every wave has finished reading this chunk
        char* dst = patch + ((chunk + 1) & p.bufmask) * (p.patch_cap * H_PIX_BYTES) + (tid >> 2) * H_PIX_BYTES + (tid & 3) * 16;
#pragma unroll
        for (int i = 0; i < H_NI; ++i) {
            u32x4 z = {0u, 0u, 0u, 0u};
            if ((tid >> 2) + 64 * i < p.patch_cap) *reinterpret_cast<u32x4*>(dst + 64 * i * H_PIX_BYTES) = c.pix[i] < 0 ? z : stage[i];
        }
        __syncthreads();
        const char* An = patch + ((chunk + 1) & p.bufmask) * (p.patch_cap * H_PIX_BYTES);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) af[i][s] = *reinterpret_cast<const u32x4*>(An + c.a_off[i] + s * 32);
    }
}

template <typename T, int KS, int TN, int TAP>
__device__ __forceinline__ void h_chunk(const ConvHArgs& p, const HCtx<T, TN>& c, int chunk, char* patch,
                                        u32x4 (&ring)[3][2][TN], u32x4 (&stage)[H_NI], u32x4 (&af)[2][2],
                                        f32x16 (&acc)[2][TN], int tid) {
    if constexpr (TAP < KS * KS) {
        h_kstep<T, KS, TN, TAP>(p, c, chunk, patch, ring, stage, af, acc, tid);
        h_chunk<T, KS, TN, TAP + 1>(p, c, chunk, patch, ring, stage, af, acc, tid);
    }
}

// the same K step over a tap subset (MASK, see mask_count in h16.h): the parity classes of the stride-2 input gradient
template <typename T, int TN, int MASK, int TI, int R>
__device__ __forceinline__ void h_kstep_m(const ConvHArgs& p, const HCtx<T, TN>& c, int chunk, char* patch,
                                          u32x4 (&ring)[3][2][TN], u32x4 (&stage)[H_NI], u32x4 (&af)[2][2],
                                          f32x16 (&acc)[2][TN], int tid) {
    typedef typename HTraits<T>::vec vec;
    constexpr int NT = mask_count(MASK);
    constexpr int PF_T = NT > 2 ? NT - 2 : 0;
    constexpr int CUR = R % 3, NXT2 = (R + 2) % 3;
    constexpr int TAP0 = mask_nth(MASK, 0);
    const int kt = chunk * NT + TI;
    const int kta = kt + 2 < c.KT ? kt + 2 : c.KT - 1;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            ring[NXT2][s][j] = *reinterpret_cast<const u32x4*>(c.wfrag[j] + ((size_t)kta * 2 + s) * 512);
    if (TI == PF_T) {
        const int cn = chunk + 1 < p.nchunks ? chunk + 1 : chunk;
        const int coff = p.x_off + cn * 32 + (tid & 3) * 8;
#pragma unroll
        for (int i = 0; i < H_NI; ++i) {
            const int px = c.pix[i] < 0 ? 0 : c.pix[i];
            stage[i] = *reinterpret_cast<const u32x4*>(p.x + (size_t)px * p.x_ld + coff);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    u32x4 an[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) an[i][s] = af[i][s];
    if (TI + 1 < NT) {                                   // a_off already points at the first tap of the set
        constexpr int NTAP = mask_nth(MASK, TI + 1 < NT ? TI + 1 : 0);
        constexpr int dkh = NTAP / 3 - TAP0 / 3, dkw = NTAP % 3 - TAP0 % 3;
        const char* Ab_next = patch + (chunk & 1) * (p.patch_cap * H_PIX_BYTES) + (dkh * p.PC + dkw) * H_PIX_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) an[i][s] = *reinterpret_cast<const u32x4*>(Ab_next + c.a_off[i] + s * 32);
    }
    // keep the next step's A reads HERE, ahead of this step's 8 MFMAs: left free, the scheduler sinks them to just
    // before their first use and every K step starts with an exposed LDS round trip (seen in the ISA)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const vec b = __builtin_bit_cast(vec, ring[CUR][s][j]);
            acc[0][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, af[0][s]), b, acc[0][j]);
            acc[1][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, af[1][s]), b, acc[1][j]);
        }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) af[i][s] = an[i][s];
    if (TI == NT - 1) {
        char* dst = patch + ((chunk + 1) & 1) * (p.patch_cap * H_PIX_BYTES) + (tid >> 2) * H_PIX_BYTES + (tid & 3) * 16;
#pragma unroll
        for (int i = 0; i < H_NI; ++i) {
            u32x4 z = {0u, 0u, 0u, 0u};
            if ((tid >> 2) + 64 * i < p.patch_cap) *reinterpret_cast<u32x4*>(dst + 64 * i * H_PIX_BYTES) = c.pix[i] < 0 ? z : stage[i];
        }
        __syncthreads();
        const char* An = patch + ((chunk + 1) & 1) * (p.patch_cap * H_PIX_BYTES);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) af[i][s] = *reinterpret_cast<const u32x4*>(An + c.a_off[i] + s * 32);
    }
}

template <typename T, int TN, int MASK, int CC, int TI>
__device__ __forceinline__ void h_chunk_m(const ConvHArgs& p, const HCtx<T, TN>& c, int chunk, char* patch,
                                          u32x4 (&ring)[3][2][TN], u32x4 (&stage)[H_NI], u32x4 (&af)[2][2],
                                          f32x16 (&acc)[2][TN], int tid) {
    constexpr int NT = mask_count(MASK);
    if constexpr (TI < NT) {
        h_kstep_m<T, TN, MASK, TI, (CC * NT + TI) % 3>(p, c, chunk, patch, ring, stage, af, acc, tid);
        h_chunk_m<T, TN, MASK, CC, TI + 1>(p, c, chunk, patch, ring, stage, af, acc, tid);
    }
}

// 1x1: one tap per chunk -> unroll three chunks so the ring index stays compile-time. Activations are fetched TWO chunks
// ahead into a 3-slot register rotation (slots = pairs of stage[]): a chunk is only 8-16 MFMAs (~300 cycles), so with the
// usual one-chunk distance every chunk waited out a full L2 round trip (stamps: 700-1300 cycles per chunk).
template <typename T, int TN, int R>
__device__ __forceinline__ void h_kstep_1x1(const ConvHArgs& p, const HCtx<T, TN>& c, int chunk, char* patch,
                                            u32x4 (&ring)[3][2][TN], u32x4 (&stage)[H_NI], u32x4 (&af)[2][2],
                                            f32x16 (&acc)[2][TN], int tid) {
    typedef typename HTraits<T>::vec vec;
    constexpr int CUR = R % 3, NXT2 = (R + 2) % 3;
    constexpr int S_LOAD = ((R + 2) % 3) * 2, S_WRITE = ((R + 1) % 3) * 2;      // chunk + 2 arrives, chunk + 1 goes to LDS
    static_assert(H_NI >= 6, "three 2-entry slots");
    const int kta = chunk + 2 < c.KT ? chunk + 2 : c.KT - 1;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            ring[NXT2][s][j] = *reinterpret_cast<const u32x4*>(c.wfrag[j] + ((size_t)kta * 2 + s) * 512);
    {
        const int cn = chunk + 2 < p.nchunks ? chunk + 2 : p.nchunks - 1;
        const int coff = p.x_off + cn * 32 + (tid & 3) * 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {                   // 1x1 patch = 128 pixels = 2 passes of 64
            const int px = c.pix[i] < 0 ? 0 : c.pix[i];
            stage[S_LOAD + i] = *reinterpret_cast<const u32x4*>(p.x + (size_t)px * p.x_ld + coff);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const vec b = __builtin_bit_cast(vec, ring[CUR][s][j]);
            acc[0][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, af[0][s]), b, acc[0][j]);
            acc[1][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, af[1][s]), b, acc[1][j]);
        }
    char* dst = patch + ((chunk + 1) & 1) * (p.patch_cap * H_PIX_BYTES) + (tid >> 2) * H_PIX_BYTES + (tid & 3) * 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        u32x4 z = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(dst + 64 * i * H_PIX_BYTES) = c.pix[i] < 0 ? z : stage[S_WRITE + i];
    }
    __syncthreads();
    const char* An = patch + ((chunk + 1) & 1) * (p.patch_cap * H_PIX_BYTES);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) af[i][s] = *reinterpret_cast<const u32x4*>(An + c.a_off[i] + s * 32);
}

template <typename T, int KS, int STRIDE, int BN, int MASK>
__device__ __forceinline__ void conv_patch_h16_body(const ConvHArgs& p);

template <typename T, int KS, int STRIDE, int BN, int MASK = 0>
__global__ __launch_bounds__(256) void conv_patch_h16(const ConvHArgs p) { conv_patch_h16_body<T, KS, STRIDE, BN, MASK>(p); }

// Register cap for the 64-wide variants. Measured with per-block stamps: a CU held THREE blocks of the 1x1 variant
// (128 VGPRs + 32 AGPRs = 160) but never more than TWO of the 3x3 variant at 132 + 32 = 164, although the compiler's
// occupancy estimate says 3 for both (and LDS allows 4: tools/lds_occ_probe.hip) — the hardware allocates registers in
// coarser granules than the estimate assumes. With this attribute the compiler keeps the accumulators in VGPRs and lands at
// 154 (3x3) / 108 (1x1) registers in total; worth 1-2 % on the 64-wide layers.
template <typename T, int KS, int STRIDE, int MASK = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(128))) void conv_patch_h16_n64(const ConvHArgs p) {
    conv_patch_h16_body<T, KS, STRIDE, 64, MASK>(p);
}

template <typename T, int KS, int STRIDE, int BN, int MASK>
__device__ __forceinline__ void conv_patch_h16_body(const ConvHArgs& p) {
    constexpr int TN = BN / 64;
    constexpr int NI = KS == 1 ? 2 : H_NI;                             // staged pixels per 4-lane group that can be live (1x1: 128-pixel patch)
    static_assert(MASK == 0 || (KS == 3 && STRIDE == 1), "tap subsets are defined on the 3x3 stride-1 window");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* patch = smem_raw;                                             // [2 or 1][patch_cap][80 B]
    int* mtab = reinterpret_cast<int*>(patch + p.mtab_off);             // [128] output pixel of tile row, [128] head-layout base

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int fh = lane >> 5, frow = lane & 31;
#ifdef H16_STAMPS   // diagnostic build (make stamps): per-block phase stamps into the buffer passed as nan_flag
    const unsigned long long st0 = __builtin_amdgcn_s_memtime();
#endif

    if (p.stagger > 0 && (int)blockIdx.x < p.first_wave) {             // see conv_f32_v2.hip
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const int slot = (hw >> 16) & 15;
        for (int i = 0; i < slot * p.stagger; ++i) __builtin_amdgcn_s_sleep(32);
    }
    int bid = blockIdx.x;
    {
        const int nb = p.nblocks, q = nb / 8, r = nb % 8, xcd = bid % 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
    }
    const int sp = fdiv(bid, p.mg_tn, p.tiles_n);
    const int n_tile = bid - sp * p.tiles_n;

    // ---- prologue. Order matters: a 16-bit block's matrix work is ~9k cycles, so every exposed memory round trip counts.
    // (1) weight fragments of K steps 0 and 1 and the folded BatchNorm scale / shift need nothing but n_tile: request them
    //     FIRST, so they travel while the patch indices are computed (the index math used to run in front of every load)
    HCtx<T, TN> c;
    c.KT = p.KT;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nt = n_tile * (BN / 32) + j * 2 + wn;          // pass j of the epilogue = 64 CONTIGUOUS channels (full 128-B lines)
        c.wfrag[j] = p.wf + (size_t)nt * p.KT * 1024 + lane * 8;
    }
    u32x4 ring[3][2][TN], stage[H_NI], af[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int kq = q < p.KT ? q : p.KT - 1;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                ring[q][s][j] = *reinterpret_cast<const u32x4*>(c.wfrag[j] + ((size_t)kq * 2 + s) * 512);
    }
    float sc[TN], sh[TN];                                       // this lane's output channel of pass j: n_tile*BN + j*64 + wn*32 + frow
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        sc[j] = 1.f; sh[j] = 0.f;                              // gradient kernels (MASK): plain accumulation
        if (!MASK) {
            const int n = n_tile * BN + j * 64 + wn * 32 + frow;
            const int ncl = n < p.Cout ? n : p.Cout - 1;       // clamped: unconditional loads
            sc[j] = p.scale[ncl];
            sh[j] = p.shift[ncl];
            if (n >= p.Cout) { sc[j] = 0.f; sh[j] = 0.f; }
        }
    }
    __builtin_amdgcn_sched_barrier(0);

    // (2) patch geometry. Branch-free: every entry is computed for every lane and invalidated by a select (the nested
    //     ifs compiled to ~20 exec-mask branches per lane)
    const int r_tile = fdiv(sp, p.mg_tw, p.tiles_w);
    const int w_tile = sp - r_tile * p.tiles_w;
    const int g0 = r_tile * p.TH, c0 = w_tile * p.TW;
    const int g_last = (g0 + p.TH < p.rows_total ? g0 + p.TH : p.rows_total) - 1;
    const int Hp = p.Hin + 2;
    auto vrow = [&](int g) {
        if (KS != 3) return g;
        const int n = fdiv(g, p.mg_H, p.H);
        return n * Hp + STRIDE * (g - n * p.H);
    };
    const int v0 = vrow(g0);
    const int PR = vrow(g_last) + (KS == 3 ? 3 : 1) - v0;
#pragma unroll
    for (int i = 0; i < H_NI; ++i) c.pix[i] = -1;
#pragma unroll
    for (int i = 0; i < NI; ++i) {   // staged patch pixels of this 4-lane group: idx = (tid >> 2) + 64 i
        const int idx = (tid >> 2) + 64 * i;
        const int pr = fdiv(idx, p.mg_PC, p.PC), pc = idx - pr * p.PC;
        int pix;
        bool ok;
        if (KS == 3) {
            const int vv = v0 + pr;
            const int n = fdiv(vv, p.mg_Hp, Hp), yy = vv - n * Hp;
            const int hi = yy - 1, wi = STRIDE * c0 + pc - 1;
            ok = (pr < PR) & ((unsigned)hi < (unsigned)p.Hin) & ((unsigned)wi < (unsigned)p.Win);
            pix = (n * p.Hin + hi) * p.Win + wi;
        } else {
            pix = c0 + pc;
            ok = (pr < PR) & (pix < p.W);
        }
        c.pix[i] = ok ? pix : -1;
    }
    // (3) patch of chunk 0 (and, 1x1, of chunk 1 into register slot 1: h_kstep_1x1 runs two chunks ahead)
    {
        const int coff = p.x_off + (tid & 3) * 8;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int px = c.pix[i] < 0 ? 0 : c.pix[i];
            stage[i] = *reinterpret_cast<const u32x4*>(p.x + (size_t)px * p.x_ld + coff);
        }
    }
    if constexpr (KS == 1 && MASK == 0) {
        const int cn = 1 < p.nchunks ? 1 : 0;
        const int coff = p.x_off + cn * 32 + (tid & 3) * 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int px = c.pix[i] < 0 ? 0 : c.pix[i];
            stage[2 + i] = *reinterpret_cast<const u32x4*>(p.x + (size_t)px * p.x_ld + coff);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // (4) while those loads are in flight: A-fragment offsets and the tile-row -> output-pixel table of the epilogue
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pp = wm * 64 + i * 32 + frow;
        const int r = fdiv(pp, p.mg_TW, p.TW), cc = pp - r * p.TW;
        const int g = g0 + r;
        const bool ok = (pp < p.TH * p.TW) & (g <= g_last) & (c0 + cc < p.W);
        c.a_off[i] = (ok ? ((vrow(g) - v0) * p.PC + STRIDE * cc) * H_PIX_BYTES : 0) + 16 * fh;
        if (MASK) c.a_off[i] += ((mask_nth(MASK, 0) / 3) * p.PC + mask_nth(MASK, 0) % 3) * H_PIX_BYTES;
    }
    if (tid < 128) {
        const int r = fdiv(tid, p.mg_TW, p.TW), cc = tid - r * p.TW;
        const int g = g0 + r;
        int m = -1, mh = 0;
        if (tid < p.TH * p.TW && g <= g_last && c0 + cc < p.W) {
            if (MASK) {                               // parity class: dx pixel (2r + ph, 2c + pw) of image n
                const int n = fdiv(g, p.mg_H, p.H), rr = g - n * p.H;
                m = (n * 2 * p.H + 2 * rr + p.cls_ph) * (2 * p.W) + 2 * (c0 + cc) + p.cls_pw;
            } else {
                m = g * p.W + c0 + cc;
                if (p.out_mode == YOLO_OUT_HEAD) mh = m + 2 * (m / (p.Ho * p.Wo)) * (p.Ho * p.Wo);   // (img*3)*HoWo + pixel
            }
        }
        mtab[tid] = m;
        mtab[128 + tid] = mh;
    }
    {
        char* dst = patch + (tid >> 2) * H_PIX_BYTES + (tid & 3) * 16;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            u32x4 z = {0u, 0u, 0u, 0u};
            if (i < 3 || (tid >> 2) + 64 * i < p.patch_cap)              // patch_cap >= 224: the first three always fit
                *reinterpret_cast<u32x4*>(dst + 64 * i * H_PIX_BYTES) = c.pix[i] < 0 ? z : stage[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) af[i][s] = *reinterpret_cast<const u32x4*>(patch + c.a_off[i] + s * 32);
#pragma unroll
    for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(sc[j]), "+v"(sh[j]));   // pinned here: not re-loaded in the epilogue

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#ifdef H16_STAMPS
    asm volatile("s_nop 0" ::: "memory");
    const unsigned long long st1 = __builtin_amdgcn_s_memtime();
#endif
    if constexpr (MASK != 0) {
        int chunk = 0;
        for (; chunk + 3 <= p.nchunks; chunk += 3) {
            h_chunk_m<T, TN, MASK, 0, 0>(p, c, chunk, patch, ring, stage, af, acc, tid);
            h_chunk_m<T, TN, MASK, 1, 0>(p, c, chunk + 1, patch, ring, stage, af, acc, tid);
            h_chunk_m<T, TN, MASK, 2, 0>(p, c, chunk + 2, patch, ring, stage, af, acc, tid);
        }
        if (chunk < p.nchunks) h_chunk_m<T, TN, MASK, 0, 0>(p, c, chunk, patch, ring, stage, af, acc, tid);
        if (chunk + 1 < p.nchunks) h_chunk_m<T, TN, MASK, 1, 0>(p, c, chunk + 1, patch, ring, stage, af, acc, tid);
    } else if constexpr (KS == 3) {
        for (int chunk = 0; chunk < p.nchunks; ++chunk) h_chunk<T, 3, TN, 0>(p, c, chunk, patch, ring, stage, af, acc, tid);
    } else {
        int chunk = 0;
        for (; chunk + 3 <= p.nchunks; chunk += 3) {
            h_kstep_1x1<T, TN, 0>(p, c, chunk, patch, ring, stage, af, acc, tid);
            h_kstep_1x1<T, TN, 1>(p, c, chunk + 1, patch, ring, stage, af, acc, tid);
            h_kstep_1x1<T, TN, 2>(p, c, chunk + 2, patch, ring, stage, af, acc, tid);
        }
        if (chunk < p.nchunks) h_kstep_1x1<T, TN, 0>(p, c, chunk, patch, ring, stage, af, acc, tid);
        if (chunk + 1 < p.nchunks) h_kstep_1x1<T, TN, 1>(p, c, chunk + 1, patch, ring, stage, af, acc, tid);
    }

#ifdef H16_STAMPS
    asm volatile("s_nop 0" ::: "memory");
    const unsigned long long st2 = __builtin_amdgcn_s_memtime();
#endif
    // ---------------------------------------------------------------------- epilogue (fp32 math)
    // No memory round trip may sit on the critical path here: scale / shift came with the prologue, the residual rows of
    // BOTH 64-channel passes are requested before the accumulators go through LDS, and nothing ever waits for a store
    // (an s_waitcnt vmcnt(0) in front of a late load also waits for every store issued before it).
    const bool has_res = p.flags & YOLO_FLAG_RESIDUAL;
    const bool nan_chk = p.flags & YOLO_FLAG_NANCHECK;
    constexpr int OLD = 68;
    float* ost = reinterpret_cast<float*>(patch);                     // [128][68] fp32 = 34,816 B
    const bool vec_ok = p.flags & H_FLAG_VEC_EPILOGUE;               // 16-byte rows of y (and of the residual): patch_vec_epilogue
    bool saw_nan = false;
    __syncthreads();                                                  // every wave is done reading the patch
    const int c8 = tid & 7;
    int mrow[4];
    u32x4 rr[TN][4];
    if (vec_ok) {
#pragma unroll
        for (int it = 0; it < 4; ++it) mrow[it] = mtab[(tid >> 3) + 32 * it];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                rr[j][it] = z;
            }
        if (has_res) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int n = n_tile * BN + j * 64 + c8 * 8;
                    const int mc = mrow[it] < 0 ? 0 : mrow[it];
                    const int ncl = n < p.Cout ? n : 0;             // clamped: unconditional loads, discarded below
                    rr[j][it] = *reinterpret_cast<const u32x4*>(p.res + (size_t)mc * p.r_ld + p.r_off + ncl);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        {
            float* dst = ost + wn * 32 + frow;
            YOLO_SWITCH_ACT(p.act,
                _Pragma("unroll") for (int i = 0; i < 2; ++i)
                    _Pragma("unroll") for (int r = 0; r < 16; ++r) {
                        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                        dst[row * OLD] = act_c<ACT>(acc[i][j][r] * sc[j] + sh[j]);
                    })
        }
        __syncthreads();
        if (vec_ok) {
            unsigned short* yo = reinterpret_cast<unsigned short*>(p.y);
            const int n = n_tile * BN + j * 64 + c8 * 8;
            f32x4 va[4], vb[4];
            if (j == 0 && has_res) {
                // all residual rows (both passes) are awaited HERE, before the first store is issued: a later wait for a
                // pass-2 row would be counted against the stores issued in between (one in-order counter for loads and stores)
#pragma unroll
                for (int jj = 0; jj < TN; ++jj)
#pragma unroll
                    for (int it = 0; it < 4; ++it) asm volatile("" : "+v"(rr[jj][it]));
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {                           // all LDS reads first: one latency, not four
                const int row = (tid >> 3) + 32 * it;
                va[it] = *reinterpret_cast<const f32x4*>(ost + row * OLD + c8 * 8);
                vb[it] = *reinterpret_cast<const f32x4*>(ost + row * OLD + c8 * 8 + 4);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int m = mrow[it];
                if (m < 0 || n >= p.Cout) continue;
                float v[8] = {va[it][0], va[it][1], va[it][2], va[it][3], vb[it][0], vb[it][1], vb[it][2], vb[it][3]};
                if (has_res) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[2 * e] += HTraits<T>::to_f32((unsigned short)(rr[j][it][e] & 0xffffu));
                        v[2 * e + 1] += HTraits<T>::to_f32((unsigned short)(rr[j][it][e] >> 16));
                    }
                }
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (nan_chk && (v[2 * e] != v[2 * e] || v[2 * e + 1] != v[2 * e + 1])) saw_nan = true;
                    o[e] = (unsigned)HTraits<T>::from_f32(v[2 * e]) | ((unsigned)HTraits<T>::from_f32(v[2 * e + 1]) << 16);
                }
                if (p.out_mode == YOLO_OUT_NHWC) {
                    *reinterpret_cast<u32x4*>(yo + (size_t)m * p.y_ld + p.y_off + n) = o;
                } else {
                    const int HoWo = p.Ho * p.Wo;
                    const int img = m / HoWo;
                    const int rem = m - img * HoWo;
                    const int ho = rem / p.Wo;
                    const int wo2 = rem - ho * p.Wo;
                    const int W2 = 2 * p.Wo;
                    unsigned short* d = yo + ((size_t)(img * 2 * p.Ho + 2 * ho) * W2 + 2 * wo2) * p.y_ld + p.y_off + n;
                    *reinterpret_cast<u32x4*>(d) = o;
                    *reinterpret_cast<u32x4*>(d + p.y_ld) = o;
                    *reinterpret_cast<u32x4*>(d + (size_t)W2 * p.y_ld) = o;
                    *reinterpret_cast<u32x4*>(d + (size_t)(W2 + 1) * p.y_ld) = o;
                }
            }
        } else if (p.out_mode == YOLO_OUT_HEAD && !has_res) {   // detection heads: fp32 (B,3,g,g,5+nc), channel = a*(5+nc) + k
            const int col = tid & 63;
            const int n = n_tile * BN + j * 64 + col;
            const int head_a = n / p.nc5, head_k = n - head_a * p.nc5;
            const int HoWo = p.Ho * p.Wo;
            float* yo = reinterpret_cast<float*>(p.y);
            if (n < p.Cout) {
#pragma unroll 8
                for (int it = 0; it < 32; ++it) {
                    const int row = (tid >> 6) + 4 * it;
                    if (mtab[row] < 0) continue;
                    const float v = ost[row * OLD + col];
                    if (nan_chk && v != v) saw_nan = true;
                    yo[(size_t)(mtab[128 + row] + head_a * HoWo) * p.nc5 + head_k] = v;
                }
            }
        } else {                                    // odd channel counts outside the heads (block-level tests)
            const int HoWo = p.Ho * p.Wo;
            for (int it = 0; it < 32; ++it) {
                const int idx = tid + 256 * it;
                const int row = idx >> 6, col = idx & 63;
                const int m = mtab[row];
                const int n = n_tile * BN + j * 64 + col;
                if (m < 0 || n >= p.Cout) continue;
                float v = ost[row * OLD + col];
                if (has_res) v += HTraits<T>::to_f32(p.res[(size_t)m * p.r_ld + p.r_off + n]);
                if (nan_chk && v != v) saw_nan = true;
                const int img = m / HoWo;
                const int rem = m - img * HoWo;
                const int ho = rem / p.Wo;
                const int wo2 = rem - ho * p.Wo;
                if (p.out_mode == YOLO_OUT_HEAD) {
                    const int head_a = n / p.nc5, head_k = n - head_a * p.nc5;
                    reinterpret_cast<float*>(p.y)[((size_t)((img * 3 + head_a) * p.Ho + ho) * p.Wo + wo2) * p.nc5 + head_k] = v;
                } else if (p.out_mode == YOLO_OUT_NHWC) {
                    reinterpret_cast<unsigned short*>(p.y)[(size_t)m * p.y_ld + p.y_off + n] = HTraits<T>::from_f32(v);
                } else {
                    const int W2 = 2 * p.Wo;
                    unsigned short* d = reinterpret_cast<unsigned short*>(p.y) + ((size_t)(img * 2 * p.Ho + 2 * ho) * W2 + 2 * wo2) * p.y_ld + p.y_off + n;
                    const unsigned short hv = HTraits<T>::from_f32(v);
                    d[0] = hv; d[p.y_ld] = hv; d[(size_t)W2 * p.y_ld] = hv; d[(size_t)(W2 + 1) * p.y_ld] = hv;
                }
            }
        }
        if (j + 1 < TN) __syncthreads();
    }
    if (nan_chk && saw_nan) atomicOr(p.nan_flag, 2);
#ifdef H16_STAMPS
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st3 = __builtin_amdgcn_s_memtime();
        if (tid == 0) {
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* o = reinterpret_cast<unsigned long long*>(p.nan_flag) + (size_t)blockIdx.x * 6;
            o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3; o[4] = hw; o[5] = xcc;
        }
    }
#endif
}

// ------------------------------------------------------------------------------ host side
void pick_tile_h(int Hin, int Hout, int Wout, int ks, int stride, int* th, int* tw, int* prmax, int patch_cap) {
    if (ks == 1) { *th = 1; *tw = 128; *prmax = 1; return; }
    double best = -1;
    *th = 1; *tw = 1; *prmax = 3 + 2;
    for (int TW = 1; TW <= (Wout < 126 ? Wout : 126); ++TW) {
        int TH = 128 / TW;
        int pr = 0;
        while (TH >= 1) {
            const int cross = (TH + Hout - 1) / Hout;
            pr = stride * (TH - 1) + 3 + 2 * cross;
            if (pr * (stride * (TW - 1) + 3) <= patch_cap) break;
            --TH;
        }
        if (TH < 1) continue;
        const double eff = ((double)Wout / (ceil_div(Wout, TW) * TW)) * (TH * TW / 128.0);
        if (eff > best + 1e-9) { best = eff; *th = TH; *tw = TW; *prmax = pr; }
    }
    (void)Hin;
}

// The epilogue's vector path moves 8 channels per 16-byte store (and residual load): every address it forms must be 16-byte
// aligned, i.e. whole groups of 8 channels, and y (with a residual: r as well) with row stride and channel offset on 16 bytes
// (tensor base pointers are). Any other view takes the element-wise path. The heads (fp32 output) have a store of their own.
static void patch_vec_epilogue(ConvHArgs& a) {
    auto rows16 = [](int ld, int off) { return (ld & 7) == 0 && (off & 7) == 0; };
    const bool ok = a.out_mode != YOLO_OUT_HEAD && a.Cout % 8 == 0 && rows16(a.y_ld, a.y_off) &&
                    (!(a.flags & YOLO_FLAG_RESIDUAL) || rows16(a.r_ld, a.r_off));
    a.flags = ok ? a.flags | H_FLAG_VEC_EPILOGUE : a.flags & ~H_FLAG_VEC_EPILOGUE;
}

template <typename T, int KS, int STRIDE, int BN>
static int launch_h_t(ConvHArgs& a, hipStream_t s) {
    tile_grid_h(a, BN);
    patch_vec_epilogue(a);
    // Stride-2 3x3: the patch of 128 output pixels is ~500 input pixels, and two buffers of it (82 KB) leave ONE block per
    // CU (measured: >= 82 KB -> 1, 42-52 KB -> 3), i.e. nothing to overlap a block's staging and epilogue with. One buffer
    // + one more barrier per 32-channel chunk instead; the region also holds the epilogue's 128 x 68 fp32 staging tile.
    a.bufmask = (KS == 3 && STRIDE == 2) ? 0 : 1;
    size_t patch_bytes = (size_t)(a.bufmask + 1) * a.patch_cap * H_PIX_BYTES;
    if (patch_bytes < 128 * 68 * sizeof(float)) patch_bytes = 128 * 68 * sizeof(float);
    a.mtab_off = (int)patch_bytes;
    const size_t lds = patch_bytes + 256 * sizeof(int);
    if constexpr (BN == 64) hipLaunchKernelGGL((conv_patch_h16_n64<T, KS, STRIDE>), dim3(a.nblocks), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((conv_patch_h16<T, KS, STRIDE, BN>), dim3(a.nblocks), dim3(256), lds, s, a);
    return check_launch("conv_patch_h16");
}

template <typename T, int BN, int MASK>
static int launch_cls(ConvHArgs& a, hipStream_t s) {
    tile_grid_h(a, BN);
    patch_vec_epilogue(a);
    a.bufmask = 1;
    a.mtab_off = 2 * a.patch_cap * H_PIX_BYTES;
    const size_t lds = (size_t)a.mtab_off + 256 * sizeof(int);
    if constexpr (BN == 64) hipLaunchKernelGGL((conv_patch_h16_n64<T, 3, 1, MASK>), dim3(a.nblocks), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((conv_patch_h16<T, 3, 1, BN, MASK>), dim3(a.nblocks), dim3(256), lds, s, a);
    return check_launch("conv_patch_h16 (dgrad s2 class)");
}

template <typename T, int BN>
static int launch_cls_of(ConvHArgs& a, int cls, hipStream_t s) {
    switch (cls) {
    case 0: return launch_cls<T, BN, cls_mask(0, 0)>(a, s);
    case 1: return launch_cls<T, BN, cls_mask(0, 1)>(a, s);
    case 2: return launch_cls<T, BN, cls_mask(1, 0)>(a, s);
    default: return launch_cls<T, BN, cls_mask(1, 1)>(a, s);
    }
}

// the four parity classes of a stride-2 input gradient, one launch each; their fragment streams lie back to back in `wf`
int dgrad_s2_classes(ConvHArgs& a, const unsigned short* wf, int cin, int cout, int bn, int dtype, hipStream_t s) {
    for (int cls = 0; cls < 4; ++cls) {
        a.cls_ph = cls >> 1; a.cls_pw = cls & 1;
        a.wf = wf;
        a.KT = a.nchunks * mask_count(cls_mask(a.cls_ph, a.cls_pw));
        int rc;
        YOLO_SWITCH_H16(dtype, rc = bn == 128 ? launch_cls_of<T, 128>(a, cls, s) : launch_cls_of<T, 64>(a, cls, s));
        if (rc) return rc;
        wf += cls_frag_elems(cin, cout, cls);
    }
    return YOLO_OK;
}

template <typename T>
static int dispatch_h(ConvHArgs& a, int ks, int stride, int bn, hipStream_t s) {
    if (ks == 1) return bn == 128 ? launch_h_t<T, 1, 1, 128>(a, s) : launch_h_t<T, 1, 1, 64>(a, s);
    if (stride == 1) return bn == 128 ? launch_h_t<T, 3, 1, 128>(a, s) : launch_h_t<T, 3, 1, 64>(a, s);
    return bn == 128 ? launch_h_t<T, 3, 2, 128>(a, s) : launch_h_t<T, 3, 2, 64>(a, s);
}

int launch_h(ConvHArgs& a, int ks, int stride, int bn, int dtype, hipStream_t s) {
    YOLO_SWITCH_H16(dtype, return dispatch_h<T>(a, ks, stride, bn, s));
}

}  // namespace yolo
