// =====================================================================================================
// conv3_dma_h16 — 3x3 stride-1 blocks with EVERY operand delivered by LDS-DMA (global_load_lds_dwordx4).
//
// Why (per-block stamps of conv_patch_h16, 128->256 @52x52, batch 32): a block's main loop takes ~19.5k cycles whether
// or not the second resident block is computing — 2 x the 9.2k cycles of its matrix work. The weight fragments travel
// L2 -> VGPR with a look-ahead of ~2 K steps (~580 matrix cycles), less than the L2 round trip under load, and a deeper
// REGISTER ring does not fit. Alone on its SIMDs a wave therefore runs at half rate, so the prologue / epilogue of one
// block is never covered by the other. Here the weights stream through a D_SLOTS-deep ring in LDS instead (shared by
// the four waves: half the L2 traffic, D_P K steps = ~1,000 matrix cycles of look-ahead, no staging registers), and the
// activation patch comes the same way, so the loop contains no register-destination load at all: every wait is a
// counted s_waitcnt vmcnt(N) in front of ONE raw s_barrier per K step (cdna_hip_programming.md "Pipelining across
// barriers"; a __syncthreads() would drain the DMA queue).
//   LDS: [2][256 px][64 B] patch (chunk double buffer) | [D_SLOTS][BN/32][2 KiB] weight ring | tile-row tables.
//   * patch rows are 64 B (32 channels) with the 16-byte granules XOR-swizzled by (pixel >> 2) & 3: an LDS-DMA image is
//     lane-linear, so the swizzle is applied to the per-lane SOURCE address and again in the fragment read; 16
//     consecutive pixels then cover all 16 granule slots of the 256-B bank row (conflict-free ds_read_b128);
//   * halo pixels outside the image read a zero page (g_zero_page) instead of being masked;
//   * the weight ring holds the fragment-order stream as it lies in HBM: wave w copies n-tile w of the block, every
//     wave reads its B fragments back lane-linearly.
//   K step t:  [DMA weights t+D_P] [tap 4: DMA patch of the next chunk] [ds_read A/B of step t+1] [8 MFMAs of step t]
//              [s_waitcnt vmcnt: own DMAs of step t+2 landed] [s_barrier].
// =====================================================================================================
#include "h16_dma_epilogue.h"

namespace yolo {

constexpr int D_PATCH_BYTES = D_PATCH_PIX * 64;  // 16 KiB per buffer
constexpr int D_P = 4;                           // weight K steps in flight
constexpr int D_SLOTS = D_P + 1;
constexpr int D_PF_TAP = 4;                      // tap at which the next chunk's patch is requested

template <typename T, int TN>
struct DCtx {
    const unsigned short* wsrc;      // this wave's n-tile of the fragment stream (+ lane * 8)
    const unsigned short* psrc[D_NI];// this lane's source granule of patch round i, chunk 0
    int p0[2];                       // patch pixel (tap 0,0) of this lane's row in m-tile 0 / 1
    int KT, PC;
};

template <typename T, int BN, int TAP, bool LAST>
__device__ __forceinline__ void d_kstep(const ConvHArgs& p, const DCtx<T, BN / 64>& c, int chunk, char* patch, char* wring,
                                        const unsigned short*& wp, int& slot_w, int& slot_r, u32x4 (&af)[2][2], u32x4 (&bf)[2][BN / 64],
                                        f32x16 (&acc)[2][BN / 64], int wave, int lane, int wn, int fh, const DRes& rs,
                                        u32x4 (&rr)[2][BN / 64][2]) {
    typedef typename HTraits<T>::vec vec;
    constexpr int TN = BN / 64;
    static_assert(TN == 2, "the interleave below is written for 2 x 2 tiles per wave");
    constexpr int SLOT_BYTES = (BN / 32) * 2048;
    // The WEIGHT fragment is the MFMA's A operand and the activation fragment its B operand (the two operand layouts are
    // mirror images, so the same packed streams serve either way): D = [channel][pixel], i.e. a lane owns ONE pixel and 16
    // channels of it in runs of 4 — the layout the register epilogue below stores from without an LDS round trip.
    // A lone wave must keep its matrix pipe fed by itself (the other resident block is in its prologue / epilogue half of the
    // time), so nothing is issued in a burst: the DMA requests and the 8 fragment reads of step t + 1 sit one per MFMA gap
    // (an MFMA occupies the pipe for 32 cycles and the issue port for 8 of them).
#define D_MFMA(i, j, s) acc[i][j] = HTraits<T>::mfma(__builtin_bit_cast(vec, bf[s][j]), __builtin_bit_cast(vec, af[i][s]), acc[i][j])
    u32x4 an[2][2], bn[2][TN];
    constexpr int NTAP = (TAP + 1) % 9;
    constexpr int nkh = NTAP / 3, nkw = NTAP % 3;
    const int nchunk = TAP == 8 ? chunk + 1 : chunk;
    const char* pb = patch + (nchunk & 1) * D_PATCH_BYTES;
    const char* wb = wring + slot_r * SLOT_BYTES + wn * 2048 + lane * 16;
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(0, 0, 0);
    constexpr bool last = LAST;                             // the last chunk of a tile is its own instantiation
    constexpr bool fetch = TAP < 9 - D_P || !last;          // nothing to fetch in the last D_P steps
    if (LAST && TAP == 7 && rs.has_res) {                   // residual rows, first half (see the note at the wait below)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const int ch = rs.ch0 + j * 64 + kp * 16;
                rr[0][j][kp] = *reinterpret_cast<const u32x4*>(rs.rptr[0] + (ch < p.Cout ? ch : 0));   // clamped, discarded in the epilogue
            }
    }
    char* wdst = wring + slot_w * SLOT_BYTES + wave * 2048;
    if (fetch) glds16(wp, wdst);                            // (1) weights of step t + D_P -> ring slot slot_w: first KiB here ...
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(1, 0, 0);
    {   // (2) activation fragments of step t + 1 (landed and made visible by the wait + barrier that closed step t - 1)
        const int px = c.p0[0] + nkh * c.PC + nkw;
        const int a0 = (px << 6) | ((((px >> 2) ^ fh) & 3) << 4);              // granule (s = 0) = fh, swizzled
        an[0][0] = *reinterpret_cast<const u32x4*>(pb + a0);
        an[0][1] = *reinterpret_cast<const u32x4*>(pb + (a0 ^ 32));            // granule 2 + fh
    }
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(0, 1, 0);
    {
        const int px = c.p0[1] + nkh * c.PC + nkw;
        const int a0 = (px << 6) | ((((px >> 2) ^ fh) & 3) << 4);
        an[1][0] = *reinterpret_cast<const u32x4*>(pb + a0);
        an[1][1] = *reinterpret_cast<const u32x4*>(pb + (a0 ^ 32));
    }
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(1, 1, 0);
    bn[0][0] = *reinterpret_cast<const u32x4*>(wb);                            // (3) weight fragments of step t + 1
    bn[1][0] = *reinterpret_cast<const u32x4*>(wb + 1024);
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(0, 0, 1);
    if (fetch) {                                            // ... second KiB four MFMAs later (a request costs ~60 cycles of issue, an
        glds16(wp + 512, wdst + 1024);                      //     MFMA covers 32: two in one gap leave the matrix pipe idle)
        wp += 1024;
        slot_w = slot_w + 1 == D_SLOTS ? 0 : slot_w + 1;
    }
    bn[0][1] = *reinterpret_cast<const u32x4*>(wb + 4096);
    bn[1][1] = *reinterpret_cast<const u32x4*>(wb + 4096 + 1024);
    slot_r = slot_r + 1 == D_SLOTS ? 0 : slot_r + 1;
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(1, 0, 1);
    if (LAST && TAP == 7 && rs.has_res) {                   // residual rows, second half
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const int ch = rs.ch0 + j * 64 + kp * 16;
                rr[1][j][kp] = *reinterpret_cast<const u32x4*>(rs.rptr[1] + (ch < p.Cout ? ch : 0));
            }
    }
    if (TAP == D_PF_TAP && !last) {   // (4) patch of the next chunk
        char* dst = patch + ((chunk + 1) & 1) * D_PATCH_BYTES + wave * 1024;
#pragma unroll
        for (int i = 0; i < D_NI; ++i) glds16(c.psrc[i] + (chunk + 1) * 32, dst + i * 4096);
    }
    __builtin_amdgcn_sched_barrier(0);
    D_MFMA(0, 1, 1);
    D_MFMA(1, 1, 1);
#undef D_MFMA
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) af[i][s] = an[i][s];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[s][j] = bn[s][j];
    __builtin_amdgcn_sched_barrier(0);
    // (5) own DMAs of step t + 2 have landed (2 weight ops per step are younger: steps t - 1 and t; + the patch ops if they
    //     were issued in one of those two steps), then the block-wide rendezvous that makes every wave's pieces visible.
    //     In the last chunk nothing is issued from tap 9 - D_P on (and no patch): the counts shrink with the queue, and
    //     the epilogue finds it empty
    //     From tap 6 of the last chunk the queue is empty: the residual rows of the epilogue are requested in tap 7 (ordinary
    //     loads: with no DMA pending hipcc counts them normally) and have the last two K steps + the epilogue's arithmetic
    //     to arrive; taps 7 and 8 wait for nothing.
    static_assert(D_P == 4 && D_PF_TAP == 4, "wait counts below");
    if (TAP == 4) { if (last) wait_vmcnt<4>(); else wait_vmcnt<4 + D_NI>(); }
    else if (TAP == 5) { if (last) wait_vmcnt<2>(); else wait_vmcnt<4 + D_NI>(); }
    else if (TAP == 6) { if (last) wait_vmcnt<0>(); else wait_vmcnt<4>(); }
    else if (TAP >= 7) { if (!last) wait_vmcnt<4>(); }
    else wait_vmcnt<4>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

template <typename T, int BN, int TAP, bool LAST>
__device__ __forceinline__ void d_chunk(const ConvHArgs& p, const DCtx<T, BN / 64>& c, int chunk, char* patch, char* wring,
                                        const unsigned short*& wp, int& slot_w, int& slot_r, u32x4 (&af)[2][2], u32x4 (&bf)[2][BN / 64],
                                        f32x16 (&acc)[2][BN / 64], int wave, int lane, int wn, int fh, const DRes& rs,
                                        u32x4 (&rr)[2][BN / 64][2]) {
    if constexpr (TAP < 9) {
        d_kstep<T, BN, TAP, LAST>(p, c, chunk, patch, wring, wp, slot_w, slot_r, af, bf, acc, wave, lane, wn, fh, rs, rr);
        d_chunk<T, BN, TAP + 1, LAST>(p, c, chunk, patch, wring, wp, slot_w, slot_r, af, bf, acc, wave, lane, wn, fh, rs, rr);
    }
}

template <typename T, int BN>
__global__ __launch_bounds__(256) void conv3_dma_h16(const ConvHArgs p) {
    constexpr int TN = BN / 64;
    constexpr int SLOT_BYTES = (BN / 32) * 2048;
    static_assert(BN / 32 == 4, "one weight n-tile per wave");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    char* patch = smem_raw;                                             // [2][256 px][64 B]
    char* wring = smem_raw + 2 * D_PATCH_BYTES;                         // [D_SLOTS][BN/32][2 KiB]
    int* mtab = reinterpret_cast<int*>(wring + D_SLOTS * SLOT_BYTES);   // [128] output pixel of tile row, [128] head-layout base
    float* sstab = reinterpret_cast<float*>(mtab + 256);                // [BN] scale, [BN] shift

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);         // wave id on the scalar unit: the DMA destinations need no VALU
    const int wm = wave >> 1, wn = wave & 1;
    const int fh = lane >> 5, frow = lane & 31;
#ifdef H16_STAMPS
    const unsigned long long st0 = __builtin_amdgcn_s_memtime();
#endif

    if (p.stagger > 0 && (int)blockIdx.x < p.first_wave) {             // see conv_f32_v2.hip
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const int slot = (hw >> 16) & 15;
        for (int i = 0; i < slot * p.stagger; ++i) __builtin_amdgcn_s_sleep(32);
    }
#ifdef H16_STAMPS
    const unsigned long long st0b = __builtin_amdgcn_s_memtime();
#endif
    int bid = blockIdx.x;
    {
        const int nb = p.nblocks, q = nb / 8, r = nb % 8, xcd = bid % 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
    }
    const int sp = fdiv(bid, p.mg_tn, p.tiles_n);
    const int n_tile = bid - sp * p.tiles_n;

    // The other resident block is usually in its main loop: its waves need the issue port for 8 of every 32 cycles (one
    // MFMA), this wave's prologue / epilogue needs it all the time. Priority, then age, arbitrates the port between the two
    // waves of a SIMD (MI355X_MICROARCH.md): take it while there is no matrix work here, give it back for the loop.
    if (p.prio) __builtin_amdgcn_s_setprio(2);
    DCtx<T, TN> c;
    c.KT = p.KT;
    c.PC = p.PC;
    c.wsrc = p.wf + (size_t)(n_tile * (BN / 32) + wave) * p.KT * 1024 + lane * 8;
    // ---- prologue: weight steps 0 and 1 leave at once (they need nothing but n_tile); steps 2 .. D_P-1 follow the patch,
    //      so that the first wait can leave them in flight (one in-order counter)
    auto issue_w = [&](int q) {
        const int kq = q < p.KT ? q : p.KT - 1;
        const unsigned short* src = c.wsrc + (size_t)kq * 1024;
        char* dst = wring + q * SLOT_BYTES + wave * 2048;
        glds16(src, dst);
        glds16(src + 512, dst + 1024);
    };
    issue_w(0);
    issue_w(1);
    // folded BatchNorm scale / shift of the block's BN channels: by LDS-DMA too (4 bytes per lane; waves 0-1 scale, 2-3 shift).
    // An ordinary load here would be awaited with vmcnt(0) — hipcc does not count a register load apart from pending DMAs
    {
        const int n = n_tile * BN + (wave & 1) * 64 + lane;
        const int ncl = n < p.Cout ? n : p.Cout - 1;
        __builtin_amdgcn_global_load_lds((gptr_t)((wave < 2 ? p.scale : p.shift) + ncl), (lptr_t)(sstab + wave * 64), 4, 0, 0);
    }
    // patch geometry (as conv_patch_h16, KS = 3, stride 1)
    const int r_tile = fdiv(sp, p.mg_tw, p.tiles_w);
    const int w_tile = sp - r_tile * p.tiles_w;
    const int g0 = r_tile * p.TH, c0 = w_tile * p.TW;
    const int g_last = (g0 + p.TH < p.rows_total ? g0 + p.TH : p.rows_total) - 1;
    const int Hp = p.Hin + 2;
    auto vrow = [&](int g) {
        const int n = fdiv(g, p.mg_H, p.H);
        return n * Hp + (g - n * p.H);
    };
    const int v0 = vrow(g0);
    const int PR = vrow(g_last) + 3 - v0;
    {
        const int gs = (tid & 3) ^ ((tid >> 4) & 3);           // source granule of LDS granule (pixel (tid>>2) + 64 i, slot tid & 3)
        const unsigned short* zp = reinterpret_cast<const unsigned short*>(g_zero_page) + gs * 8;
#pragma unroll
        for (int i = 0; i < D_NI; ++i) {
            const int idx = (tid >> 2) + 64 * i;
            const int pr = fdiv(idx, p.mg_PC, p.PC), pc = idx - pr * p.PC;
            const int vv = v0 + pr;
            const int n = fdiv(vv, p.mg_Hp, Hp), yy = vv - n * Hp;
            const int hi = yy - 1, wi = c0 + pc - 1;
            const bool ok = (pr < PR) & ((unsigned)hi < (unsigned)p.Hin) & ((unsigned)wi < (unsigned)p.Win);
            const int pix = (n * p.Hin + hi) * p.Win + wi;
            c.psrc[i] = ok ? p.x + (size_t)pix * p.x_ld + p.x_off + gs * 8 : zp;
        }
        char* dst = patch + wave * 1024;
#pragma unroll
        for (int i = 0; i < D_NI; ++i) glds16(c.psrc[i], dst + i * 4096);
    }
#pragma unroll
    for (int q = 2; q < D_P; ++q) issue_w(q);
    // while those travel: fragment rows and the tile-row -> output-pixel tables of the epilogue
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pp = wm * 64 + i * 32 + ((((p.qperm >> ((frow >> 2) * 4)) & 7) << 2) | (frow & 3));
        const int r = fdiv(pp, p.mg_TW, p.TW), cc = pp - r * p.TW;
        const int g = g0 + r;
        const bool ok = (pp < p.TH * p.TW) & (g <= g_last) & (c0 + cc < p.W);
        c.p0[i] = ok ? (vrow(g) - v0) * p.PC + cc : 0;
    }
    if (tid < 128) {
        const int pp = (tid & ~31) | (((p.qperm >> (((tid & 31) >> 2) * 4)) & 7) << 2) | (tid & 3);
        const int r = fdiv(pp, p.mg_TW, p.TW), cc = pp - r * p.TW;
        const int g = g0 + r;
        int m = -1, mh = 0;
        if (pp < p.TH * p.TW && g <= g_last && c0 + cc < p.W) {
            m = g * p.W + c0 + cc;
            if (p.out_mode == YOLO_OUT_HEAD) mh = m + 2 * (m / (p.Ho * p.Wo)) * (p.Ho * p.Wo);
        }
        mtab[tid] = m;
        mtab[128 + tid] = mh;
    }
    // weights of steps 0 and 1 and the patch of chunk 0 must have landed; steps 2 .. D_P-1 (the 2 (D_P - 2) youngest ops)
    // stay in flight — the same count the loop keeps
    wait_vmcnt<2 * (D_P - 2)>();
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    u32x4 af[2][2], bf[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int px = c.p0[i];
        const int a0 = (px << 6) | ((((px >> 2) ^ fh) & 3) << 4);
        af[i][0] = *reinterpret_cast<const u32x4*>(patch + a0);
        af[i][1] = *reinterpret_cast<const u32x4*>(patch + (a0 ^ 32));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        bf[0][j] = *reinterpret_cast<const u32x4*>(wring + wn * 2048 + lane * 16 + j * 4096);
        bf[1][j] = *reinterpret_cast<const u32x4*>(wring + wn * 2048 + lane * 16 + j * 4096 + 1024);
    }
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
    int slot_w = D_P % D_SLOTS, slot_r = 1;
    const unsigned short* wp = c.wsrc + (size_t)D_P * 1024;         // weights of step D_P: advanced by one step per request
    __builtin_amdgcn_s_setprio(0);
    // what the residual requests inside the last chunk need: this lane's output pixels and first channel
    const bool has_res = p.flags & YOLO_FLAG_RESIDUAL;
    int mpix[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) mpix[i] = mtab[wm * 64 + i * 32 + frow];
    DRes rs;
    rs.ch0 = n_tile * BN + wn * 32 + 8 * fh;
    rs.has_res = has_res;
    u32x4 rr[2][TN][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        rs.rptr[i] = p.res + (size_t)(mpix[i] < 0 ? 0 : mpix[i]) * p.r_ld + p.r_off;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                rr[i][j][kp] = z;
            }
    }
    for (int chunk = 0; chunk + 1 < p.nchunks; ++chunk)
        d_chunk<T, BN, 0, false>(p, c, chunk, patch, wring, wp, slot_w, slot_r, af, bf, acc, wave, lane, wn, fh, rs, rr);
    d_chunk<T, BN, 0, true>(p, c, p.nchunks - 1, patch, wring, wp, slot_w, slot_r, af, bf, acc, wave, lane, wn, fh, rs, rr);
    if (p.prio) __builtin_amdgcn_s_setprio(2);
#ifdef H16_STAMPS
    asm volatile("s_nop 0" ::: "memory");
    const unsigned long long st2 = __builtin_amdgcn_s_memtime();
#endif

    // ---------------------------------------------------------------------- epilogue (fp32 math, from registers)
    // acc[i][j]: rows = the 32 channels of this wave's n-tile j, columns = the 32 pixels of m-tile i. A lane owns pixel
    // (lane & 31) and channels 8g + 4h + {0..3} (g = 0..3, h = lane >> 5). Scale / shift / activation in that layout; then
    // one v_permlane32_swap per register pair exchanges halves so that lanes 0-31 hold channels 8k .. 8k+7 and lanes 32-63
    // channels 8k+8 .. 8k+15 of their pixel (k = 0, 2): 16 contiguous bytes of output per lane -> ONE 16-byte store (and one
    // 16-byte residual load) per lane, pixel and 16 channels. No LDS round trip, no barrier (cdna_hip_programming.md T21).
    const bool nan_chk = p.flags & YOLO_FLAG_NANCHECK;
    const int ch0 = rs.ch0;                                           // + j * 64 + 16 * kp: first of this lane's 8 output channels
    size_t ooff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = mpix[i] < 0 ? 0 : mpix[i];
        if (p.out_mode == YOLO_OUT_NHWC) {
            ooff[i] = (size_t)m * p.y_ld + p.y_off + ch0;
        } else {                                                      // 2x nearest upsample into the concat buffer
            const int HoWo = p.Ho * p.Wo;
            const int img = m / HoWo;
            const int rem = m - img * HoWo;
            const int ho = rem / p.Wo;
            const int wo2 = rem - ho * p.Wo;
            ooff[i] = ((size_t)(img * 2 * p.Ho + 2 * ho) * (2 * p.Wo) + 2 * wo2) * p.y_ld + p.y_off + ch0;
        }
    }
    // One straight-line instance per (activation, residual): chosen by ONE wave-uniform switch here. With the switch inside the
    // tile loops hipcc merged the variants through ~190 v_mov and a branch per tile, and with the residual add between the
    // stores every add waited for the stores before it (s_waitcnt vmcnt(0): one in-order counter, and the rows were requested
    // in another basic block) — ~500 cycles per store group on the 23 residual layers.
    bool saw_nan = false;
    if (p.stats != nullptr) {                                         // train-mode forward: raw z + BatchNorm partial sums
        if (p.bz == nullptr) d_epilogue_stats<T, BN>(p, acc, mpix, ooff, ch0, lane, sp * 2 + wm);
        else if (p.bact == YOLO_ACT_LEAKY) d_epilogue_bstats<T, BN, YOLO_ACT_LEAKY>(p, acc, rr, has_res, mpix, ooff, ch0, lane, sp * 2 + wm);
        else d_epilogue_bstats<T, BN, YOLO_ACT_MISH>(p, acc, rr, has_res, mpix, ooff, ch0, lane, sp * 2 + wm);
    } else {
    YOLO_SWITCH_ACT(p.act, saw_nan = has_res ? (d_epilogue<T, BN, ACT, true>(p, acc, rr, sstab, mpix, ooff, ch0, wn, fh))
                                             : (d_epilogue<T, BN, ACT, false>(p, acc, rr, sstab, mpix, ooff, ch0, wn, fh)));
    }
    if (nan_chk && saw_nan) atomicOr(p.nan_flag, 2);
#ifdef H16_STAMPS
    {
        const unsigned long long st3 = __builtin_amdgcn_s_memtime();      // stores issued, not awaited
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st4 = __builtin_amdgcn_s_memtime();
        if (tid == 0) {
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned long long* o = reinterpret_cast<unsigned long long*>(p.nan_flag) + (size_t)blockIdx.x * 6;
            o[0] = st0b; o[1] = st1; o[2] = st2; o[3] = st3; o[4] = hw; o[5] = xcc | ((st4 - st3) << 8) | ((st0b - st0) << 36);
        }
    }
#endif
}

int launch_dma(ConvHArgs& a, int dtype, hipStream_t s) {
    constexpr int BN = 128;
    tile_grid_h(a, BN);
    a.bufmask = 1;
    a.prio = switches().dma_prio ? 1 : 0;
    a.mtab_off = 2 * D_PATCH_BYTES + D_SLOTS * (BN / 32) * 2048;
    const size_t lds = (size_t)a.mtab_off + 256 * sizeof(int) + 2 * BN * sizeof(float);
    YOLO_SWITCH_H16(dtype,
        static LdsOnce once;                                // per kernel instantiation and device (common.h)
        if (int rc = reserve_lds(once, reinterpret_cast<const void*>(&conv3_dma_h16<T, BN>), lds, "conv3_dma_h16")) return rc;
        hipLaunchKernelGGL((conv3_dma_h16<T, BN>), dim3(a.nblocks), dim3(256), lds, s, a));
    return check_launch("conv3_dma_h16");
}

}  // namespace yolo
