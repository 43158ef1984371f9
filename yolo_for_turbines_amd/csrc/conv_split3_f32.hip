// conv_split3_f32.hip — fp32 implicit-GEMM convolution whose products run on the bf16 matrix cores (YOLO_FLAG_SPLIT_BF16).
//
// Same GEMM view, staging geometry, packed weights (row-major section) and epilogue as conv_igemm_f32 (conv_f32.hip). What
// differs is the arithmetic: v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate, and every fp32 value is exactly the sum of
// three bf16 values, a = a1 + a2 + a3 (8 + 8 + 8 significand bits). Before the LDS write each staged value is split into
// (hi, mid, lo) by truncation (masking the low 16 bits and subtracting: both steps exact, and a truncated value never
// overflows). Six of the nine partial products, accumulated in fp32 by v_mfma_f32_32x32x16_bf16 in one fixed order, smallest
// terms first, give a*b to fp32 accuracy: (hi,lo) (lo,hi) (mid,mid) (hi,mid) (mid,hi) (hi,hi). The dropped three are below
// 2^-23 relative. Six bf16 MFMAs cost 6/16 of the f32 MFMA they replace.
//
// LDS: three bf16 planes per operand, rows of 32 k = 64 bytes = four 16-byte slots, unpadded; slot s of row r is stored at slot
// s ^ ((r >> 2) & 3). A fragment read is 16 bytes per lane (row l & 31, k = 8 * (l >> 5) .. + 7 of a 16-wide chunk);
// ds_read_b128 banks over 256 bytes by 16-lane groups whose rows are {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31}: r & 3 picks the
// 64-byte quarter of the bank row and (r >> 2) & 3 the slot inside it, and each group holds all 16 combinations, so a read is
// conflict-free. The staging store is 8 bytes per lane (ds_write_b64: groups of 16 contiguous lanes = two adjacent rows of eight
// chunks, banks over 128 bytes): with a 64-byte pitch the two rows fill the two halves of the 128 bytes, whatever the order of the
// slots inside a row, so the store is conflict-free too. (A first version padded rows to 80 bytes: reads were clean but every
// store group put its two rows 4 banks into each other, 2-way; the swizzle took 2 - 10 % off 128x64 launches and 20 % off 64x64.)
// 64x64 blocks double-buffer (48 KB, three workgroups per CU); 128x64 and 128x128 keep one buffer and a second barrier per K
// step (36 KB of operands; the 128x128 epilogue's transpose takes 66 KB), so that at least two workgroups share a CU and one's
// split arithmetic runs under the other's MFMAs.
//
// Inf and NaN: the split of an Inf is Inf - Inf, and Inf times a zero mid / lo part of the other operand is NaN, so the split
// product cannot keep an Inf. Every thread tracks whether anything it staged was not finite; a block that saw such a value
// computes its tile again with v_mfma_f32_32x32x2_f32 straight from global memory, in conv_igemm_f32's order of additions:
// that tile then equals the exact kernel's bit for bit (Inf stays Inf, NaN stays NaN, finite stays finite).
//
// Prepared weights (YOLO_FLAG_SPLIT_WEIGHTS_READY, WREADY): inference weights stay the same from call to call, so
// split3_weights_f32 (yolo_split3_weights) splits the row-major section once, with s3_split. The prepared buffer is
//     [the packed weights as they are, padded to 16 bytes]
//     [K step][plane hi / mid / lo][cout_pad128][64 bytes]
//     [cout_pad128 / 32] 32-bit words,
// each 64-byte row with the slot swizzle above already applied (the row index is the output channel; blocks start at
// multiples of 64, so the channel's swizzle is the LDS row's). The BN rows a block needs of one (K step, plane) are BN * 64
// contiguous bytes and byte for byte the LDS image: the B side of a WREADY launch is a linear copy, 16 bytes per thread, with
// no split arithmetic and no chk. Word g of the table behind the planes is non-zero when a weight of output channels
// 32 g .. 32 g + 31 is an Inf or a NaN; a block ORs the words of its BN channels into its vote, so it takes the exact path
// exactly where the in-flight kernel does. The exact path reads its fp32 weights from the packed weights in front, as the
// in-flight kernel does. That copy in front is also what lets a packed buffer with room behind it be prepared in place: the same
// pointer then serves launches with and without the flag. 6 bytes per weight on top of the packed weights.
// WDMA moves the prepared B rows by LDS-DMA (global_load_lds, 16 bytes per lane) instead of through registers: a B ring of two
// slots, step kt + 1 requested at the top of step kt and retired by the vmcnt(0) in front of the barrier that ends the step.
// (One K step of A and B in flight, on every tile: two and three steps of A were built and measured; they gain nothing
// on 128x128 and 64x64 and cost the 128x64 tile its fourth workgroup.)
// 64x64 blocks have the two slots already (48 KB), a 128x128 block takes 72 KB with them (still two workgroups per CU), a 128x64
// block would take 48 KB and lose its fourth workgroup, so that tile copies through registers (ds_write_b128, 36 KB as before).
#include "conv_f32_epilogue.h"
#include "split3.h"
#include "wino_dma.h"      // wn_glds16_s, wn_wait_vmcnt

namespace yolo {

// The barriers of the K loop. A __syncthreads() is a fence too, and with LDS-DMA in the kernel the compiler makes that fence wait
// vmcnt(0): the barrier in the middle of a step would wait for the A and B requests of the next step, which only the end of the step
// needs. The WDMA kernels order their LDS traffic themselves: the wave's own LDS reads and writes are done, then the barrier; what
// has to have landed by DMA is waited for in front of the barrier that ends the step.
template <bool WDMA>
__device__ __forceinline__ void s3_sync() {
    if constexpr (WDMA) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
}

constexpr int S3_ROWB = 64;      // bytes per LDS row: 32 bf16 as four 16-byte slots, slot s of row r stored at s ^ ((r >> 2) & 3)

// byte offset, inside a plane of 64-byte rows, of the 8 bytes that hold k = 4 * chunk .. + 3 of row r
__device__ __forceinline__ int s3_row_off(int r, int chunk) { return r * S3_ROWB + (((chunk >> 1) ^ ((r >> 2) & 3)) * 16 + (chunk & 1) * 8); }

typedef __attribute__((address_space(3))) void* s3_lptr;

// Prepared weights of yolo_split3_weights: one block per 32 output channels, the staging geometry of conv_split3_f32 (thread =
// row tid >> 3, 16-byte chunk tid & 7 of every K step), so that the bytes written are the ones store_lds would have written.
struct S3PrepArgs {
    const float* w;      // row-major section of the packed weights [cout_pad128][Kpad]
    char* out;           // the planes (behind the packed weights of the prepared buffer)
    int Kpad, KT, cp;    // cp = cout_pad128
};

__global__ __launch_bounds__(256) void split3_weights_f32(const S3PrepArgs p) {
    const int tid = threadIdx.x;
    const int chunk = tid & 7;
    const int n = blockIdx.x * 32 + (tid >> 3);
    const size_t plane_b = (size_t)p.cp * S3_ROWB;
    const float* src = p.w + (size_t)n * p.Kpad + chunk * 4;
    char* dst = p.out + s3_row_off(n, chunk);
    f32x4 chk = {0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < p.KT; ++kt) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + kt * BK);
        u32x2 h, m, l;
        s3_split(v, h, m, l, chk);
        char* d = dst + (size_t)kt * 3 * plane_b;
        *reinterpret_cast<u32x2*>(d) = h;
        *reinterpret_cast<u32x2*>(d + plane_b) = m;
        *reinterpret_cast<u32x2*>(d + 2 * plane_b) = l;
    }
    const bool nonfinite = chk[0] != chk[0] || chk[1] != chk[1] || chk[2] != chk[2] || chk[3] != chk[3];
    const int any = __syncthreads_or(nonfinite);
    if (tid == 0) reinterpret_cast<unsigned*>(p.out + (size_t)p.KT * 3 * plane_b)[blockIdx.x] = any ? 1u : 0u;
}

// WREADY: p.w_planes points at the planes of the prepared buffer above, whose front p.w is. WDMA (with WREADY): its rows go to LDS by LDS-DMA.
template <int BM, int BN, bool WREADY, bool WDMA>
__global__ __launch_bounds__(256, 2) void conv_split3_f32(const ConvArgs p) {
    static_assert(WREADY || !WDMA, "LDS-DMA needs the prepared weights");
    constexpr int WM = BM / 2, WN = BN / 2;      // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;    // 32x32 MFMA tiles per wave
    constexpr int RA = BM / 32, RB = BN / 32;    // rows staged per thread
    constexpr bool DBUF = BM + BN <= 128;
    constexpr int A_BYTES = 3 * BM * S3_ROWB;                    // [3][BM][64 bytes]
    constexpr int B_BYTES = 3 * BN * S3_ROWB;                    // [3][BN][64 bytes]
    constexpr int BUF_BYTES = A_BYTES + B_BYTES;                 // A planes, then B planes
    constexpr bool BRING = DBUF || WDMA;                         // B has two slots: both buffers, or (one A buffer) a ring behind A
    constexpr int B_SLOT = DBUF ? BUF_BYTES : B_BYTES;           // B slot s starts at A_BYTES + s * B_SLOT
    constexpr int PB = BN / 64;                                  // prepared B: 16-byte pieces per thread and plane
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tile_n = blockIdx.x % p.tiles_n;
    const int tile_m = blockIdx.x / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int HoWo = p.Ho * p.Wo;

    // base address and tap mask of output pixel m (conv_igemm_f32's)
    auto row_geom = [&](int m, long long& base, unsigned& mask) {
        const bool mv = m < p.M;
        const int mm = mv ? m : 0;
        const int n = mm / HoWo;
        const int rem = mm - n * HoWo;
        const int ho = rem / p.Wo;
        const int wo = rem - ho * p.Wo;
        const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
        base = ((long long)(n * p.H + hi0) * p.W + wi0) * p.x_ld + p.x_off;
        unsigned mk = 0;
        for (int kh = 0; kh < p.ks; ++kh)
            for (int kw = 0; kw < p.ks; ++kw)
                if (mv && (unsigned)(hi0 + kh) < (unsigned)p.H && (unsigned)(wi0 + kw) < (unsigned)p.W)
                    mk |= 1u << (kh * p.ks + kw);
        mask = mk;
    };

    // ---------------------------------------------------------------- staging geometry
    const int chunk = tid & 7;       // 16-byte chunk inside the 32-float K step
    const int lrow = tid >> 3;       // 0..31
    long long a_base[RA];
    unsigned a_mask[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) row_geom(m0 + lrow + 32 * i, a_base[i], a_mask[i]);
    const float* wrow = p.w + (size_t)(n0 + lrow) * p.Kpad + chunk * 4;
    // prepared weights: plane (kt, q) of this block is BN * 64 contiguous bytes, thread tid copies bytes 16 * tid .. + 15 of every 4 KB
    const char* wq = p.w_planes;
    const size_t plane_b = (size_t)((p.Cout + 127) & ~127) * S3_ROWB;
    const char* wsrc = wq + (size_t)n0 * S3_ROWB + tid * 16;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);          // the same address as wave-uniform base + 16 lane
    const char* wdma_src = wq + (size_t)n0 * S3_ROWB + wave_u * 1024;
    const unsigned wdma_dst = (unsigned)(size_t)(s3_lptr)smem_raw + A_BYTES + wave_u * 1024;

    f32x4 ra[RA], rb[RB];
    unsigned av;                     // bit i: row i of what ra holds is a tap inside the image (the others are zeroed when it is split)
    s3_u32x4 rw[3][PB];
    f32x4 chk = {0.f, 0.f, 0.f, 0.f};
    // A of step kt: RA loads, every one issued whatever the tap (a padding tap reads the first pixel of the view, and store_lds puts
    // zeros in its place): no branch around a load, and nothing here uses a loaded value, so nothing waits before the products.
    auto load_a = [&](int kt) {
        const int kg = kt * BK;
        const int tap = kg / p.Cin;
        const int coff = kg - tap * p.Cin + chunk * 4;
        const int kh = tap / p.ks, kw = tap - kh * p.ks;
        const long long toff = (long long)(kh * p.W + kw) * p.x_ld + coff;
        unsigned valid = 0;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const bool v = (a_mask[i] >> tap) & 1u;
            valid |= (unsigned)v << i;
            ra[i] = *reinterpret_cast<const f32x4*>(p.x + (v ? a_base[i] + toff : (long long)p.x_off + coff));
        }
        av = valid;
    };
    auto load_b = [&](int kt) {
        if constexpr (!WREADY) {
#pragma unroll
            for (int i = 0; i < RB; ++i)
                rb[i] = *reinterpret_cast<const f32x4*>(wrow + (size_t)(32 * i) * p.Kpad + kt * BK);
        } else {
            const char* src = wsrc + (size_t)kt * 3 * plane_b;
            // WDMA: the wave's KB of every 4, lane l lands 16 l in. The request is wn_glds16_s's text, not the builtin: while a
            // request that the compiler knows of is pending, every vmcnt it needs for the A registers becomes vmcnt(0) (it takes
            // an LDS-DMA for a flat access that may return out of order). B is requested before A, so the counts that the compiler
            // makes for the A registers without knowing of these requests cover them: loads return in order.
            const char* dsrc = wdma_src + (size_t)kt * 3 * plane_b;
            const unsigned dst = wdma_dst + (kt & 1) * B_SLOT;
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < PB; ++i) {
                    if constexpr (WDMA)
                        wn_glds16_s(dsrc + q * plane_b + i * 4096, lane * 16, dst + q * BN * S3_ROWB + i * 4096);
                    else
                        rw[q][i] = *reinterpret_cast<const s3_u32x4*>(src + q * plane_b + i * 4096);
                }
        }
    };
    auto store_lds = [&](int buf, int bslot) {
        char* a = smem_raw + buf * BUF_BYTES + s3_row_off(lrow, chunk);
        char* b = smem_raw + A_BYTES + bslot * B_SLOT + s3_row_off(lrow, chunk);
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            u32x2 h, m, l;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            s3_split((av >> i) & 1u ? ra[i] : z, h, m, l, chk);
            *reinterpret_cast<u32x2*>(a + (0 * BM + 32 * i) * S3_ROWB) = h;
            *reinterpret_cast<u32x2*>(a + (1 * BM + 32 * i) * S3_ROWB) = m;
            *reinterpret_cast<u32x2*>(a + (2 * BM + 32 * i) * S3_ROWB) = l;
        }
        if constexpr (!WREADY) {
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                u32x2 h, m, l;
                s3_split(rb[i], h, m, l, chk);
                *reinterpret_cast<u32x2*>(b + (0 * BN + 32 * i) * S3_ROWB) = h;
                *reinterpret_cast<u32x2*>(b + (1 * BN + 32 * i) * S3_ROWB) = m;
                *reinterpret_cast<u32x2*>(b + (2 * BN + 32 * i) * S3_ROWB) = l;
            }
        } else if constexpr (!WDMA) {
            char* bw = smem_raw + A_BYTES + bslot * B_SLOT + tid * 16;
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < PB; ++i) *reinterpret_cast<s3_u32x4*>(bw + q * BN * S3_ROWB + i * 4096) = rw[q][i];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment reads: lane l -> row (l & 31), k = 8 * (l >> 5) .. + 7 of each 16-wide chunk
    const int frow = lane & 31, fh = lane >> 5;
    const int a_frag = (wm * WM + frow) * S3_ROWB;
    const int b_frag = A_BYTES + (wn * WN + frow) * S3_ROWB;       // in B slot 0
    const int fsw = (frow >> 2) & 3;                       // the swizzle of this lane's rows (the same in every 32-row tile)
    const int f_slot[2] = {(fh ^ fsw) * 16, ((2 + fh) ^ fsw) * 16};

    // One K step. MORE: step kt + 1 exists; its B and then its A are requested at the top and split / stored at the end. MORE is a
    // constant of the text (the loop runs the steps that ask, the last step is written out behind it), so that the requests, the
    // split and the waits of a step sit in one block that the scheduler orders as a whole.
    auto step = [&](auto MORE, int kt) {
        constexpr bool more = decltype(MORE)::value;
        const int cur = DBUF ? (kt & 1) : 0;
        const int bcur = BRING ? (kt & 1) : 0;
        if constexpr (more) {
            load_b(kt + 1);                          // (WDMA: B slot bcur ^ 1 was last read in step kt - 1, behind that step's barrier)
            load_a(kt + 1);
        }
        __builtin_amdgcn_sched_barrier(0);           // the requests go out before the products ...
        const char* Ab = smem_raw + cur * BUF_BYTES + a_frag;
        const char* Bb = smem_raw + bcur * B_SLOT + b_frag;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            s3_bf16x8 af[TM][3], bf[TN][3];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    af[i][q] = *reinterpret_cast<const s3_bf16x8*>(Ab + (q * BM + i * 32) * S3_ROWB + f_slot[c]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    bf[j][q] = *reinterpret_cast<const s3_bf16x8*>(Bb + (q * BN + j * 32) * S3_ROWB + f_slot[c]);
            // (a part, b part) with 0 = hi, 1 = mid, 2 = lo: smallest terms first, the same order everywhere
            constexpr int QA[6] = {0, 2, 1, 0, 1, 0};
            constexpr int QB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][QA[t]], bf[j][QB[t]], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);           // ... and the split, which has to wait for them, stays behind the products
        if (!DBUF) s3_sync<WDMA>();                  // one buffer: everybody has read step kt before step kt + 1 lands
        if constexpr (more) store_lds(DBUF ? (cur ^ 1) : 0, BRING ? (bcur ^ 1) : 0);
        if constexpr (WDMA) wn_wait_vmcnt<0>();      // the DMA of step kt + 1 has landed before the barrier
        s3_sync<WDMA>();
    };

    load_b(0);
    load_a(0);
    store_lds(0, 0);
    if constexpr (WDMA) wn_wait_vmcnt<0>();
    s3_sync<WDMA>();

    for (int kt = 0; kt + 1 < p.KT; ++kt) step(std::true_type{}, kt);
    step(std::false_type{}, p.KT - 1);

    // A block that staged an Inf or a NaN computes its tile again with exact f32 products, straight from global memory (rare, so
    // slow is fine) and in conv_igemm_f32's order: k = 8 s + 4 (l >> 5) + e for MFMA (s, e) of each K step.
    // The whole block goes that way, the rows of a neighbouring image that share it included: their finite outputs then carry the
    // exact kernel's bits instead of the split products' (batch independence holds for finite data).
    bool nonfinite = chk[0] != chk[0] || chk[1] != chk[1] || chk[2] != chk[2] || chk[3] != chk[3];
    if constexpr (WREADY) {                      // chk saw the A side only: the weights' vote was taken when they were prepared
        const unsigned* table = reinterpret_cast<const unsigned*>(wq + (size_t)p.KT * 3 * plane_b);
#pragma unroll
        for (int g = 0; g < BN / 32; ++g) nonfinite |= table[n0 / 32 + g] != 0;
    }
    if (__syncthreads_or(nonfinite)) {
        long long f_base[TM];
        unsigned f_mask[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) row_geom(m0 + wm * WM + i * 32 + frow, f_base[i], f_mask[i]);
        const float* fw = p.w + (size_t)(n0 + wn * WN + frow) * p.Kpad + 4 * fh;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        for (int kt = 0; kt < p.KT; ++kt) {
            const int kg = kt * BK;
            const int tap = kg / p.Cin;
            const int kh = tap / p.ks, kw = tap - kh * p.ks;
            const long long toff = (long long)(kh * p.W + kw) * p.x_ld + (kg - tap * p.Cin) + 4 * fh;
            for (int s = 0; s < 4; ++s) {
                f32x4 af[TM], bf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    af[i] = ((f_mask[i] >> tap) & 1u) ? *reinterpret_cast<const f32x4*>(p.x + f_base[i] + toff + s * 8) : z;
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(fw + (size_t)(32 * j) * p.Kpad + kg + s * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
            }
        }
    }

    conv_f32_epilogue<BM, BN>(p, acc, reinterpret_cast<float*>(smem_raw), m0, n0);   // [BM][BN + 4] floats, idle behind the barrier
}

// ------------------------------------------------------------------------------ host side
bool split3_supported(const yolo_conv_desc* d) {
    return d->dtype == YOLO_F32 && (d->ksize == 1 || d->ksize == 3) && (d->stride == 1 || d->stride == 2) && d->cin % 32 == 0;
}

template <int BM, int BN, bool WREADY, bool WDMA>
static int launch_split3(const ConvArgs& a, hipStream_t s) {
    constexpr bool dbuf = BM + BN <= 128;
    constexpr size_t operands = dbuf ? (size_t)2 * 3 * (BM + BN) * S3_ROWB : (size_t)3 * (BM + (WDMA ? 2 : 1) * BN) * S3_ROWB;
    constexpr size_t transpose = (size_t)BM * (BN + 4) * sizeof(float);
    constexpr size_t lds = operands > transpose ? operands : transpose;
    ConvArgs p = a;
    p.tiles_n = ceil_div(a.Cout, BN);
    const long long blocks = (long long)ceil_div(a.M, BM) * p.tiles_n;
    if (blocks > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "conv_split3_f32: too many blocks");
    if (lds > 64 * 1024) {
        static LdsOnce once;
        if (int rc = reserve_lds(once, reinterpret_cast<const void*>(&conv_split3_f32<BM, BN, WREADY, WDMA>), lds, "conv_split3_f32")) return rc;
    }
    hipLaunchKernelGGL((conv_split3_f32<BM, BN, WREADY, WDMA>), dim3((unsigned)blocks), dim3(256), lds, s, p);
    return check_launch("conv_split3_f32");
}

// How a launch on prepared weights moves them into LDS, per tile (batch 32, medians in us, profiles/r07/conv_bench_regs.txt and
// conv_bench_dma.txt). 128x128 and 64x64: LDS-DMA, 6 - 13 % under the in-flight kernel on the stride-2 layers and up to 22 % at
// 13 x 13, where registers gain 0 - 5 %. 128x64: registers. Its DMA ring takes 48 KB, three workgroups per CU instead of four, and
// loses 3 - 8 % on the launches with few K steps (64 -> 32 at 208 x 208, the 52 x 52 head, 32 -> 64 3x3); registers are level
// with the in-flight kernel there (0 - 2 %, inside the spread) and never behind it.
constexpr bool kS3Dma128x128 = true, kS3Dma128x64 = false, kS3Dma64x64 = true;

template <int BM, int BN, bool WDMA>
static int launch_split3(const ConvArgs& a, hipStream_t s) {
    return a.w_planes ? launch_split3<BM, BN, true, WDMA>(a, s) : launch_split3<BM, BN, false, false>(a, s);
}

// ---- prepared weights (yolo_split3_weights): layout in the comment at the top of this file
size_t split3_weight_bytes(const yolo_conv_desc* d) {
    const size_t cp = coutpad_of(d->cout), KT = kpad_of(d->cin, d->ksize) / BK;
    return packed_f32(d->cout, d->cin, d->ksize).tail_bytes + KT * 3 * cp * S3_ROWB + cp / 32 * sizeof(unsigned);
}

int split3_weights_launch(const yolo_conv_desc* d, const void* w_packed, void* out, hipStream_t s) {
    const size_t off = packed_f32(d->cout, d->cin, d->ksize).tail_bytes;
    if (out != w_packed) {                           // not in place: the packed weights go in front
        const char *a = static_cast<const char*>(w_packed), *b = static_cast<const char*>(out);
        if (a < b + split3_weight_bytes(d) && b < a + off) return fail(YOLO_ERR_ARG, "yolo_split3_weights: out overlaps w_packed (pass the same pointer to prepare in place)");
        if (hipMemcpyAsync(out, w_packed, off, hipMemcpyDeviceToDevice, s) != hipSuccess) return check_launch("yolo_split3_weights: copy");
    }
    S3PrepArgs p;
    p.w = static_cast<const float*>(w_packed);
    p.out = static_cast<char*>(out) + off;
    p.Kpad = kpad_of(d->cin, d->ksize);
    p.KT = p.Kpad / BK;
    p.cp = coutpad_of(d->cout);
    hipLaunchKernelGGL(split3_weights_f32, dim3(p.cp / 32), dim3(256), 0, s, p);
    return check_launch("split3_weights_f32");
}

// Tile of the heuristic: the layer's shape only, never the batch. Measured at batch 32 (tools/conv_bench.py --split3 /
// --split3-ready --tile 1,2,4, medians in us).
// Weights split in flight (profiles/r06/conv_bench_split3.txt). Stride-2 3x3: 128x128 wins with 64 .. 256 input channels (349 /
// 323 / 353 against 379 / 353 / 363 for 128x64), 128x64 wins 32 -> 64 at 416 x 416 (cout 64: half a 128-wide block would be
// padding) and 512 -> 1024 at 26 x 26 (348 against 381). 1x1: 128x64 wins wherever it makes enough blocks; the launches with
// h * w * cout below 100,000 (256 -> 128 at 26 x 26, 1024 -> 512 at 13 x 13: 338 / 344 blocks of 128x64 at batch 32 on 256 CUs)
// run faster as twice as many 64x64 blocks (20.2 against 24.1, 54.1 against 65.2). 64x64 wins nowhere else.
// Prepared weights (profiles/r07/conv_bench_ready.txt): the B side of a 128x128 block is a DMA and A's split is shared by 128
// columns, so 128x128 also wins 512 -> 1024 stride 2 at 26 x 26 (345 against 357) and the 1x1 layers with a multiple of 128 output
// channels and many K steps: 256 -> 128 and 384 -> 128 at 52 x 52 (46.4 / 63.0 against 49.8 / 68.9), 768 -> 256 at 26 x 26 (64.9
// against 65.8). 512 -> 256 at 26 x 26 (46.6 against 47.2) gains less than its own spread and stays.
// Fitted again after the K step was rewritten (profiles/split3_ahead/conv_bench.txt: every tile 2 - 5 % faster, in step): the
// same choices. 128x128 / 128x64 / 64x64 now: stride 2 with 64 .. 512 channels 305 / 354 / 395, 283 / 331 / 368, 294 / 338 / 359, 322 /
// 336 / 356; 256 -> 128 and 384 -> 128 at 52 x 52 43.8 / 46.4 and 59.7 / 65.2; 768 -> 256 at 26 x 26 60.6 / 63.1; 512 -> 256 at 26 x 26 43.9 /
// 44.4, still inside its spread; 1024 -> 512 at 13 x 13 53.6 / 53.8 / 44.7.
static int pick_split3_tile(const ConvArgs& a, bool ready) {
    if (a.ks == 3 && a.stride == 2 && a.Cin >= 64 && (ready || a.Cin < 512)) return kTileF32Reg128x128;
    if (a.ks == 1 && (long long)a.H * a.W * a.Cout < 100000) return kTileF32Reg64x64;
    if (ready && a.ks == 1 && a.Cout % 128 == 0 && a.Cin >= ((long long)a.H * a.W >= 52 * 52 ? 256 : 768)) return kTileF32Reg128x128;
    return kTileF32Reg128x64;
}

// Shapes that the eval plan runs on this kernel: the supported ones whose median at batch 32 improved by more than the spread of
// their own baseline (profiles/r06/conv_bench_split3.txt, profiles/r07/conv_bench_ready.txt). The five stride-2 3x3 layers gain
// 20 - 34 %, 32 -> 64 3x3 stride 1 at 208 x 208 gains 11 % on conv_patch_f32 (smaller maps of that layer were not measured and
// stay), the 1x1 layers and heads with h * w * cout >= 80,000 gain 11 - 28 %. The two 13 x 13 launches below that (512 -> 256 and
// the 1024 -> 255 head, 43,000: 340 blocks of 64x64 at batch 32) were level with the exact kernel while every block split its
// weights; on prepared weights they gain 17 % and 22 %, so the bound is 40,000 now. Nothing smaller was measured.
bool split3_eligible(const yolo_conv_desc* d) {
    if (!split3_supported(d)) return false;
    if (d->ksize == 3) return d->stride == 2 || (d->cin == 32 && (long long)d->h * d->w >= 208 * 208);
    return d->stride == 1 && (long long)d->h * d->w * d->cout >= 40000;
}

int conv_split3_launch(const ConvArgs& a, int tile, hipStream_t s) {
    switch (tile ? tile : pick_split3_tile(a, a.w_planes != nullptr)) {
    case kTileF32Reg128x128: return launch_split3<128, 128, kS3Dma128x128>(a, s);
    case kTileF32Reg128x64: return launch_split3<128, 64, kS3Dma128x64>(a, s);
    case kTileF32Reg64x64: return launch_split3<64, 64, kS3Dma64x64>(a, s);
    default: return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_BF16 has tiles 1 (128x128), 2 (128x64) and 4 (64x64), not %d", tile);
    }
}

}  // namespace yolo
