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
#include "conv_f32_epilogue.h"

namespace yolo {

typedef __bf16 s3_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int s3_u32x4 __attribute__((ext_vector_type(4)));

constexpr int S3_ROWB = 64;      // bytes per LDS row: 32 bf16 as four 16-byte slots, slot s of row r stored at s ^ ((r >> 2) & 3)

// two floats' upper halves as one bf16 pair, `a` in the low half (the lower k)
__device__ __forceinline__ unsigned s3_pack(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

// v = hi + mid + lo exactly, each with 8 significand bits; chk turns NaN when v holds an Inf or a NaN
__device__ __forceinline__ void s3_split(const f32x4 v, u32x2& hi, u32x2& mid, u32x2& lo, f32x4& chk) {
    const s3_u32x4 vb = __builtin_bit_cast(s3_u32x4, v);
    const f32x4 h = __builtin_bit_cast(f32x4, vb & 0xffff0000u);
    const f32x4 r1 = v - h;
    const s3_u32x4 r1b = __builtin_bit_cast(s3_u32x4, r1);
    const f32x4 m = __builtin_bit_cast(f32x4, r1b & 0xffff0000u);
    const f32x4 r2 = r1 - m;
    const s3_u32x4 r2b = __builtin_bit_cast(s3_u32x4, r2);
    chk += r2 * 0.f;
    hi[0] = s3_pack(vb[0], vb[1]); hi[1] = s3_pack(vb[2], vb[3]);
    mid[0] = s3_pack(r1b[0], r1b[1]); mid[1] = s3_pack(r1b[2], r1b[3]);
    lo[0] = s3_pack(r2b[0], r2b[1]); lo[1] = s3_pack(r2b[2], r2b[3]);
}

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void conv_split3_f32(const ConvArgs p) {
    constexpr int WM = BM / 2, WN = BN / 2;      // wave tile
    constexpr int TM = WM / 32, TN = WN / 32;    // 32x32 MFMA tiles per wave
    constexpr int RA = BM / 32, RB = BN / 32;    // rows staged per thread
    constexpr bool DBUF = BM + BN <= 128;
    constexpr int A_BYTES = 3 * BM * S3_ROWB;                    // [3][BM][64 bytes]
    constexpr int BUF_BYTES = 3 * (BM + BN) * S3_ROWB;           // A planes, then B planes [3][BN][64 bytes]
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

    f32x4 ra[RA], rb[RB];
    f32x4 chk = {0.f, 0.f, 0.f, 0.f};
    auto load_global = [&](int kt) {
        const int kg = kt * BK;
        const int tap = kg / p.Cin;
        const int coff = kg - tap * p.Cin + chunk * 4;
        const int kh = tap / p.ks, kw = tap - kh * p.ks;
        const long long toff = (long long)(kh * p.W + kw) * p.x_ld + coff;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const bool v = (a_mask[i] >> tap) & 1u;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            ra[i] = v ? *reinterpret_cast<const f32x4*>(p.x + a_base[i] + toff) : z;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i)
            rb[i] = *reinterpret_cast<const f32x4*>(wrow + (size_t)(32 * i) * p.Kpad + kt * BK);
    };
    auto store_lds = [&](int buf) {
        char* a = smem_raw + buf * BUF_BYTES + lrow * S3_ROWB + (((chunk >> 1) ^ ((lrow >> 2) & 3)) * 16 + (chunk & 1) * 8);
        char* b = a + A_BYTES;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            u32x2 h, m, l;
            s3_split(ra[i], h, m, l, chk);
            *reinterpret_cast<u32x2*>(a + (0 * BM + 32 * i) * S3_ROWB) = h;
            *reinterpret_cast<u32x2*>(a + (1 * BM + 32 * i) * S3_ROWB) = m;
            *reinterpret_cast<u32x2*>(a + (2 * BM + 32 * i) * S3_ROWB) = l;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            u32x2 h, m, l;
            s3_split(rb[i], h, m, l, chk);
            *reinterpret_cast<u32x2*>(b + (0 * BN + 32 * i) * S3_ROWB) = h;
            *reinterpret_cast<u32x2*>(b + (1 * BN + 32 * i) * S3_ROWB) = m;
            *reinterpret_cast<u32x2*>(b + (2 * BN + 32 * i) * S3_ROWB) = l;
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
    const int b_frag = A_BYTES + (wn * WN + frow) * S3_ROWB;
    const int fsw = (frow >> 2) & 3;                       // the swizzle of this lane's rows (the same in every 32-row tile)
    const int f_slot[2] = {(fh ^ fsw) * 16, ((2 + fh) ^ fsw) * 16};

    load_global(0);
    store_lds(0);
    __syncthreads();

    for (int kt = 0; kt < p.KT; ++kt) {
        const int cur = DBUF ? (kt & 1) : 0;
        const bool more = kt + 1 < p.KT;
        if (more) load_global(kt + 1);
        const char* Ab = smem_raw + cur * BUF_BYTES + a_frag;
        const char* Bb = smem_raw + cur * BUF_BYTES + b_frag;
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
        if (!DBUF) __syncthreads();              // one buffer: everybody has read step kt before step kt + 1 lands
        if (more) store_lds(DBUF ? (cur ^ 1) : 0);
        __syncthreads();
    }

    // A block that staged an Inf or a NaN computes its tile again with exact f32 products, straight from global memory (rare, so
    // slow is fine) and in conv_igemm_f32's order: k = 8 s + 4 (l >> 5) + e for MFMA (s, e) of each K step.
    // The whole block goes that way, the rows of a neighbouring image that share it included: their finite outputs then carry the
    // exact kernel's bits instead of the split products' (batch independence holds for finite data).
    const bool nonfinite = chk[0] != chk[0] || chk[1] != chk[1] || chk[2] != chk[2] || chk[3] != chk[3];
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

template <int BM, int BN>
static int launch_split3(const ConvArgs& a, hipStream_t s) {
    constexpr size_t operands = (size_t)(BM + BN <= 128 ? 2 : 1) * 3 * (BM + BN) * S3_ROWB;
    constexpr size_t transpose = (size_t)BM * (BN + 4) * sizeof(float);
    constexpr size_t lds = operands > transpose ? operands : transpose;
    ConvArgs p = a;
    p.tiles_n = ceil_div(a.Cout, BN);
    const long long blocks = (long long)ceil_div(a.M, BM) * p.tiles_n;
    if (blocks > 0x7fffffffLL) return fail(YOLO_ERR_UNSUPPORTED, "conv_split3_f32: too many blocks");
    if (lds > 64 * 1024) {
        static LdsOnce once;
        if (int rc = reserve_lds(once, reinterpret_cast<const void*>(&conv_split3_f32<BM, BN>), lds, "conv_split3_f32")) return rc;
    }
    hipLaunchKernelGGL((conv_split3_f32<BM, BN>), dim3((unsigned)blocks), dim3(256), lds, s, p);
    return check_launch("conv_split3_f32");
}

// Tile of the heuristic: the layer's shape only, never the batch. Measured at batch 32 (tools/conv_bench.py --split3 --tile 1,2,4,
// profiles/r06/conv_bench_split3.txt, medians in us). Stride-2 3x3: 128x128 wins with 64 .. 256 input channels (349 / 323 / 353
// against 379 / 353 / 363 for 128x64), 128x64 wins 32 -> 64 at 416 x 416 (cout 64: half a 128-wide block would be padding) and
// 512 -> 1024 at 26 x 26 (348 against 381). 1x1: 128x64 wins wherever it makes enough blocks; the launches with h * w * cout below
// 100,000 (256 -> 128 at 26 x 26, 1024 -> 512 at 13 x 13: 338 / 344 blocks of 128x64 at batch 32 on 256 CUs) run faster as twice
// as many 64x64 blocks (20.2 against 24.1, 54.1 against 65.2). 64x64 wins nowhere else.
static int pick_split3_tile(const ConvArgs& a) {
    if (a.ks == 3 && a.stride == 2 && a.Cin >= 64 && a.Cin < 512) return kTileF32Reg128x128;
    if (a.ks == 1 && (long long)a.H * a.W * a.Cout < 100000) return kTileF32Reg64x64;
    return kTileF32Reg128x64;
}

// Shapes that the eval plan runs on this kernel: the supported ones whose median at batch 32 improved by more than the spread of
// their own baseline (profiles/r06/conv_bench_split3.txt). The five stride-2 3x3 layers gain 20 - 31 %, 32 -> 64 3x3 stride 1 at
// 208 x 208 gains 11 % on conv_patch_f32 (smaller maps of that layer were not measured and stay), the 1x1 layers and heads with
// h * w * cout >= 80,000 gain 11 - 25 %. The two 13 x 13 launches below that (512 -> 256 and the 1024 -> 255 head, 43,000) are
// 340 blocks of 64x64 at batch 32 and level with the exact kernel (-3.7 % and -0.2 %): they stay.
bool split3_eligible(const yolo_conv_desc* d) {
    if (!split3_supported(d)) return false;
    if (d->ksize == 3) return d->stride == 2 || (d->cin == 32 && (long long)d->h * d->w >= 208 * 208);
    return d->stride == 1 && (long long)d->h * d->w * d->cout >= 80000;
}

int conv_split3_launch(const ConvArgs& a, int tile, hipStream_t s) {
    switch (tile ? tile : pick_split3_tile(a)) {
    case kTileF32Reg128x128: return launch_split3<128, 128>(a, s);
    case kTileF32Reg128x64: return launch_split3<128, 64>(a, s);
    case kTileF32Reg64x64: return launch_split3<64, 64>(a, s);
    default: return fail(YOLO_ERR_UNSUPPORTED, "conv: YOLO_FLAG_SPLIT_BF16 has tiles 1 (128x128), 2 (128x64) and 4 (64x64), not %d", tile);
    }
}

}  // namespace yolo
