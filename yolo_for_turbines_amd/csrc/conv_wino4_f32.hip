// conv_wino4_f32.hip — the fp32 3x3 stride-1 blocks on large maps by Winograd F(4x4, 3x3):
//
//     Y = A^T [ (G g G^T) .* (B^T d B) ] A            per 6x6 input tile d (stride 4), 3x3 filter g, 4x4 output tile Y
//
// 36 multiplications per 16 outputs and (ci, co) pair instead of F(2x2)'s 16 per 4: the matrix cores execute 0.5625x the
// work of conv_wino_f32.hip, and the transformed input V4 is 2.25x the activation instead of 4x. Interpolation points
// (0, 1, -1, 2, -1/2, inf) instead of the textbook (0, +-1, +-2, inf): the fp32 error of the transforms is ~4x smaller
// (max|err| / max|y| ~3e-6 against an fp64 convolution at K = 128 .. 256). From the points:
//   A^T[i][j] = p_j^i (the column of inf is e_3), G[j][k] = p_j^k / prod_{l != j} (p_j - p_l) (the row of inf is e_2), and
//   B^T solves sum_j A^T[i][j] G[j][k] B^T[j][l] = delta(l, i + k). A^T and B^T hold dyadic fractions only (exact in fp32);
//   G holds thirds and fifteenths: the filter transform runs in fp64 and rounds once.
//
// Two kernels per launch:
//   wino4_xform_f32  V4[xi][c4][tile_pad64][4] = (B^T d B)[xi] for every 6x6 input tile, xi = 6a + b, c4 running to C4p (= C4
//                    rounded up to even, the padding plane zero); the blocks behind the input transform write
//                    U4[xi][c4][co_pad64][4] = (G g G^T)[xi] from the row-major section at the start of the packed weights
//                    (yolo_pack_weights, and yolo_pack_weights_dgrad with flip = 1 for the stride-1 input gradient). U4 is
//                    computed per launch and lives in the workspace behind V4: the packed weight format stays as it is.
//                    Inference, whose weights stay the same from call to call, makes U4 once instead (wino4_filters_f32 through
//                    yolo_wino4_filters, YOLO_FLAG_FILTERS_READY): the launch then has no filter blocks.
//                    wino4_xform_f32<true> (YOLO_FLAG_WINO_SPLIT_BF16) writes the same V4, and the caller's finished U4, as bf16 planes
//                    for conv_wino4s_f32.hip instead (wino4_planes.h); where the caller keeps the filter planes too
//                    (YOLO_FLAG_FILTER_PLANES, made once by yolo_wino4_filter_planes) its trailing blocks only read them ahead.
//   conv_wino4_f32   per workgroup 64 tiles x 64 output channels (the block of conv_wino_f32: the same operand bytes per MFMA, so
//                    the same LDS-DMA price per matrix cycle): 36 GEMMs D_xi[co][tile] = sum_ci U4_xi[co][ci] V4_xi[tile][ci] in SIX
//                    passes over K, one row a of the 6x6 product matrix M per pass (xi = 6a .. 6a + 5). Y = A^T M A is linear in the
//                    rows of M, so each pass folds its row into the 4x4 output tiles right away (t = M[a][.] A, Y += A^T[.][a] t^T)
//                    and only those partial tiles survive a pass. 8 waves, two per SIMD; a wave owns 32 tiles x 16 channels as two
//                    16 x 16 blocks of v_mfma_f32_16x16x4_f32 per xi: 48 accumulators per pass (VGPRs), 128 partial-tile registers
//                    (parked in the AGPR half between passes). A stage is 8 channels = two planes x 6 xi x (V, U) = 24 KiB.
//                    Epilogue: BN scale / shift, activation, residual, ld / off views and the NaN flag as in conv_wino_f32,
//                    staged through LDS one output row of the tile at a time; the residual is requested one row ahead.
//                    One workgroup per CU and round: the tile blocks of a last round that would fill at most half the CUs run as
//                    two workgroups of 32 tiles each (wino4_whole_blocks), the same 16 x 16 MFMA blocks in the same order on half
//                    the waves, so a tile's bits do not depend on the cut.
#include "split3.h"
#include "wino4_planes.h"
#include "wino4_epilogue.h"

namespace yolo {

// points (0, 1, -1, 2, -1/2, inf)
__device__ constexpr float W4_BT[6][6] = {
    {1.f, 1.5f, -2.f, -1.5f, 1.f, 0.f},
    {0.f, -1.f, -2.5f, -0.5f, 1.f, 0.f},
    {0.f, 1.f, 0.5f, -2.5f, 1.f, 0.f},
    {0.f, -0.5f, -1.f, 0.5f, 1.f, 0.f},
    {0.f, 2.f, -1.f, -2.f, 1.f, 0.f},
    {0.f, 1.f, 1.5f, -2.f, -1.5f, 1.f},
};
__device__ constexpr double W4_G[6][3] = {
    {1.0, 0.0, 0.0},
    {-1.0 / 3, -1.0 / 3, -1.0 / 3},
    {1.0 / 3, -1.0 / 3, 1.0 / 3},
    {1.0 / 15, 2.0 / 15, 4.0 / 15},
    {-16.0 / 15, 8.0 / 15, -4.0 / 15},
    {0.0, 0.0, 1.0},
};

// ------------------------------------------------------------------------------ transform pass: V4 = B^T d B, U4 = G g G^T
struct Wino4XArgs {
    const float* x;
    float* V;
    int H, W, C4, C4p;
    int x_ld, x_off;
    int th, tw, T, Tpad;
    int ncg;                 // channel groups of 32 (over C4p): the fastest-running part of blockIdx.x
    int nxb;                 // blocks of the input transform; the blocks behind them transform the filters
    const float* w;          // row-major section of the packed weights: [row co][(3 kh + kw) * cinp + ci], rows kpad apart
    float* U;
    int cout, cin, coutp, cinp, kpad;
    long long utotal;        // C4p * coutp * 4: one thread per (ci, co) pair computes all 36 xi
};

// U4 = G g G^T: element i = (c4, co, e) of every xi plane, for i = first, first + stride, ... One function for the per-launch
// blocks of wino4_xform_f32 and for wino4_filters_f32 (yolo_wino4_filters), so both write the same bits.
__device__ __forceinline__ void wino4_filter_elems(const Wino4XArgs& p, long long first, long long stride) {
    for (long long i = first; i < p.utotal; i += stride) {
        const int e = (int)(i & 3);
        const long long r = i >> 2;
        const int co = (int)(r % p.coutp), c4 = (int)(r / p.coutp);
        const int ci = 4 * c4 + e;
        double g[3][3];
        const bool ok = co < p.cout && ci < p.cin;
#pragma unroll
        for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = ok ? (double)p.w[(size_t)co * p.kpad + k * p.cinp + ci] : 0.0;
        double t[6][3];                                  // G g
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) t[j][q] = W4_G[j][0] * g[0][q] + W4_G[j][1] * g[1][q] + W4_G[j][2] * g[2][q];
        float* dst = p.U + i;
        const size_t xs = (size_t)p.C4p * p.coutp * 4;
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int l = 0; l < 6; ++l)
                dst[(6 * j + l) * xs] = (float)(t[j][0] * W4_G[l][0] + t[j][1] * W4_G[l][1] + t[j][2] * W4_G[l][2]);
    }
}

// the filters alone, once per weight update (yolo_wino4_filters): only w, U and the filter geometry of the arguments are read
__global__ __launch_bounds__(256) void wino4_filters_f32(const Wino4XArgs p) {
    wino4_filter_elems(p, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

// The same filters as bf16 planes (wino4_planes.h), from the finished fp32 U4 that p.w points at here, into p.U: element i =
// (xi, chunk, co, channel quad of the chunk), the quad running fastest so that eight threads write one 64-byte row of each plane
__device__ __forceinline__ void wino4_filter_planes(const Wino4XArgs& p, long long first, long long stride) {
    const int nkc = p.C4p / 8, n_nt = p.coutp / 64;
    char* out = reinterpret_cast<char*>(p.U);
    for (long long i = first; i < 9 * p.utotal; i += stride) {      // 36 xi x C4p x coutp
        const int q = (int)(i & 7);
        const long long r = i >> 3;
        const int co = (int)(r % p.coutp);
        const int kx = (int)(r / p.coutp), kc = kx % nkc, xi = kx / nkc;
        const f32x4 u = *reinterpret_cast<const f32x4*>(p.w + (((size_t)xi * p.C4p + 8 * kc + q) * p.coutp + co) * 4);
        u32x2 h, m, l;
        f32x4 chk = {0.f, 0.f, 0.f, 0.f};
        s3_split(u, h, m, l, chk);
        char* d = out + w4s_offset(xi, 32 * kc + 4 * q, co, 0, nkc, n_nt);
        *reinterpret_cast<u32x2*>(d) = h;
        *reinterpret_cast<u32x2*>(d + W4S_PLANE) = m;
        *reinterpret_cast<u32x2*>(d + 2 * W4S_PLANE) = l;
    }
}

// Filter planes made once (YOLO_FLAG_FILTER_PLANES) lie in HBM when their layer's turn comes: a forward reads more filter bytes than
// the caches hold. conv_wino4s_f32 requested a stage three stages ahead, which covered the memory-side cache but not HBM (measured in
// the forward, DESIGN 4.15: 151 against 114 us at 26 x 26); it now requests five ahead and the forward without these reads is still
// 0.4 ms slower. So the blocks behind the input transform read the planes once, one dword per 64 bytes, while the
// input is transformed: p.U points at them, element i = 64 bytes
__device__ __forceinline__ void wino4_touch_planes(const Wino4XArgs& p, long long first, long long stride) {
    const char* pl = reinterpret_cast<const char*>(p.U);
    const long long n = p.utotal * 27 / 8;                           // 36 xi x 6 bytes x utotal / 64
    for (long long i = first; i < n; i += stride) {
        unsigned v;
        asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(pl + i * 64) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// the filter planes alone, once per weight update (yolo_wino4_filter_planes): the same device function, so the same bytes
__global__ __launch_bounds__(256) void wino4_filter_planes_f32(const Wino4XArgs p) {
    wino4_filter_planes(p, (long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x);
}

// PLANES (YOLO_FLAG_WINO_SPLIT_BF16, C4 % 8 == 0): the same values v, each split into three bf16 (s3_split) and stored as the planes
// of wino4_planes.h in place of V4; the blocks behind the input transform split the caller's finished U4 the same way
template <bool PLANES>
__global__ __launch_bounds__(256) void wino4_xform_f32(const Wino4XArgs p) {
    if ((int)blockIdx.x >= p.nxb) {
        const long long first = (long long)(blockIdx.x - p.nxb) * blockDim.x + threadIdx.x, stride = (long long)(gridDim.x - p.nxb) * blockDim.x;
        if constexpr (PLANES) {
            if (p.w) wino4_filter_planes(p, first, stride);
            else wino4_touch_planes(p, first, stride);                // (the planes were made once: p.U)
        } else wino4_filter_elems(p, first, stride);
        return;
    }
    // 8 lanes = the 8 channel quads of one pixel's 128-byte line, 8 tiles per wave (the access pattern of wino_xform_f32)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cg = blockIdx.x % p.ncg, tb = blockIdx.x / p.ncg;
    const int c4 = cg * 8 + (lane & 7);
    const int t = tb * 32 + wave * 8 + (lane >> 3);
    if (c4 >= p.C4p) return;
    const bool tv = t < p.T && c4 < p.C4;                // the padding plane c4 = C4 (odd C4) and the padding tiles are zero
    const int tt = t < p.T ? t : 0;
    const int per = p.th * p.tw;
    const int n = tt / per, rem = tt - n * per;
    const int ty = rem / p.tw, tx = rem - ty * p.tw;
    const int r0 = 4 * ty - 1, c0 = 4 * tx - 1;
    const float* base = p.x + p.x_off + 4 * (c4 < p.C4 ? c4 : 0);
    // v = B^T d B, row by row of d: e = d[k][.] B (6 -> 6), v[i][.] += B^T[i][k] e
    f32x4 v[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int l = 0; l < 6; ++l) v[i][l] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int r = r0 + k;
        const bool rv = tv && r >= 0 && r < p.H;
        f32x4 d[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int c = c0 + j;
            const bool ok = rv && c >= 0 && c < p.W;
            const size_t pix = ok ? ((size_t)n * p.H + r) * p.W + c : 0;
            const f32x4 ld = *reinterpret_cast<const f32x4*>(base + pix * p.x_ld);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            d[j] = ok ? ld : z;
        }
        f32x4 e[6];
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            e[l] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (W4_BT[l][j] != 0.f) e[l] += W4_BT[l][j] * d[j];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (W4_BT[i][k] != 0.f)
#pragma unroll
                for (int l = 0; l < 6; ++l) v[i][l] += W4_BT[i][k] * e[l];
    }
    if constexpr (PLANES) {                              // the eight lanes of a tile write one 64-byte row of each plane
        const int nkc = p.C4p / 8, n_mt = p.Tpad / 64;
        char* dst = reinterpret_cast<char*>(p.V) + w4s_offset(0, 4 * c4, t, 0, nkc, n_mt);
        const size_t xs = (size_t)nkc * n_mt * W4S_PIECE;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int l = 0; l < 6; ++l) {
                u32x2 h, m, lo;
                f32x4 chk = {0.f, 0.f, 0.f, 0.f};
                s3_split(v[i][l], h, m, lo, chk);
                char* d = dst + (6 * i + l) * xs;
                *reinterpret_cast<u32x2*>(d) = h;
                *reinterpret_cast<u32x2*>(d + W4S_PLANE) = m;
                *reinterpret_cast<u32x2*>(d + 2 * W4S_PLANE) = lo;
            }
        return;
    }
    float* dst = p.V + ((size_t)c4 * p.Tpad + t) * 4;
    const size_t xs = (size_t)p.C4p * p.Tpad * 4;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int l = 0; l < 6; ++l) *reinterpret_cast<f32x4*>(dst + (6 * i + l) * xs) = v[i][l];
}

// ------------------------------------------------------------------------------ 36 GEMMs in six passes + output transform + epilogue
// (Wino4Args, the tile table, the fold of a row and the epilogue: wino4_epilogue.h)
constexpr int W4_STAGE = 24576;          // bytes per ring stage: V [2 planes][6 xi][64][4] floats, then U the same
constexpr int W4_SLOTS = 4;              // (a power of two: slot arithmetic by mask)
constexpr int W4_DMA = 3;                // DMA wave-instructions per wave and stage

// fragments of one sub-step: the U row (A operand) and the V rows of the wave's two tile blocks (B operands)
template <int OFF>
__device__ __forceinline__ void w4_read3(float& a, float& b0, float& b1, unsigned ua, unsigned va) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(a) : "v"(ua), "n"(OFF));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(b0) : "v"(va), "n"(OFF));
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(b1) : "v"(va), "n"(OFF + 256));
}

// 512 threads = 8 waves, two per SIMD: wave (wm, wn) owns tiles 32 wm .. + 31 and channels 16 wn .. + 15 of the 64 x 64 block, as
// two 16 x 16 blocks of v_mfma_f32_16x16x4_f32 per xi (D[channel][tile]: a lane holds one tile and 4 consecutive channels)
template <int ACT, bool RES>
__global__ __launch_bounds__(512, 1) void conv_wino4_f32(const Wino4Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    // block map: 8 tile blocks (one per XCD) x all channel blocks per row, so the channel blocks of a tile block share an L2. The
    // rows of the whole tile blocks come first; each row of 8 tail blocks then comes twice, once per half.
    // (Measured at 13 x 13, 512 -> 1024, batch 32, where all 256 workgroups are halves and U4 is the larger operand: a map that gives
    // an XCD 4 tile blocks x 4 channel blocks x both halves halves the launch's FETCH_SIZE and changes its time by less than the
    // spread of the rounds, profiles/r08: not kept)
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int nt = q % p.n_nt, row = q / p.n_nt;
    const int wrows = (p.n_whole + 7) >> 3;
    const bool cut = row >= wrows;
    const int half = (row - wrows) & 1;
    const int mt = cut ? p.n_whole + ((row - wrows) >> 1) * 8 + xcd : row * 8 + xcd;
    if (mt >= (cut ? p.n_mt : p.n_whole)) return;
    // a half workgroup covers tiles 32 half .. + 31 of its block: waves 0 .. 3 (one per SIMD) take the 16 channels each of that
    // half, the same 16 x 16 blocks in the same order as in a whole workgroup; waves 4 .. 7 only move their DMA pieces
    const int wm = cut ? half : wave & 1, wn = cut ? wave & 3 : wave >> 1;
    const bool busy = !cut || wave < 4;

    int* tab = reinterpret_cast<int*>(smem + W4_SLOTS * W4_STAGE);
    wino4_tile_table(p, tab, tid, mt, cut, half);

    // ---- DMA roles: waves 2 grp, 2 grp + 1 move part grp of a stage (0 / 1: plane 0 / 1 of V, 2 / 3: the same planes of U),
    // three xi each; lane = row
    const size_t v_xi = (size_t)p.C4p * p.Tpad * 4, v_c4 = (size_t)p.Tpad * 4;
    const size_t u_xi = (size_t)p.C4p * p.CoutPad * 4, u_c4 = (size_t)p.CoutPad * 4;
    const int grp = wave >> 1, x0 = 3 * (wave & 1);
    const int plane = grp & 1;
    const char* src = grp < 2 ? reinterpret_cast<const char*>(p.V + plane * v_c4 + (size_t)mt * 256)
                              : reinterpret_cast<const char*>(p.U + plane * u_c4 + (size_t)nt * 256);
    const size_t s_xi = (grp < 2 ? v_xi : u_xi) * 4, s_c4 = (grp < 2 ? v_c4 : u_c4) * 4;       // bytes
    const unsigned lane16 = lane * 16;
    const unsigned lds0 = (unsigned)(size_t)(wn_lptr)smem;
    auto issue_piece = [&](int k, int pass, int st, int slot) {
        const int x = x0 + k;
        wn_glds16_s(src + (size_t)(6 * pass + x) * s_xi + (size_t)(2 * st) * s_c4, lane16, lds0 + slot * W4_STAGE + (6 * grp + x) * 1024);
    };
    auto issue = [&](int pass, int st, int slot) { wn_for<0, W4_DMA>([&](auto K) { issue_piece(decltype(K)::value, pass, st, slot); }); };

    // ---- fragment addresses: sub-step s = 6 plane + x of a stage sits at s KiB in both halves; channel kq of the plane,
    // rows 32 wm + l16 (+ 16) of V, row 16 wn + l16 of U
    const unsigned vb = lds0 + (32 * wm + l16) * 16 + kq * 4;
    const unsigned ub = lds0 + 12288 + (16 * wn + l16) * 16 + kq * 4;

    const int nst = p.C4p / 2;
    // the partial output tiles: [tile block bb][output row i][output column j] of this lane's tile 32 wm + 16 bb + l16, its
    // channels 16 wn + 4 kq .. + 3
    f32x4 py[2][4][4];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) py[bb][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto run_pass = [&](auto PASS) {
        constexpr int a = decltype(PASS)::value;
        float fa[12], fb0[12], fb1[12];
        if constexpr (a == 0) {              // (the first stages of passes 1 .. 5 are requested before the previous pass's transform)
            issue(0, 0, 0);
            if (nst > 1) issue(0, 1, 1);
            if (nst > 2) issue(0, 2, 2);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[6][2];
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) acc[x][bb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int x = 0; x < 6; ++x) asm volatile("" : "+v"(acc[x][0]), "+v"(acc[x][1]));
        __builtin_amdgcn_sched_barrier(0);
        if (nst > 2) wn_wait_vmcnt<2 * W4_DMA>();
        else if (nst > 1) wn_wait_vmcnt<W4_DMA>();
        else wn_wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        w4_read3<0>(fa[0], fb0[0], fb1[0], ub, vb);
        w4_read3<1024>(fa[1], fb0[1], fb1[1], ub, vb);

        int slot = 0;
        for (int st = 0; st < nst; ++st) {
            const unsigned sb = (unsigned)slot * W4_STAGE;
            const int ns = (slot + 1) & (W4_SLOTS - 1);
            const unsigned nb = (unsigned)ns * W4_STAGE;
            wn_for<0, 12>([&](auto S) {
                constexpr int s = decltype(S)::value, x = s % 6;
                if constexpr (s == 10) {
                    // stage st + 1 has to be in LDS for everybody before its first fragments are read (the only requests younger
                    // than its pieces are those of stage st + 2); the slot of stage st - 1 is free once everybody is here
                    __builtin_amdgcn_sched_barrier(0);
                    if (st + 2 < nst) wn_wait_vmcnt<W4_DMA>();
                    else wn_wait_vmcnt<0>();
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (s + 2 < 12) w4_read3<(s + 2) * 1024>(fa[s + 2], fb0[s + 2], fb1[s + 2], ub + sb, vb + sb);
                // reads issued after those of sub-step s and still in flight: s < 10 -> s + 1, s + 2; 10 -> 11; 11 -> the next stage's 0
                constexpr int after = s < 10 ? 6 : 3;
                asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(fa[s]), "+v"(fb0[s]), "+v"(fb1[s]) : "n"(after));
                acc[x][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[s], fb0[s], acc[x][0], 0, 0, 0);
                acc[x][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[s], fb1[s], acc[x][1], 0, 0, 0);
                if constexpr (s < W4_DMA) {
                    // one piece of stage st + 2 behind each of the first sub-steps: its slot (= stage st - 2's) is free since the
                    // barrier of stage st - 1; stages 0 .. 2 come from the prologue
                    __builtin_amdgcn_sched_barrier(0);
                    if (st >= 1 && st + 2 < nst) issue_piece(s, a, st + 2, (slot + 2) & (W4_SLOTS - 1));
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (s >= 10) {
                    __builtin_amdgcn_sched_barrier(0);
                    w4_read3<(s - 10) * 1024>(fa[s - 10], fb0[s - 10], fb1[s - 10], ub + nb, vb + nb);
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            slot = ns;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the look-ahead reads of the stage after the last
        __syncthreads();                                     // everybody is done with the ring: the next pass's first stages / the staging may overwrite it
        if constexpr (a < 5) {                               // ... and they are requested now: in flight during the transform below
            issue(a + 1, 0, 0);
            if (nst > 1) issue(a + 1, 1, 1);
            if (nst > 2) issue(a + 1, 2, 2);
            __builtin_amdgcn_sched_barrier(0);
        }
        wino4_fold_row<a>(acc, py);
    };
    if (busy) {
        run_pass(std::integral_constant<int, 0>{});
        run_pass(std::integral_constant<int, 1>{});
        run_pass(std::integral_constant<int, 2>{});
        run_pass(std::integral_constant<int, 3>{});
        run_pass(std::integral_constant<int, 4>{});
        run_pass(std::integral_constant<int, 5>{});
    } else {
        // the idle waves of a half workgroup: the DMA pieces, the waits and the barriers of run_pass, in the same places
        for (int a = 0; a < 6; ++a) {
            if (a == 0) {
                issue(0, 0, 0);
                if (nst > 1) issue(0, 1, 1);
                if (nst > 2) issue(0, 2, 2);
            }
            if (nst > 2) wn_wait_vmcnt<2 * W4_DMA>();
            else if (nst > 1) wn_wait_vmcnt<W4_DMA>();
            else wn_wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            int slot = 0;
            for (int st = 0; st < nst; ++st) {
                if (st >= 1 && st + 2 < nst) issue(a, st + 2, (slot + 2) & (W4_SLOTS - 1));
                if (st + 2 < nst) wn_wait_vmcnt<W4_DMA>();
                else wn_wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                slot = (slot + 1) & (W4_SLOTS - 1);
            }
            __syncthreads();
            if (a < 5) {
                issue(a + 1, 0, 0);
                if (nst > 1) issue(a + 1, 1, 1);
                if (nst > 2) issue(a + 1, 2, 2);
            }
        }
    }

    wino4_epilogue<ACT, RES>(p, smem, tab, py, tid, nt, wm, wn, l16, kq, busy);
}

// ------------------------------------------------------------------------------ host side
Wino4Geom wino4_geom(const yolo_conv_desc* d) {
    Wino4Geom g{};
    if (!wino_supported(d)) return g;
    g.th = (d->h + 3) / 4; g.tw = (d->w + 3) / 4; g.T = (long long)d->n * g.th * g.tw;
    g.C4 = d->cin / 4; g.C4p = round_up(g.C4, 2); g.CoutPad = round_up(d->cout, 64);
    // four times the padded tiles as an int, and the transform pass's one-dimensional grid
    g.ok = g.T + 64 <= 0x7fffffffLL / 4 && (g.T + 63) / 32 * ((g.C4p + 7) / 8) + 1024 <= 0x7fffffffLL;
    if (!g.ok) return g;
    g.Tpad = round_up((int)g.T, 64); g.n_mt = g.Tpad / 64; g.n_nt = g.CoutPad / 64;
    g.v4_bytes = (size_t)36 * g.C4p * g.Tpad * 4 * sizeof(float);
    g.u4_bytes = (size_t)36 * g.C4p * g.CoutPad * 4 * sizeof(float);
    g.planes = d->cin % 32 == 0; g.nkc = d->cin / 32;
    if (!g.planes) return g;
    g.v_plane_bytes = (size_t)36 * g.nkc * g.n_mt * W4S_PIECE;
    g.u_plane_bytes = (size_t)36 * g.nkc * g.n_nt * W4S_PIECE;
    return g;
}

bool wino4_supported(const yolo_conv_desc* d) { return wino4_geom(d).ok; }

// Looks at the layer's shape only, never at the batch size. Measured at batch 32 (tools/conv_bench.py --tile 13,14,15):
// F(4x4) 252 / 222 / 196 us against F(2x2)'s best 415 / 330 / 270 at 104 x 104, 52 x 52, 26 x 26 (which pads to 28 x 28: 16 % of
// the tiles' pixels wasted), 351 against 297 at 13 x 13 (padded to 16 x 16: 51 % wasted). So: maps of at least 26 x 26 pixels whose
// padding to whole 4 x 4 tiles adds at most a fifth.
// That 13 x 13 figure was 128 whole workgroups on 256 CUs, each launch transforming its filters. A caller that brings the filters
// finished (YOLO_FLAG_FILTERS_APPENDED) gets a launch without filter blocks, and wino4_whole_blocks cuts it into one round of half
// workgroups: 512 -> 1024 at batch 32 (profiles/r08/conv_bench_c13.txt, medians of 7 rounds of 20) 219 / 223 us (with residual)
// against F(2x2)'s best 277 / 290 at 13 x 13, 339 / 349 against 555 / 580 at 19 x 19 (13 whole tile blocks: 208 workgroups). With
// the flag the rule admits those two shapes too, each on its own measurement; every other small map stays on F(2x2).
bool wino4_small_channels(const yolo_conv_desc* d) { return d->cin == 512 && d->cout == 1024; }

bool wino4_eligible(const yolo_conv_desc* d) {
    if (switches().no_winograd || !wino_eligible(d) || !wino4_supported(d)) return false;
    const long long area = (long long)d->h * d->w, padded = 16LL * ((d->h + 3) / 4) * ((d->w + 3) / 4);
    if (area >= 26 * 26 && 5 * padded <= 6 * area) return true;
    return (d->flags & YOLO_FLAG_FILTERS_APPENDED) && wino4_small_channels(d) && d->h == d->w && (d->h == 13 || d->h == 19);
}

// (the byte sizes of a geometry that is not ok are 0)
size_t wino4_workspace_bytes(const yolo_conv_desc* d) { const Wino4Geom g = wino4_geom(d); return g.v4_bytes + g.u4_bytes; }
size_t wino4_filter_bytes(const yolo_conv_desc* d) { return wino4_geom(d).u4_bytes; }

// compute units of the current device, asked once per device (0: no device)
int wino4_num_cus() {
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int n = cus[dev & 63].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); return 0; }
    cus[dev & 63].store(n, std::memory_order_relaxed);
    return n;
}

// How a launch of n_mt tile blocks x n_nt channel blocks is cut, one workgroup per CU and round: the tile blocks of the full rounds
// stay whole (all channel blocks of a tile block together). If the rest is at most half a round of workgroups, each of its tile
// blocks runs as two workgroups of 32 tiles, so the short last round uses twice the CUs for half the multiply work each.
// Looks at (n_mt, n_nt, CUs) only; the arithmetic of a tile does not depend on the cut.
int wino4_whole_blocks(int n_mt, int n_nt, int cus) {
    if (cus <= 0) return n_mt;
    const long long wgs = (long long)n_mt * n_nt;
    const int whole = (int)(wgs / cus * cus / n_nt);
    const long long tail = (long long)(n_mt - whole) * n_nt;
    return tail == 0 || 2 * tail > cus ? n_mt : whole;
}

Wino4Args wino4_gemm_args(const Wino4Geom& g, const yolo_conv_desc* d, const float* scale, const float* shift, const void* residual, void* y,
                          int32_t* nan_flag) {
    Wino4Args a;
    a.V = a.U = nullptr;
    a.scale = scale; a.shift = shift; a.res = (const float*)residual; a.y = (float*)y; a.nan_flag = nan_flag;
    a.T = (int)g.T; a.Tpad = g.Tpad; a.C4p = g.C4p; a.Cout = d->cout; a.CoutPad = g.CoutPad;
    a.th = g.th; a.tw = g.tw; a.H = d->h; a.W = d->w;
    a.y_ld = d->y_ld; a.y_off = d->y_off; a.r_ld = d->r_ld; a.r_off = d->r_off; a.flags = d->flags;
    a.n_mt = g.n_mt; a.n_nt = g.n_nt;
    a.n_whole = wino4_whole_blocks(a.n_mt, a.n_nt, wino4_num_cus());
    return a;
}

int wino4_grid(const Wino4Args& a) { return 8 * a.n_nt * (ceil_div(a.n_whole, 8) + 2 * ceil_div(a.n_mt - a.n_whole, 8)); }

// the arguments of the transform pass and of the filter kernels (which read the filter side only), all but the four pointers
static Wino4XArgs wino4_xform_args(const Wino4Geom& g, const yolo_conv_desc* d) {
    Wino4XArgs xa{};
    xa.H = d->h; xa.W = d->w; xa.C4 = g.C4; xa.C4p = g.C4p; xa.x_ld = d->x_ld; xa.x_off = d->x_off;
    xa.th = g.th; xa.tw = g.tw; xa.T = (int)g.T; xa.Tpad = g.Tpad; xa.ncg = ceil_div(g.C4p, 8);
    xa.nxb = (g.Tpad / 32) * xa.ncg;
    xa.cout = d->cout; xa.cin = d->cin; xa.coutp = g.CoutPad; xa.cinp = cin_pad_of(d->cin); xa.kpad = kpad_of(d->cin, 3);
    xa.utotal = (long long)g.C4p * g.CoutPad * 4;
    return xa;
}
// blocks of 256 threads that stride over n elements: at most 1,024 (the grid bound that wino4_geom checked)
static int wino4_elem_blocks(long long n) { return (int)std::min<long long>((n + 255) / 256, 1024); }

// ---- YOLO_FLAG_WINO_SPLIT_BF16: the transform pass writes bf16 planes (wino4_planes.h) for conv_wino4s_f32.hip
bool wino4_split_supported(const yolo_conv_desc* d) { return wino4_geom(d).planes; }
size_t wino4_split_workspace_bytes(const yolo_conv_desc* d) { const Wino4Geom g = wino4_geom(d); return g.v_plane_bytes + g.u_plane_bytes; }
size_t wino4_filter_plane_bytes(const yolo_conv_desc* d) { return wino4_geom(d).u_plane_bytes; }

// V planes at the start of the workspace, the planes of the caller's finished U4 behind them (made again by this launch), unless the
// caller keeps them (U_planes: nothing behind the V planes is written; the trailing blocks only read U_planes, wino4_touch_planes)
int wino4_planes_launch(const Wino4Geom& g, const yolo_conv_desc* d, const void* x, const float* U4, const void* U_planes, void* workspace,
                        hipStream_t s) {
    Wino4XArgs xa = wino4_xform_args(g, d);
    xa.x = (const float*)x; xa.V = (float*)workspace; xa.w = U_planes ? nullptr : U4;
    xa.U = static_cast<float*>(const_cast<void*>(wino4_u_planes(g, U_planes, workspace)));
    // trailing blocks: a thread per 64 bytes of the caller's planes to touch, or per quad of the planes to write (36 xi x C4p x coutp)
    const int nub = wino4_elem_blocks(U_planes ? xa.utotal * 27 / 8 : 9 * xa.utotal);
    hipLaunchKernelGGL(wino4_xform_f32<true>, dim3((unsigned)(xa.nxb + nub)), dim3(256), 0, s, xa);
    return check_launch("wino4_xform_f32 (planes)");
}

// w_rm: the row-major section at the start of the packed weights (yolo_pack_weights / yolo_pack_weights_dgrad); U4_ready: the
// filters transformed before (yolo_wino4_filters), or NULL: this launch transforms them into the workspace behind V4
int conv_wino4_launch(const yolo_conv_desc* d, const void* x, const float* w_rm, const float* U4_ready, const float* scale, const float* shift,
                      const void* residual, void* y, void* workspace, size_t workspace_bytes, int32_t* nan_flag, hipStream_t s) {
    const Wino4Geom g = wino4_geom(d);
    if (!g.ok) return fail(YOLO_ERR_UNSUPPORTED, "conv winograd F(4x4): needs fp32 3x3 stride 1, NHWC output, channels %% 4 == 0");
    const size_t need = g.v4_bytes + g.u4_bytes;
    if (!workspace || workspace_bytes < need) return fail(YOLO_ERR_WORKSPACE, "conv winograd F(4x4): workspace %zu < %zu bytes", workspace_bytes, need);
    if ((size_t)workspace & 15) return fail(YOLO_ERR_ARG, "conv winograd F(4x4): workspace must be 16-byte aligned");
    if ((size_t)U4_ready & 15) return fail(YOLO_ERR_ARG, "conv winograd F(4x4): transformed filters must be 16-byte aligned");
    float* V = (float*)workspace;
    float* U = reinterpret_cast<float*>(static_cast<char*>(workspace) + g.v4_bytes);
    Wino4XArgs xa = wino4_xform_args(g, d);
    xa.x = (const float*)x; xa.V = V; xa.w = w_rm; xa.U = U;
    const int nub = U4_ready ? 0 : wino4_elem_blocks(xa.utotal);
    hipLaunchKernelGGL(wino4_xform_f32<false>, dim3((unsigned)(xa.nxb + nub)), dim3(256), 0, s, xa);
    if (int rc = check_launch("wino4_xform_f32")) return rc;

    Wino4Args a = wino4_gemm_args(g, d, scale, shift, residual, y, nan_flag);
    a.V = V; a.U = U4_ready ? U4_ready : U;
    const int grid = wino4_grid(a);
    const bool res = d->flags & YOLO_FLAG_RESIDUAL;
    const size_t lds = (size_t)W4_SLOTS * W4_STAGE + W4_TAB;         // (the epilogue's staging, 256 x 68 x 4, lies over the idle ring)
    auto go = [&](auto kern) -> int {
        static LdsOnce once;
        if (int rc = reserve_lds(once, reinterpret_cast<const void*>(kern), lds, "conv_wino4_f32")) return rc;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, a);
        return check_launch("conv_wino4_f32");
    };
    YOLO_SWITCH_ACT(d->act, return res ? go(&conv_wino4_f32<ACT, true>) : go(&conv_wino4_f32<ACT, false>));
    return fail(YOLO_ERR_ARG, "conv winograd F(4x4): activation");
}

}  // namespace yolo

extern "C" {

size_t yolo_wino4_filter_bytes(const yolo_conv_desc* d) { return d ? yolo::wino4_filter_bytes(d) : 0; }

size_t yolo_wino4_appended_bytes(const yolo_conv_desc* d) {
    return d && yolo::wino4_supported(d) ? yolo::packed_f32(d->cout, d->cin, d->ksize).tail_bytes + yolo::wino4_filter_bytes(d) : 0;
}

int yolo_wino4_appended_wanted(const yolo_conv_desc* d) {
    return d && !yolo::switches().no_winograd && yolo::wino4_supported(d) && yolo::wino4_small_channels(d);
}

int yolo_wino4_filters(const yolo_conv_desc* d, const void* w_packed, void* U4, void* stream) {
    using namespace yolo;
    if (!d || !w_packed || !U4) return fail(YOLO_ERR_ARG, "wino4 filters: null pointer");
    const Wino4Geom g = wino4_geom(d);
    if (!g.ok) return fail(YOLO_ERR_UNSUPPORTED, "wino4 filters: needs fp32 3x3 stride 1, NHWC output, channels %% 4 == 0");
    if ((size_t)U4 & 15) return fail(YOLO_ERR_ARG, "wino4 filters: U4 must be 16-byte aligned");
    // in place (U4 behind the packed weights of the same buffer, YOLO_FLAG_FILTERS_APPENDED) is fine: only the row-major section at
    // the start of w_packed is read. U4 may not begin inside that section
    const char *rm = (const char*)w_packed, *u = (const char*)U4;
    const size_t rm_bytes = (size_t)d->cout * kpad_of(d->cin, 3) * sizeof(float);
    if (u < rm + rm_bytes && rm < u + g.u4_bytes) return fail(YOLO_ERR_ARG, "wino4 filters: U4 overlaps the weights it is made from");
    Wino4XArgs xa = wino4_xform_args(g, d);
    xa.w = (const float*)w_packed; xa.U = (float*)U4;
    hipLaunchKernelGGL(wino4_filters_f32, dim3((unsigned)wino4_elem_blocks(xa.utotal)), dim3(256), 0, (hipStream_t)stream, xa);
    return check_launch("wino4_filters_f32");
}

size_t yolo_wino4_filter_plane_bytes(const yolo_conv_desc* d) { return d ? yolo::wino4_filter_plane_bytes(d) : 0; }

int yolo_wino4_filter_planes(const yolo_conv_desc* d, const void* U4, void* planes, void* stream) {
    using namespace yolo;
    if (!d || !U4 || !planes) return fail(YOLO_ERR_ARG, "wino4 filter planes: null pointer");
    const Wino4Geom g = wino4_geom(d);
    if (!g.planes) return fail(YOLO_ERR_UNSUPPORTED, "wino4 filter planes: needs fp32 3x3 stride 1, NHWC output, cin %% 32 == 0");
    if (((size_t)U4 | (size_t)planes) & 15) return fail(YOLO_ERR_ARG, "wino4 filter planes: U4 and planes must be 16-byte aligned");
    const char *u = (const char*)U4, *pl = (const char*)planes;
    if (pl < u + g.u4_bytes && u < pl + g.u_plane_bytes) return fail(YOLO_ERR_ARG, "wino4 filter planes: planes overlap the U4 they are made from");
    Wino4XArgs xa = wino4_xform_args(g, d);
    xa.w = (const float*)U4; xa.U = (float*)planes;
    hipLaunchKernelGGL(wino4_filter_planes_f32, dim3((unsigned)wino4_elem_blocks(9 * xa.utotal)), dim3(256), 0, (hipStream_t)stream, xa);
    return check_launch("wino4_filter_planes_f32");
}

int yolo_conv_wino4_blocks(const yolo_conv_desc* d, int* whole, int* half) {
    using namespace yolo;
    if (!d || !whole || !half) return fail(YOLO_ERR_ARG, "wino4 blocks: null pointer");
    const Wino4Geom g = wino4_geom(d);
    if (!g.ok) return fail(YOLO_ERR_UNSUPPORTED, "wino4 blocks: needs fp32 3x3 stride 1, NHWC output, channels %% 4 == 0");
    const int cus = wino4_num_cus();
    if (cus <= 0) return fail(YOLO_ERR_LAUNCH, "wino4 blocks: no current device");
    *whole = wino4_whole_blocks(g.n_mt, g.n_nt, cus);
    *half = g.n_mt - *whole;
    return YOLO_OK;
}

}  // extern "C"
