// conv_wino4s_f32.hip — the 36 GEMMs of Winograd F(4x4, 3x3) on the bf16 matrix cores (YOLO_FLAG_WINO_SPLIT_BF16).
//
// conv_wino4_f32.hip multiplies on v_mfma_f32_16x16x4_f32, whose rate is the vector FMA rate. Here every fp32 value of V4 and U4
// is the exact sum of three bf16 values (split3.h), split once where it is produced: the transform pass (wino4_xform_f32<true>)
// writes the planes of wino4_planes.h. Six of the nine partial products in the fixed order of conv_split3_f32, smallest first,
// (hi, lo) (lo, hi) (mid, mid) (hi, mid) (mid, hi) (hi, hi) with the U part named first, go into one fp32 accumulator by
// v_mfma_f32_16x16x32_bf16: per 32 input channels, xi and 16 x 16 block six MFMAs of ~16 cycles instead of eight of 32. The kernel
// has no split arithmetic and no finiteness vote: an Inf or a NaN of x becomes a NaN in the planes (Inf - Inf) and in every
// output it reaches, which the epilogue's NaN flag reports.
//
// The skeleton is conv_wino4_f32's: 64 tiles x 64 output channels per workgroup, 8 waves, wave (wm, wn) owns tiles 32 wm .. + 31 and
// channels 16 wn .. + 15 as two 16 x 16 blocks (the C/D layout of the two MFMAs is the same), six passes over K, one row of M each,
// 48 accumulators per pass, the fold into 128 partial-tile registers parked in AGPRs, the tile table and the epilogue
// (wino4_epilogue.h). Only the K loop and the ring differ:
//   stage    one xi x 32 input channels: the 12 KiB piece of V (3 planes x 64 tiles x 64 bytes), then the 12 KiB piece of U. Both are
//            contiguous in global memory and byte for byte the LDS image: 24 LDS-DMA wave-instructions of 1 KiB, three per wave
//            (waves 0 - 3 move V, 4 - 7 move U). Stages run xi-fastest inside a pass: g = 6 chunk + x.
//   ring     six slots of 24 KiB, one ring for the whole kernel: the stages are numbered through the six passes (a pass is a whole
//            number of laps, so the slot of a stage is its xi mod 6, a compile-time constant of the unrolled loop). Stage g + 5 is
//            requested during stage g into the slot of stage g - 1, across the pass boundaries too: the ring drains once, in the
//            last lap of pass 5, and up to 120 KiB per CU are in flight.
//   step g   wait for the own pieces of stage g + 1 (vmcnt: the pieces of stages g + 2 .. g + 4 are younger), barrier: stage g + 1 is
//            in LDS for everybody, and everybody has read stage g - 1 out of its slot. Then: request one piece of stage g + 5 behind
//            each of the first MFMA pairs, read the nine fragments of stage g + 1 (3 U + 2 x 3 V, ds_read_b128, into the other
//            fragment set), wait for those of stage g (lgkmcnt(9)), twelve MFMAs.
//   pass end the fold (wino4_fold_row) runs with five stages in flight. The fragments of the next pass's stage 0, which the last
//            step has read, are dropped and read again behind the fold: no barrier is needed for that (stage 0 landed behind the
//            last step's barrier), and the fold keeps its registers.
// One workgroup per CU and round; the tile blocks of a short last round run as two workgroups of 32 tiles each (wino4_whole_blocks, the
// cut of conv_wino4_f32), and such a half workgroup requests only its own 32 rows of the V piece: 18 KiB per stage instead of 24.
#include "split3.h"
#include "wino4_planes.h"
#include "wino4_epilogue.h"

namespace yolo {

struct Wino4SArgs {
    Wino4Args e;             // V / U: the plane buffers; C4p is unused
    int nkc;                 // chunks of 32 input channels
    int xmap;                // all tile blocks in halves, n_mt and n_nt multiples of 4: an XCD gets 4 tile blocks x 4 channel blocks x both halves
};

constexpr int W4S_STAGE = 2 * W4S_PIECE; // bytes per ring stage: the V piece, then the U piece
constexpr int W4S_SLOTS = 6;             // one lap of the ring is the six xi of a chunk: stage g sits in slot g % 6 = its xi
constexpr int W4S_AHEAD = W4S_SLOTS - 1; // stage g + 5 is requested during stage g
constexpr int W4S_DMA = 3;               // DMA wave-instructions per wave and stage
static_assert(W4S_SLOTS == 6 && W4S_AHEAD == 5, "the slot of a stage is its xi, and the counted waits of the last lap are written out for five stages ahead");

template <int OFF>
__device__ __forceinline__ void w4s_read_at(s3_u32x4& f, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(f) : "v"(addr), "n"(OFF));
}

template <int ACT, bool RES>
__global__ __launch_bounds__(512, 1) void conv_wino4s_f32(const Wino4SArgs q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Wino4Args& p = q.e;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    // block map of conv_wino4_f32: 8 tile blocks (one per XCD) x all channel blocks per row. The rows of the whole tile blocks come
    // first; each row of 8 tail blocks then comes twice, once per half.
    const int xcd = blockIdx.x & 7, bq = blockIdx.x >> 3;
    const int row = bq / p.n_nt, wrows = (p.n_whole + 7) >> 3;
    int nt = bq % p.n_nt;
    bool cut = row >= wrows;
    int half = (row - wrows) & 1;
    int mt = cut ? p.n_whole + ((row - wrows) >> 1) * 8 + xcd : row * 8 + xcd;
    if (q.xmap) {
        // a launch that is all halves: the 32 workgroups of an XCD share 4 tile blocks and 4 channel blocks instead of one tile block
        // and all channel blocks, so an XCD's L2 streams a quarter of the U planes and half of the V planes (same bits: index
        // arithmetic only)
        const int sb = xcd + 8 * (bq >> 5), l = bq & 31, ntg = p.n_mt >> 2;
        cut = true;
        half = l & 1;
        nt = 4 * (sb / ntg) + ((l >> 1) & 3);
        mt = 4 * (sb % ntg) + (l >> 3);
    }
    if (mt >= (cut ? p.n_mt : p.n_whole)) return;
    // a half workgroup covers tiles 32 half .. + 31 of its block: waves 0 .. 3 (one per SIMD) take the 16 channels each of that
    // half, the same two 16 x 16 blocks per xi with the same six products in the same order as wave (half, wn) of a whole
    // workgroup; waves 4 .. 7 only move DMA pieces and meet the barriers
    const int wm = cut ? half : wave & 1, wn = cut ? wave & 3 : wave >> 1;
    const bool busy = !cut || wave < 4;

    int* tab = reinterpret_cast<int*>(smem + W4S_SLOTS * W4S_STAGE);
    wino4_tile_table(p, tab, tid, mt, cut, half);

    // ---- DMA roles (lane = 16 bytes). Whole workgroup: wave w moves KiB 3 w .. 3 w + 2 of a stage, waves 0 - 3 the V piece, 4 - 7 the U
    // piece. Half workgroup: 18 KiB per stage instead of 24. The computing waves 0 - 3 move the U piece, three KiB each as waves 4 - 7
    // of a whole workgroup do (so their counted waits stay); of the V piece only rows 32 half .. + 31 are requested, 2 KiB per plane,
    // contiguous in global memory and in LDS, where they go to their usual addresses: waves 4 - 6 move one plane's each, wave 7 nothing.
    const bool dv = cut ? wave >= 4 : wave < 4;
    const int dw = cut ? (wave + 4) & 7 : wave;                               // the wave of a whole workgroup whose KiB start this wave's
    const unsigned own = cut && dv ? (wave - 4) * W4S_PLANE + half * (W4S_PLANE / 2) : 3072 * dw;     // ... or the plane's half: bytes into the stage
    const char* src = (dv ? reinterpret_cast<const char*>(p.V) + (size_t)mt * W4S_PIECE : reinterpret_cast<const char*>(p.U) + (size_t)nt * W4S_PIECE)
                      + (own - (dv ? 0 : W4S_PIECE));
    const size_t s_st = (size_t)(dv ? p.n_mt : p.n_nt) * W4S_PIECE;          // bytes from one (xi, chunk) to the next
    const unsigned lane16 = lane * 16;
    const unsigned lds0 = (unsigned)(size_t)(wn_lptr)smem;
    const unsigned ldsw = lds0 + own;
    const int nkc = q.nkc;
    // piece k of stage (pass, chunk kc, xi x) into slot x; kc == nkc names chunk 0 of the next pass (the ring runs on across passes)
    auto issue_piece = [&](int k, int pass, int kc, int x) {
        const int xi = kc < nkc ? 6 * pass + x : 6 * pass + 6 + x, c = kc < nkc ? kc : 0;
        wn_glds16_s(src + ((size_t)xi * nkc + c) * s_st + k * 1024, lane16, ldsw + x * W4S_STAGE + k * 1024);
    };

    // ---- fragment addresses in slot 0: rows 32 wm + l16 (+ 16) of the V planes, row 16 wn + l16 of the U planes, channels 8 kq ..
    const unsigned sw = w4s_slot(l16, kq) * 16;          // (blocks start at multiples of 16 rows: the row quad is l16's)
    const unsigned vb = lds0 + (32 * wm + l16) * 64 + sw;
    const unsigned ub = lds0 + W4S_PIECE + (16 * wn + l16) * 64 + sw;

    f32x4 py[2][4][4];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) py[bb][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto run_pass = [&](auto PASS) {
        constexpr int a = decltype(PASS)::value;
        // Fragments of a stage: the U row and the V rows of the two tile blocks, per part. 48 accumulators leave the VGPR half no room
        // for two whole sets (2 x 36), so only the hi parts, which the first and the last product of a stage read, have two (by
        // stage parity); mid and lo are read again, for the next stage, as soon as their last product has been issued.
        s3_u32x4 uh[2], vh[2][2], um, ul, vm[2], vl[2];
        auto rd_hi = [&](auto SET, unsigned sb) {        // R1
            constexpr int S = decltype(SET)::value;
            w4s_read_at<0>(uh[S], ub + sb);
            w4s_read_at<0>(vh[S][0], vb + sb);
            w4s_read_at<1024>(vh[S][1], vb + sb);
        };
        auto rd_vlo = [&](unsigned sb) {                 // R2
            w4s_read_at<2 * W4S_PLANE>(vl[0], vb + sb);
            w4s_read_at<2 * W4S_PLANE + 1024>(vl[1], vb + sb);
        };
        auto rd_ulo = [&](unsigned sb) { w4s_read_at<2 * W4S_PLANE>(ul, ub + sb); };        // R3
        auto rd_vmid = [&](unsigned sb) {                // R4
            w4s_read_at<W4S_PLANE>(vm[0], vb + sb);
            w4s_read_at<W4S_PLANE + 1024>(vm[1], vb + sb);
        };
        auto rd_umid = [&](unsigned sb) { w4s_read_at<W4S_PLANE>(um, ub + sb); };           // R5
        auto mma = [&](f32x4 (&c)[2], const s3_u32x4& u, const s3_u32x4 (&v)[2]) {
            const s3_bf16x8 fa = __builtin_bit_cast(s3_bf16x8, u);
            c[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, __builtin_bit_cast(s3_bf16x8, v[0]), c[0], 0, 0, 0);
            c[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, __builtin_bit_cast(s3_bf16x8, v[1]), c[1], 0, 0, 0);
        };
        if constexpr (a == 0) {              // (the first stages of passes 1 .. 5 are requested by the last stages of the pass before)
            wn_for<0, W4S_AHEAD>([&](auto X) { wn_for<0, W4S_DMA>([&](auto K) { issue_piece(decltype(K)::value, 0, 0, decltype(X)::value); }); });
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
        if constexpr (a == 0) {
            wn_wait_vmcnt<(W4S_AHEAD - 1) * W4S_DMA>();  // stage 0 has landed (mine; stages 1 .. 4 are younger), ...
            __builtin_amdgcn_s_barrier();                // ... everybody's
        }
        // (stage 0 of passes 1 .. 5 is stage g + 1 of the last step of the pass before: it landed behind that step's barrier, and its
        // slot is written again only behind the barrier of step 1 of this pass)
        __builtin_amdgcn_sched_barrier(0);
        rd_hi(std::integral_constant<int, 0>{}, 0u);     // the order R1 .. R5 in which every stage requests the next one's
        rd_vlo(0u);
        rd_ulo(0u);
        rd_vmid(0u);
        rd_umid(0u);

        for (int kc = 0; kc < nkc; ++kc) {
            const bool more = kc + 1 < nkc;              // another chunk behind this one
            wn_for<0, 6>([&](auto X) {
                constexpr int x = decltype(X)::value, set = x & 1;       // (6 is even: the hi set of stage g is x & 1)
                // Stages are numbered through the six passes, g = 6 (a nkc + kc) + x, and the ring never drains between them.
                const bool on = a < 5 || more;           // not the last lap of the kernel: every stage up to g + 6 - x exists
                const bool next = x < 5 || on;           // stage g + 1 exists
                const bool ahead = x < 1 || on;          // stage g + 5 exists: it goes into slot (x + 5) % 6, the slot of stage g - 1
                constexpr int ax = (x + W4S_AHEAD) % W4S_SLOTS;
                const int akc = x < 1 ? kc : kc + 1;     // its chunk (nkc: chunk 0 of pass a + 1)
                unsigned nb = (unsigned)((x + 1) % W4S_SLOTS) * W4S_STAGE;
                asm volatile("" : "+s"(nb));             // (added per stage: twelve fragment bases kept in registers would not fit)
                __builtin_amdgcn_sched_barrier(0);
                // The six products (U part, V part), smallest terms first, the order of conv_split3_f32. The waits count the reads
                // requested behind the ones a product needs (LDS reads return in order): R3 R4 R5 of the stage before and R1 behind
                // R2 = 7, and so on. The last stage of a pass reads the same way, into registers that nothing uses (stage 0 of the
                // next pass, which that pass reads again; after pass 5 a slot that nothing is written to any more): no branch
                // around the reads, one count for every stage.
                if (next) {
                    // stage g + 1 has to be in LDS for everybody before its fragments are read (the requests younger than its pieces
                    // are those of stages g + 2 .. g + 4; stage g + 5 is requested below); the slot of stage g - 1 is free once
                    // everybody is here. In the last lap of the kernel stages g + 2 .. exist only up to xi 5: 3, 3, 2, 1, 0.
                    constexpr int young = x < 2 ? W4S_AHEAD - 2 : x < 4 ? 4 - x : 0;
                    if (on) wn_wait_vmcnt<(W4S_AHEAD - 2) * W4S_DMA>();
                    else wn_wait_vmcnt<young * W4S_DMA>();
                    __builtin_amdgcn_s_barrier();
                }
                __builtin_amdgcn_sched_barrier(0);
                rd_hi(std::integral_constant<int, set ^ 1>{}, nb);
                asm volatile("s_waitcnt lgkmcnt(7)" : "+v"(uh[set]), "+v"(vl[0]), "+v"(vl[1]));
                mma(acc[x], uh[set], vl);                // hi lo
                __builtin_amdgcn_sched_barrier(0);
                if (ahead) issue_piece(0, a, akc, ax);
                rd_vlo(nb);
                asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(ul), "+v"(vh[set][0]), "+v"(vh[set][1]));
                __builtin_amdgcn_sched_barrier(0);
                mma(acc[x], ul, vh[set]);                // lo hi
                __builtin_amdgcn_sched_barrier(0);
                if (ahead) issue_piece(1, a, akc, ax);
                rd_ulo(nb);
                asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(um), "+v"(vm[0]), "+v"(vm[1]));
                __builtin_amdgcn_sched_barrier(0);
                mma(acc[x], um, vm);                     // mid mid
                __builtin_amdgcn_sched_barrier(0);
                if (ahead) issue_piece(2, a, akc, ax);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc[x], uh[set], vm);                // hi mid
                __builtin_amdgcn_sched_barrier(0);
                rd_vmid(nb);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc[x], um, vh[set]);                // mid hi
                __builtin_amdgcn_sched_barrier(0);
                rd_umid(nb);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc[x], uh[set], vh[set]);           // hi hi
            });
        }
        // The accumulators' last operands have arrived, and so have the reads of the last step: after passes 0 .. 4 those are the
        // fragments of the next pass's stage 0, which that pass reads again behind the fold (36 registers the fold has no room for).
        // The ring runs on: stages 0 .. 4 of the next pass are in flight during the fold below.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (a == 5) __syncthreads();               // everybody is done with the ring: the staging may overwrite it
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
        // the idle waves of a half workgroup: their DMA pieces (two per stage, the 2 KiB of one V plane; wave 7 has none), the waits and
        // the barriers of run_pass, in the same places
        constexpr int HD = 2;
        const bool mover = wave < 7;
        auto issue_half = [&](int pass, int kc, int x) {
            if (mover) {
                issue_piece(0, pass, kc, x);
                issue_piece(1, pass, kc, x);
            }
        };
        for (int x = 0; x < W4S_AHEAD; ++x) issue_half(0, 0, x);
        wn_wait_vmcnt<(W4S_AHEAD - 1) * HD>();
        __builtin_amdgcn_s_barrier();
        for (int a = 0; a < 6; ++a)
            for (int kc = 0; kc < nkc; ++kc) {
                const bool on = a < 5 || kc + 1 < nkc;       // (run_pass: on, next, the counts, ahead)
                for (int x = 0; x < 6; ++x) {
                    if (x < 5 || on) {
                        if (on || x < 2) wn_wait_vmcnt<(W4S_AHEAD - 2) * HD>();
                        else if (x == 2) wn_wait_vmcnt<2 * HD>();
                        else if (x == 3) wn_wait_vmcnt<HD>();
                        else wn_wait_vmcnt<0>();
                        __builtin_amdgcn_s_barrier();
                    }
                    if (x < 1 || on) issue_half(a, x < 1 ? kc : kc + 1, (x + W4S_AHEAD) % W4S_SLOTS);
                }
            }
        __syncthreads();
    }

    // The epilogue's thread and lane numbers are made again here (every lane of every wave is active), from the wave number in its
    // SGPR: carried through the K loops they were spilled, and the reload between two loops made the compiler wait vmcnt(0) with
    // the ring full.
    const int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    wino4_epilogue<ACT, RES>(p, smem, tab, py, wave * 64 + lane_e, nt, wm, wn, lane_e & 15, lane_e >> 4, busy);
}

// ------------------------------------------------------------------------------ host side
// Shapes that the eval plan runs on this kernel: looks at the layer's shape only, never at the batch. The rule of split3_eligible: a
// shape is listed once its median at batch 32 (tools/conv_bench.py --wino-split both --filter-planes on, 7 rounds of 20 launches,
// transform pass included, filter planes made once) improved by more than the spread of its own baseline's rounds; where that stays
// undecided, the whole forward decides (bench.py on builds that differ in the list entry alone). Measured again with the six-slot
// ring (profiles/wino4_ring; the four-slot figures are in profiles/wino4_planes_once); medians in us,
// f32 GEMMs -> bf16 planes:
//   256 -> 512 at 26 x 26     189 -> 122, with residual 196 -> 129 (baseline spread 21 - 24): listed.
//   512 -> 1024 at 13 x 13    231 -> 153, with residual 234 -> 157 (256 half workgroups; baseline spread 44 - 50): listed.
//   512 -> 1024 at 19 x 19    339 -> 244, with residual 351 -> 257 (baseline spread 36 - 45): listed.
//   128 -> 256 at 52 x 52     192 -> 145, with residual 216 -> 171 (baseline spread 22 - 24): listed.
//   64 -> 128 at 104 x 104    252 -> 233, with residual 284 -> 269 (baseline spread 31 and 28): a gain of 20 and 15, inside the spread:
//                             undecided per shape. The forward with the entry ran 9.727 - 9.758 ms against 9.731 - 9.794 without, the
//                             medians 0.015 ms apart and the ranges overlapping: not a gain, stays on the f32 GEMMs.
// conv_bench.py repeats one layer, whose filters then stay in the memory-side cache; in a forward they come from HBM, which is why the
// transform pass reads the planes ahead (wino4_touch_planes: still worth 0.4 ms of the forward with five stages in flight) and why
// the forward has the last word.
// Nothing else was measured (the 38 x 38 and 76 x 76 maps of the 608 network stay on the f32 GEMMs).
bool wino4_split_eligible(const yolo_conv_desc* d) {
    if (!wino4_split_supported(d) || d->h != d->w) return false;
    if (d->h == 26 && d->cin == 256 && d->cout == 512) return true;
    if ((d->h == 13 || d->h == 19) && d->cin == 512 && d->cout == 1024) return true;
    return d->h == 52 && d->cin == 128 && d->cout == 256;
}

// U_planes: the planes of U4 made once (YOLO_FLAG_FILTER_PLANES: the transform pass only reads them ahead and the U region of the
// workspace is left alone), or NULL: this launch makes them there
int conv_wino4s_launch(const yolo_conv_desc* d, const void* x, const float* U4, const void* U_planes, const float* scale, const float* shift,
                       const void* residual, void* y, void* workspace, size_t workspace_bytes, int32_t* nan_flag, hipStream_t s) {
    const Wino4Geom g = wino4_geom(d);
    if (!g.planes) return fail(YOLO_ERR_UNSUPPORTED, "conv winograd F(4x4) on bf16 planes: needs fp32 3x3 stride 1, NHWC output, cin %% 32 == 0");
    const size_t need = g.v_plane_bytes + g.u_plane_bytes;
    if (!workspace || workspace_bytes < need) return fail(YOLO_ERR_WORKSPACE, "conv winograd F(4x4) on bf16 planes: workspace %zu < %zu bytes", workspace_bytes, need);
    if ((size_t)workspace & 15) return fail(YOLO_ERR_ARG, "conv winograd F(4x4) on bf16 planes: workspace must be 16-byte aligned");
    if (!U4 || ((size_t)U4 & 15)) return fail(YOLO_ERR_ARG, "conv winograd F(4x4) on bf16 planes: transformed filters must be 16-byte aligned");
    if ((size_t)U_planes & 15) return fail(YOLO_ERR_ARG, "conv winograd F(4x4) on bf16 planes: filter planes must be 16-byte aligned");
    if (int rc = wino4_planes_launch(g, d, x, U4, U_planes, workspace, s)) return rc;

    Wino4SArgs q;
    Wino4Args& a = q.e;
    a = wino4_gemm_args(g, d, scale, shift, residual, y, nan_flag);
    a.V = (const float*)workspace;
    a.U = (const float*)wino4_u_planes(g, U_planes, workspace);
    q.nkc = g.nkc;
    q.xmap = a.n_whole == 0 && a.n_mt % 4 == 0 && a.n_nt % 4 == 0 && (a.n_mt / 4) * (a.n_nt / 4) % 8 == 0;
    const int grid = q.xmap ? 2 * a.n_mt * a.n_nt : wino4_grid(a);
    const bool res = d->flags & YOLO_FLAG_RESIDUAL;
    const size_t lds = (size_t)W4S_SLOTS * W4S_STAGE + W4_TAB;       // (the epilogue's staging, 256 x 68 x 4, lies over the idle ring)
    auto go = [&](auto kern) -> int {
        static LdsOnce once;
        if (int rc = reserve_lds(once, reinterpret_cast<const void*>(kern), lds, "conv_wino4s_f32")) return rc;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, s, q);
        return check_launch("conv_wino4s_f32");
    };
    YOLO_SWITCH_ACT(d->act, return res ? go(&conv_wino4s_f32<ACT, true>) : go(&conv_wino4s_f32<ACT, false>));
    return fail(YOLO_ERR_ARG, "conv winograd F(4x4) on bf16 planes: activation");
}

}  // namespace yolo
