// nms_scan.hip — NMS stage 3: the greedy pass over the suppression words.   BUILD WITH -ffp-contract=off.
//
// A box is kept iff no kept box before it suppresses it: the one sequential part of greedy NMS. Both kernels walk the 64-row
// blocks in order, resolve a block's diagonal word serially with readlane broadcasts and OR the kept rows' words into a
// removed-bitmap held in LDS; they write the kept boxes' original indices in the reference's order (descending score).
//   nms_scan_kernel          one workgroup per image over rows in score order (plain mask)
//   nms_scan_classes_kernel  class-major rows (class-sorted mask): classes never interact, so every class range gets a wave or a
//                            team of waves of its own; the kept rows go back to score order through their global ranks
#include "nms.h"

namespace yolo {

// The serial step of a 64-row block: lane t holds row t's diagonal word d (0 for a row outside the range), rem the rows
// already removed (uniform). Only rows with a diagonal bit can change the outcome, and only while they are not removed
// themselves: dropping the removed rows from the walk after every step makes its length the number of KEPT rows with a
// diagonal bit (clustered boxes: all 64 rows have one, two or three survive - the walk was most of the scan there).
__device__ __forceinline__ unsigned long long resolve_diagonal(unsigned long long d, unsigned long long rem) {
    unsigned long long cand = __ballot(d != 0ull) & ~rem;
    const unsigned dlo = (unsigned)d, dhi = (unsigned)(d >> 32);
    while (cand) {
        const int t = __builtin_ctzll(cand);
        const unsigned wl = __builtin_amdgcn_readlane(dlo, t);
        const unsigned wh = __builtin_amdgcn_readlane(dhi, t);
        rem |= ((unsigned long long)wh << 32) | wl;
        cand &= cand - 1ull;
        cand &= ~rem;
    }
    return rem;
}

// one 256-thread workgroup per image. Per 64-row block: wave 0 resolves the diagonal word (the only
// sequential part of greedy NMS; skipped outright when no row of the block has a diagonal bit and none
// is already removed), then every thread owns column words and ORs in the rows that are kept AND have
// any suppression bit at all (row_any, written by the mask kernel) — with many classes most rows
// suppress nothing and cost no memory traffic.
__global__ __launch_bounds__(256) void nms_scan_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ order,
                                                       const int* __restrict__ nvalid, const unsigned long long* __restrict__ row_any,
                                                       int n, int W, int* __restrict__ keep_idx, int* __restrict__ keep_count) {
    extern __shared__ unsigned long long removed[];     // [W] + 2 words: kept broadcast, kept-and-nonzero broadcast
    const int b = blockIdx.x;
    const int nv = nvalid[b];
    const int tid = threadIdx.x;
    for (int c = tid; c < W + 2; c += 256) removed[c] = 0;
    __syncthreads();
    const unsigned long long* mk = mask + (size_t)b * n * W;
    const unsigned long long* any = row_any + (size_t)b * W;
    const int* ord = order + (size_t)b * n;
    int* out = keep_idx + (size_t)b * n;
    int count = 0;                                      // meaningful in wave 0 only
    const int nblk = (nv + 63) / 64;
    // the row block's diagonal words, row_any word and original indices are fetched ONE block ahead: the loop is a serial
    // chain of ~160 iterations per image, and a dependent global load per iteration was most of each iteration
    unsigned long long d_next = 0ull, any_next = 0ull;
    int ord_next = 0;
    if (tid < 64 && nblk > 0) {
        d_next = tid < nv ? mk[(size_t)tid * W] : 0ull;
        any_next = any[0];
        ord_next = tid < nv ? ord[tid] : 0;
    }
    for (int rb = 0; rb < nblk; ++rb) {
        const int rows = nv - rb * 64 < 64 ? nv - rb * 64 : 64;
        if (tid < 64) {
            const int i = rb * 64 + tid;
            const unsigned long long d = d_next, any_rb = any_next;
            const int ord_i = ord_next;
            if (rb + 1 < nblk) {
                const int in = i + 64;
                d_next = in < nv ? mk[(size_t)in * W + rb + 1] : 0ull;
                any_next = any[rb + 1];
                ord_next = in < nv ? ord[in] : 0;
            }
            unsigned long long rem = removed[rb];
            const unsigned long long rowmask = rows == 64 ? ~0ull : ((1ull << rows) - 1ull);
            unsigned long long kept;
            if (__ballot(d != 0ull) == 0ull) {
                kept = rowmask & ~rem;                  // nothing inside this block suppresses anything
            } else {
                kept = rowmask & ~resolve_diagonal(d, rem);
            }
            if (tid < rows && ((kept >> tid) & 1ull)) {
                const int pos = count + __popcll(kept & ((1ull << tid) - 1ull));
                out[pos] = ord_i;
            }
            count += __popcll(kept);
            if (tid == 0) {
                removed[W] = kept;
                removed[W + 1] = kept & any_rb;         // kept rows that suppress something in a later block
            }
        }
        __syncthreads();
        unsigned long long work = removed[W + 1];
        if (work) {
            for (int c = rb + 1 + tid; c < nblk; c += 256) {     // column blocks >= nblk were never written
                unsigned long long acc = 0;
                unsigned long long wk = work;
                while (wk) {
                    const int t = __builtin_ctzll(wk);
                    wk &= wk - 1;
                    acc |= mk[(size_t)(rb * 64 + t) * W + c];
                }
                if (acc) removed[c] |= acc;             // column c is owned by exactly this thread
            }
        }
        __syncthreads();
    }
    if (tid == 0) keep_count[b] = count;
}

// ---- scan for class-sorted rows: classes never interact, so the image's rows are cut at class boundaries into up to 16
// ranges of about equal length and ONE WAVE runs the greedy pass over each range, with no workgroup barrier inside the
// loop (the per-image chain of ~160 row blocks becomes ~10 per wave at 80 classes; with 2 classes two waves work).
// A 64-row block that straddles a cut is visited by both neighbours, each with its own row mask. Kept rows are reported
// as bits of an LDS word array (ds_or: straddling blocks) and emitted in global score order at the end of the kernel.
constexpr int SCAN_MLP = 8;

// ---- few classes: a TEAM of waves per class range ------------------------------------------------------------------------
// With 2 classes only 2 of an image's 16 waves had a range, and each spent its time waiting for the kept rows' mask words
// (5-6 dependent rounds of loads per 64-row block, ~2.2 us per block, 78 blocks in a chain). When at most half the waves
// have a range, every range gets G = K / ranges waves: a leader that walks the serial chain and G - 1 helpers that do the
// far pushes, talking through LDS (all waves of a workgroup are resident, so a spin on an LDS word cannot deadlock; LDS
// operations of one wave execute in order, so "data, then counter" needs no wait in between):
//   * columns rb + 1 .. rb + SCAN_NEAR of row block rb are the leader's: it loads the 64 rows' words of those columns
//     UNCONDITIONALLY two iterations ahead (no dependence on which rows are kept) and, once the kept word of block rb - d is
//     known, ORs the kept rows' words together across the wave (DPP) - no memory latency on the chain;
//   * columns beyond belong to the helpers, in S sets that take the row blocks in turn (block k -> set k % S): the leader
//     publishes kept & row_any of block rb in a ring, the helpers of that set split its rows (t % P), OR the words into the
//     team's removed[] (ds_or) and report the block done. The leader only needs block rb - SCAN_NEAR - 1 finished before it
//     resolves block rb, and it reads the progress counters and removed[rb + 1] one iteration early (counters first: if they
//     pass, the word read after them is complete), so no LDS round trip sits on the chain either.
constexpr int SCAN_RING = 8;                // > SCAN_NEAR + 1: the leader is never further ahead of a helper than that
constexpr int SCAN_HELP_MLP = 16;           // rows in flight per helper (x 2 column slices)

__device__ __forceinline__ unsigned wave_or32(unsigned v) {       // OR over the 64 lanes (all active), result wave-uniform
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);     // row_half_mirror
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);     // row_mirror: every lane holds its row's OR
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) | (unsigned)__builtin_amdgcn_readlane((int)v, 16) |
           (unsigned)__builtin_amdgcn_readlane((int)v, 32) | (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
}

// one member of a team; returns the number of kept rows (leader) or 0 (helpers). `removed` is the team's word array, `ctrl`
// its control block (both zeroed): ring[SCAN_RING] u64, then int pub, pad, int prog[H]. `single`: the range is one class
// bucket, so every word the team touches was written by the mask kernel. Byte offsets into the image's mask are 32-bit.
__device__ __forceinline__ int scan_team(const unsigned long long* __restrict__ mk, const unsigned long long* __restrict__ any,
                                         const int* lo, const int* hi, int W, int s0, int s1, bool single, unsigned long long* removed,
                                         unsigned long long* ctrl, int member, int H, int lane, unsigned long long* keptw_b,
                                         const unsigned long long* __restrict__ near_b) {
    // relaxed workgroup-scope atomics, not volatile: the address-space inference leaves volatile accesses as flat loads
    unsigned long long* ring = ctrl;
    int* pub = (int*)(ctrl + SCAN_RING);
    int* prog = pub + 2;
    auto ld = [](const int* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto st = [](int* q, int v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    const int rb0 = s0 >> 6, rb1 = (s1 - 1) >> 6;
    const unsigned W8 = (unsigned)W * 8u;
    const char* mkb = reinterpret_cast<const char*>(mk);
    const int S = H >= 6 ? 3 : (H >= 2 ? 2 : 1);
    auto rows_of = [&](int rb) -> unsigned long long {   // rows of block rb inside [s0, s1)
        const int a = s0 - rb * 64 > 0 ? s0 - rb * 64 : 0, z = s1 - rb * 64 < 64 ? s1 - rb * 64 : 64;
        const unsigned long long upto = z == 64 ? ~0ull : ((1ull << z) - 1ull);
        return upto & ~((1ull << a) - 1ull);
    };
    if (member == 0) {
        // branch-free prefetch: the address is clamped into the range's rows and column blocks and the word is masked when it
        // is used (a load under a branch makes the compiler wait for vmcnt(0), i.e. for the prefetches just issued, too)
        auto word_of = [&](int rr, int c) -> unsigned long long {       // row rr * 64 + lane, column block c = rr + d, d <= SCAN_NEAR
            const int rs = rr < rb0 ? rb0 : (rr > rb1 ? rb1 : rr);      // any valid address; what is out of range is never used
            return near_b[(size_t)((rs * (SCAN_NEAR + 1) + (c - rr)) * 64 + lane)];
        };
        auto near_ok = [&](int rr, int c) -> bool { return single || lo[c] <= hi[rr > rb0 ? rr : rb0]; };   // else never written
        // two register sets, used alternately (the loop is unrolled by two): a set is consumed and then refilled for the block
        // two iterations ahead, so no in-flight load result is ever copied (a rotation n0 = n1 would wait for vmcnt(0))
        // row_any through the VECTOR memory path: a scalar load shares lgkmcnt with LDS and returns out of order, so every wait for
        // an LDS word would also wait for the s_load just issued - a global-memory latency on the chain, every iteration
        int vzero;
        asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
        struct Pre { unsigned long long d, a, n[SCAN_NEAR]; };
        auto fill = [&](Pre& p, int c) {
            p.d = word_of(c, c);
            p.a = any[(c < rb1 ? c : rb1) + vzero];
#pragma unroll
            for (int q = 0; q < SCAN_NEAR; ++q) p.n[q] = word_of(c - (q + 1), c);
        };
        Pre X, Y;
        fill(X, rb0);
        fill(Y, rb0 + 1);
        unsigned long long kp[SCAN_NEAR];              // kept words of blocks rb - 1, rb - 2, ... (0 before the range)
#pragma unroll
        for (int q = 0; q < SCAN_NEAR; ++q) kp[q] = 0ull;
        int count = 0;
        const int lane_set = lane % S;
        int needv = 0, phase = 0;                       // per lane (= helper): blocks that helper must have finished
        int pg = 0;                                     // its progress counter, read one iteration early ...
        unsigned long long rv = removed[rb0];           // ... followed by the removed word of the block
        auto iter = [&](int rb, Pre& p) {
            const int k = rb - rb0;
            const unsigned long long rowmask = rows_of(rb);
            const unsigned long long d = ((rowmask >> lane) & 1ull) ? p.d : 0ull, any_rb = uniform64(p.a);
            unsigned long long v = 0ull;
#pragma unroll
            for (int q = 0; q < SCAN_NEAR; ++q) v |= (near_ok(rb - (q + 1), rb) && ((kp[q] >> lane) & 1ull)) ? p.n[q] : 0ull;
            const unsigned long long near_rem = ((unsigned long long)wave_or32((unsigned)(v >> 32)) << 32) | wave_or32((unsigned)v);
            fill(p, rb + 2);
            const int kk = k - SCAN_NEAR - 1;           // the block whose far pushes become necessary now (its set: kk % S)
            if (kk >= 0) {
                if (lane_set == phase) needv = kk + 1;
                phase = phase + 1 == S ? 0 : phase + 1;
            }
            if (__ballot(lane < H && pg < needv) != 0ull) {          // a helper is behind: wait, then read the word again
                do {
                    __builtin_amdgcn_s_sleep(1);
                    pg = lane < H ? ld(prog + lane) : 0x7fffffff;
                } while (__ballot(lane < H && pg < needv) != 0ull);
                asm volatile("" ::: "memory");
                rv = removed[rb];
            }
            unsigned long long rem = uniform64(rv) | near_rem;
            {                                                        // next block's counters, then its word (in this order)
                pg = lane < H ? ld(prog + lane) : 0x7fffffff;
                asm volatile("" ::: "memory");
                rv = removed[rb + 1 <= rb1 ? rb + 1 : rb1];
            }
            const unsigned long long kept = rowmask & ~resolve_diagonal(d, rem);
            const unsigned long long work = kept & any_rb;
            if (lane == 0) {
                __hip_atomic_store(ring + (k & (SCAN_RING - 1)), work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                asm volatile("" ::: "memory");          // the ring entry before the counter (in-order LDS: no wait needed)
                st(pub, k + 1);
                if (kept) atomicOr(&keptw_b[rb], kept);
            }
            count += __popcll(kept);
#pragma unroll
            for (int q = SCAN_NEAR - 1; q > 0; --q) kp[q] = kp[q - 1];
            kp[0] = kept;
        };
        for (int rb = rb0; rb <= rb1; rb += 2) {
            iter(rb, X);
            if (rb + 1 <= rb1) iter(rb + 1, Y);
        }
        return count;
    }
    const int h = member - 1;
    const int set = h % S, part = h / S, P = (H - set + S - 1) / S;      // this helper: part `part` of the P helpers of its set
    const unsigned long long sel = __ballot(lane % P == part);
    for (int k = set; k <= rb1 - rb0; k += S) {
        const int rb = rb0 + k;
        while (__builtin_amdgcn_readfirstlane(ld(pub)) <= k) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
        const unsigned long long work = uniform64(__hip_atomic_load(ring + (k & (SCAN_RING - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) & sel;
        if (work) {
            const int hi_r = hi[rb];
            const char* blkp = mkb + (size_t)((unsigned)(rb * 64) * W8);
            for (int cb = rb + SCAN_NEAR + 1; cb <= rb1; cb += 128) {           // two column slices (lane, lane + 64) per pass
                const int c0 = cb + lane, c1 = c0 + 64;
                const int cc0 = c0 < rb1 ? c0 : rb1, cc1 = c1 < rb1 ? c1 : rb1;   // clamped: unconditional loads, masked below
                const bool ok0 = c0 <= rb1 && (single || lo[cc0] <= hi_r);       // else never written: classes above this row block's
                const bool ok1 = c1 <= rb1 && (single || lo[cc1] <= hi_r);
                const unsigned o0 = (unsigned)cc0 * 8u, o1 = (unsigned)cc1 * 8u;
                unsigned long long acc0 = 0ull, acc1 = 0ull, wk = work;
                int tl = 0;
                if (__ballot(ok1) != 0ull) {
                    while (wk) {                        // SCAN_HELP_MLP rows' words in flight (a spent slot repeats the last row)
                        unsigned long long w0[SCAN_HELP_MLP], w1[SCAN_HELP_MLP];
#pragma unroll
                        for (int u = 0; u < SCAN_HELP_MLP; ++u) {
                            if (wk) { tl = __builtin_ctzll(wk); wk &= wk - 1ull; }
                            const char* rowp = blkp + (size_t)((unsigned)tl * W8);
                            w0[u] = *reinterpret_cast<const unsigned long long*>(rowp + o0);
                            w1[u] = *reinterpret_cast<const unsigned long long*>(rowp + o1);
                        }
#pragma unroll
                        for (int u = 0; u < SCAN_HELP_MLP; ++u) { acc0 |= w0[u]; acc1 |= w1[u]; }
                    }
                } else {
                    while (wk) {
                        unsigned long long w0[SCAN_HELP_MLP];
#pragma unroll
                        for (int u = 0; u < SCAN_HELP_MLP; ++u) {
                            if (wk) { tl = __builtin_ctzll(wk); wk &= wk - 1ull; }
                            w0[u] = *reinterpret_cast<const unsigned long long*>(blkp + (size_t)((unsigned)tl * W8) + o0);
                        }
#pragma unroll
                        for (int u = 0; u < SCAN_HELP_MLP; ++u) acc0 |= w0[u];
                    }
                }
                if (ok0 && acc0) atomicOr(&removed[c0], acc0);       // several helpers share a word
                if (ok1 && acc1) atomicOr(&removed[c1], acc1);
            }
        }
        asm volatile("" ::: "memory");                  // the ORs before the progress counter (in-order LDS)
        if (lane == 0) st(prog + h, k + 1);
    }
    return 0;
}

__global__ __launch_bounds__(1024) void nms_scan_classes_kernel(const unsigned long long* __restrict__ mask,
                                                               const unsigned long long* __restrict__ sorted2,
                                                               const int* __restrict__ nvalid, const unsigned long long* __restrict__ row_any,
                                                               const int* __restrict__ blk_lo, const int* __restrict__ blk_hi, int n, int W,
                                                               const int* __restrict__ grank, int* __restrict__ keep_count,
                                                               const unsigned long long* __restrict__ near,
                                                               const unsigned long long* __restrict__ sorted1, int* __restrict__ keep_idx) {
    extern __shared__ unsigned long long lds[];         // [K][W] removed words per wave, kept[W], then lo[W], hi[W] (int), the count, cuts
    const int b = blockIdx.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, K = blockDim.x >> 6;
    const int nv = nvalid[b];
    const int nblk = (nv + 63) / 64;
    unsigned long long* removed = lds + (size_t)wave * W;
    unsigned long long* keptl = lds + (size_t)K * W;    // [W] kept rows, bit q % 64 of word q / 64 (ds_or: a block that straddles a cut has two writers)
    int* lo = (int*)(lds + (size_t)(K + 1) * W);
    int* hi = lo + W;
    int* total = hi + W;
    for (int c = tid; c < (K + 1) * W; c += blockDim.x) lds[c] = 0ull;
    for (int c = tid; c < nblk; c += blockDim.x) { lo[c] = blk_lo[(size_t)b * W + c]; hi[c] = blk_hi[(size_t)b * W + c]; }
    if (tid == 0) *total = 0;
    __syncthreads();
    // range of this wave: cuts at the first class boundary at or after k nv / K (upper bound of the bucket just before it).
    // Wave k - 1 finds cut k: the first block that STARTS above the target's bucket from the block classes in LDS, then the
    // exact row with one 64-key load of the block before it (a per-thread binary search over the keys was ~14 dependent
    // global loads, 10+ us before any wave could start).
    const unsigned long long* keys = sorted2 + (size_t)b * n;
    int* cuts = total + 1;                              // [K + 1]
    if (tid == 0) { cuts[0] = 0; cuts[K] = nv; }
    if (wave + 1 < K) {
        const int target = (int)((long long)nv * (wave + 1) / K);
        int res = 0;
        if (target > 0) {
            const int bucket = (int)(unsigned)((keys[target - 1] >> 40) & 0xfffull);      // uniform
            const int tb = target >> 6;
            int c = nblk;                               // first block after tb whose first row is above the bucket
            for (int c0 = tb + 1; c0 < nblk; c0 += 64) {
                const unsigned long long above = __ballot(c0 + lane < nblk && lo[c0 + lane] > bucket);
                if (above) { c = c0 + __builtin_ctzll(above); break; }
            }
            const int q = (c - 1) * 64 + lane;          // the boundary is inside block c - 1 or at the start of block c
            const bool in = q >= target && q < nv;
            const unsigned long long key = keys[in ? q : target - 1];
            const unsigned long long above = __ballot(in && (int)(unsigned)((key >> 40) & 0xfffull) > bucket);
            res = above ? (c - 1) * 64 + __builtin_ctzll(above) : (c * 64 < nv ? c * 64 : nv);
        }
        if (lane == 0) cuts[wave + 1] = res;
    }
    __syncthreads();
    int R = 0;                                          // ranges that hold rows
    for (int k = 0; k < K; ++k) R += cuts[k] < cuts[k + 1] ? 1 : 0;
    const int G = (R > 0 && 2 * R <= K && (unsigned long long)n * W * 8ull < (1ull << 32)) ? K / R : 1;   // teams use 32-bit byte offsets
    const unsigned long long* mk = mask + (size_t)b * n * W;
    const unsigned long long* any = row_any + (size_t)b * W;
    int s0 = 0, s1 = 0;
    int count = 0;
    if (G >= 2) {                                       // few classes: teams of G waves (see scan_team)
        const int team = wave / G, member = wave - team * G;
        if (team < R) {
            int idx = -1;
            for (int k = 0; k < K; ++k)
                if (cuts[k] < cuts[k + 1] && ++idx == team) { s0 = cuts[k]; s1 = cuts[k + 1]; }
            unsigned long long* team_removed = lds + (size_t)(team * G) * W;       // the leader's array; the first helper's holds the control block
            const bool single = ((keys[s0] >> 40) & 0xfffull) == ((keys[s1 - 1] >> 40) & 0xfffull);
            count = scan_team(mk, any, lo, hi, W, s0, s1, single, team_removed, team_removed + W, member, G - 1, lane, keptl,
                              near + (size_t)b * W * (SCAN_NEAR + 1) * 64);
        }
        s0 = s1 = 0;
    } else {
        s0 = cuts[wave]; s1 = cuts[wave + 1];
    }
    if (s0 < s1) {
        const int rb0 = s0 >> 6, rb1 = (s1 - 1) >> 6;
        auto rows_of = [&](int rb) -> unsigned long long {   // rows of block rb inside [s0, s1)
            const int a = s0 - rb * 64 > 0 ? s0 - rb * 64 : 0, z = s1 - rb * 64 < 64 ? s1 - rb * 64 : 64;
            const unsigned long long upto = z == 64 ? ~0ull : ((1ull << z) - 1ull);
            return upto & ~((1ull << a) - 1ull);
        };
        const unsigned long long* diag = near + (size_t)b * W * (SCAN_NEAR + 1) * 64 + lane;      // block rb's diagonal words: diag[rb * (NEAR + 1) * 64]
        unsigned long long d_next = ((rows_of(rb0) >> lane) & 1ull) ? diag[(size_t)rb0 * (SCAN_NEAR + 1) * 64] : 0ull;
        unsigned long long any_next = any[rb0];
        for (int rb = rb0; rb <= rb1; ++rb) {
            const unsigned long long rowmask = rows_of(rb);
            const unsigned long long d = d_next, any_rb = any_next;
            if (rb < rb1) {
                d_next = ((rows_of(rb + 1) >> lane) & 1ull) ? diag[(size_t)(rb + 1) * (SCAN_NEAR + 1) * 64] : 0ull;
                any_next = any[rb + 1];
            }
            const unsigned long long rem_v = removed[rb];   // wave-uniform: keep the serial chain on the scalar unit
            const unsigned rem_lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)rem_v);
            const unsigned rem_hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(rem_v >> 32));
            unsigned long long rem = ((unsigned long long)rem_hi << 32) | rem_lo;
            const unsigned long long kept = rowmask & ~resolve_diagonal(d, rem);
            count += __popcll(kept);
            if (lane == 0 && kept) atomicOr(&keptl[rb], kept);
            const unsigned long long work_v = kept & any_rb;  // kept rows with a bit in some later column block
            // wave-uniform by construction; said so to the compiler, which otherwise walks the row bits with ~12 VALU
            // instructions + a 64-bit multiply per row and lane. Scalar: s_ff1 / s_andn2 per row, the row base in SGPRs and
            // the lane's column as the 32-bit offset of the load.
            const unsigned long long work = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(work_v >> 32)) << 32) |
                                            (unsigned)__builtin_amdgcn_readfirstlane((unsigned)work_v);
            if (work) {
                const int hi_r = hi[rb];
                const unsigned long long* blkp = mk + (size_t)rb * 64 * W;
                for (unsigned c = (unsigned)(rb + 1 + lane); (int)c <= rb1; c += 64) {
                    if (lo[c] > hi_r) break;            // never written: classes above this row block's
                    unsigned long long acc = 0ull, wk = work;
                    int tl = 0;
                    while (wk) {                        // SCAN_MLP rows' words in flight (a spent slot repeats the last row)
                        unsigned long long wv[SCAN_MLP];
#pragma unroll
                        for (int u = 0; u < SCAN_MLP; ++u) {
                            if (wk) { tl = __builtin_ctzll(wk); wk &= wk - 1ull; }
                            wv[u] = blkp[(size_t)tl * W + c];
                        }
#pragma unroll
                        for (int u = 0; u < SCAN_MLP; ++u) acc |= wv[u];
                    }
                    if (acc) removed[c] |= acc;         // this lane owns word c of this wave's array
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own LDS writes before its next read
        }
    }
    if (lane == 0 && count) atomicAdd(total, count);
    __syncthreads();
    if (tid == 0) keep_count[b] = *total;
    // Output: the kept boxes' original indices in global score order (the reference's order).
    const int* gr = grank + (size_t)b * n;
    // Mark the kept rows' GLOBAL RANKS in an LDS bitmap (ds_or instead of a scattered global store per kept box), prefix the
    // words' popcounts, and let thread g emit rank g - coalesced loads of the rank's key in order 1 (its low bits are the
    // original index) and coalesced stores. (A slot array indexed by rank + a separate compaction launch did this before:
    // 5 + 10 us of the 115 us at 80 classes.)
    unsigned long long* krank = lds;                 // the removed[] arrays are dead
    int* wpre = lo;                                  // and so are the block class bounds
    for (int c = tid; c < W; c += blockDim.x) krank[c] = 0ull;
    __syncthreads();
    for (int q0 = 0; q0 < nv; q0 += 4 * (int)blockDim.x) {
        int g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {               // unconditional loads, four in flight
            const int q = q0 + u * (int)blockDim.x + tid;
            g[u] = gr[q < nv ? q : nv - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * (int)blockDim.x + tid;
            if (q < nv && ((keptl[q >> 6] >> (q & 63)) & 1ull)) atomicOr(&krank[g[u] >> 6], 1ull << (g[u] & 63));
        }
    }
    __syncthreads();
    if (wave == 0) {                                 // exclusive prefix of the words' popcounts, (W + 63) / 64 words per lane
        const int per = (W + 63) >> 6, w0 = lane * per;
        int sum = 0;
        for (int c = 0; c < per; ++c) sum += w0 + c < W ? __popcll(krank[w0 + c]) : 0;
        int inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        int run = inc - sum;
        for (int c = 0; c < per; ++c)
            if (w0 + c < W) { wpre[w0 + c] = run; run += __popcll(krank[w0 + c]); }
    }
    __syncthreads();
    const unsigned long long* ord1 = sorted1 + (size_t)b * n;
    int* out = keep_idx + (size_t)b * n;
    for (int g0 = 0; g0 < nv; g0 += 4 * (int)blockDim.x) {
        unsigned long long key[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * (int)blockDim.x + tid;
            key[u] = ord1[g < nv ? g : nv - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * (int)blockDim.x + tid;
            if (g < nv) {
                const unsigned long long w = krank[g >> 6];
                if ((w >> (g & 63)) & 1ull) out[wpre[g >> 6] + __popcll(w & ((1ull << (g & 63)) - 1ull))] = (int)(unsigned)(key[u] & 0xffffffffull);
            }
        }
    }
}

// ---- host side
int nms_scan_plain(const unsigned long long* mask, const int* order, const int* nvalid, const unsigned long long* row_any, int b, int n, int W,
                   int* keep_idx, int* keep_count, hipStream_t st) {
    hipLaunchKernelGGL(nms_scan_kernel, dim3(b), dim3(256), (size_t)(W + 2) * 8, st, mask, order, nvalid, row_any, n, W, keep_idx, keep_count);
    return check_launch("nms_scan");
}

// LDS of nms_scan_classes_kernel in the 60 KiB a workgroup may ask for without an attribute: kept words, lo / hi, count, cuts ...
static size_t class_scan_fixed_lds(int W) { return (size_t)W * 16 + 128; }
constexpr long long SCAN_LDS = 60 * 1024;

int nms_class_scan_waves(int W) {                        // ... and one removed[] array of W words per wave
    const int K = (int)((SCAN_LDS - (long long)class_scan_fixed_lds(W)) / (long long)((size_t)W * 8));
    return K > 16 ? 16 : K;
}

int nms_scan_class_sorted(const unsigned long long* mask, const unsigned long long* sorted1, const unsigned long long* sorted2, const int* nvalid,
                          const unsigned long long* row_any, const int* blk_lo, const int* blk_hi, const int* grank, const unsigned long long* near,
                          int b, int n, int W, int* keep_idx, int* keep_count, hipStream_t st) {
    const int K = nms_class_scan_waves(W);
    hipLaunchKernelGGL(nms_scan_classes_kernel, dim3(b), dim3(64 * K), (size_t)K * W * 8 + class_scan_fixed_lds(W), st, mask, sorted2, nvalid,
                       row_any, blk_lo, blk_hi, n, W, grank, keep_count, near, sorted1, keep_idx);
    return check_launch("nms_scan_classes");
}

}  // namespace yolo
