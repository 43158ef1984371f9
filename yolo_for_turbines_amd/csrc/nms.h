// nms.h — what the stages of the batched non-max suppression share: the sorted box record, the 64-bit ordering keys, the
// constants of the chunk sort, the mask and the scan, and the host launch functions each stage offers to the dispatcher.
// One unit per stage, every one BUILT WITH -ffp-contract=off (POST_OBJS in the Makefile):
//   nms_order.hip  candidates in the reference's order: counting rank, library sort, chunk sort + rank merges; yolo_sort_u64
//   nms_mask.hip   the 64-bit suppression words (plain and class-sorted)
//   nms_scan.hip   the greedy pass over the words (plain and per class range)
//   nms_host.hip   workspace, routing (the table is there), yolo_nms
//   nms_soft.hip   yolo_soft_nms: the rescoring walk (Soft-NMS) on the candidates nms_order.hip ordered; neither mask nor scan
// Kernels are launched from the unit that defines them (no relocatable device code).
#pragma once
#include "common.h"

namespace yolo {

struct SBox { float x1, y1, x2, y2, area, cls; float w, h; };   // 32 B, sorted order

// the record of box row s = [x, y, w, h, obj, cls]
__device__ __forceinline__ SBox make_sbox(const float* s, int center) {
    float x = s[0], y = s[1];
    const float w = s[2], h = s[3];
    if (center) { x = x - w / 2.0f; y = y - h / 2.0f; }            // utils.py:60-64
    SBox o;
    o.x1 = x; o.y1 = y; o.x2 = x + w; o.y2 = y + h; o.area = w * h; o.cls = s[5]; o.w = w; o.h = h;
    return o;
}

__device__ __forceinline__ unsigned long long make_key(float score, int idx, double obj_thr) {
    if (!((double)score > obj_thr)) return ~0ull;       // filtered (also NaN): never smaller than a candidate
    score = score + 0.0f;                                // -0.0 -> +0.0 (they compare equal in Python)
    unsigned u = __float_as_uint(score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // ascending-orderable
    return ((unsigned long long)(~u) << 32) | (unsigned)idx;   // descending score, ascending index
}

// Library-sort keys (image | score field | index, nms_keys_kernel): a key is "valid" iff its score field is not all ones (only
// a NaN score could map there, and NaN is filtered), so the kernels after the sort read validity off the key and the one
// thread at the valid/filtered boundary of an image writes nvalid[b] (zeroed before): no counting atomics (2,500 same-address
// atomics per call were most of this kernel's 30 us).
__device__ __forceinline__ bool key_valid(unsigned long long k) { return ((k >> 20) & 0xffffffffull) != 0xffffffffull; }

constexpr int CLASS_BUCKETS = 4095;      // class_bucket() values: 0 .. 4093 and the lump 4094
__device__ __forceinline__ unsigned class_bucket(float c) {   // equal float classes -> equal bucket; ascending-sortable
    return (c >= 0.0f && c < 4094.0f && c == floorf(c)) ? (unsigned)c : 4094u;
}

// ---- chunk sort + rank merge (nms_order.hip)
constexpr int SC = 2048;                 // keys per chunk
constexpr int SC_MAXCH = 128;            // chunks per call: yolo_sort_u64 takes SC * SC_MAXCH = 262,144 keys; an image on the class-sorted path has at most 80 (n <= 163,456)
constexpr int SC_GROUP = 15;             // chunks ranked at once by the merge kernels (registers); more chunks: several rounds
constexpr int SC_ROW = 80;               // 8 keys (64 B) + 16 B pad per LDS row: a lane's 8 contiguous keys never share banks with its neighbours'

// ---- mask and scan
// The words of the diagonal and of the SCAN_NEAR column blocks after it are ALSO stored as near[b][rb][d][lane] (d = cb - rb):
// the scan reads exactly those for all 64 rows of a block at once, and in the mask itself they are 64 separate cache lines
// (one per row, W words apart) - an uncoalesced, HBM-latency load on the scan's serial chain; here they are 512 contiguous bytes.
constexpr int SCAN_NEAR = 3;

constexpr int MS_WAVES = 4;      // waves per workgroup = column-block stride (a 64-thread workgroup per (row block, stride) was dispatch-bound at 80
                                 // classes). Same-box A/B: 8 waves give 2 classes 540 -> 572 M boxes/s but 80 classes 1,590 -> 1,527 M; 2 waves 383 M / 1,564 M

// ---- host launch functions. boxes [b][n][6]; W = ceil(n / 64) words per mask row. Each returns YOLO_OK or what fail() returned.
// nms_order.hip: all three leave sbox[b][r] (the candidates' records in the stage's order) and nvalid[b]. The counting rank and the
// library sort (ONE radix sort of the batch) order by score, also write order[b][r] = original index and need nvalid zeroed.
int nms_order_rank(const float* boxes, int b, int n, double obj_thr, int center, int* order, SBox* sbox, int* nvalid, hipStream_t st);
size_t nms_library_sort_tmp_bytes(int b, int n);         // runs on a machine without a GPU too
int nms_order_library_sort(const float* boxes, int b, int n, double obj_thr, int center, unsigned long long* keys_in, unsigned long long* keys_out,
                           void* sort_tmp, size_t sort_tmp_bytes, int* order, SBox* sbox, int* nvalid, hipStream_t st);
// chunk sort + rank merge twice: sorted1[b][g] the candidates' keys in score order (low 32 bits: original index), then rows in
// class-major order with sorted2[b][q] (class bucket in bits 40..51), grank[b][q] = g and the class bounds of every 64-row
// block. Needs nothing zeroed: writes nvalid, chunk_valid and zeroes row_any itself.
int nms_order_class_sorted(const float* boxes, int b, int n, int W, double obj_thr, int center, unsigned long long* chunked, int* chunk_valid,
                           unsigned long long* sorted1, unsigned long long* sorted2, int* nvalid, unsigned long long* row_any, int* grank,
                           SBox* sbox, int* blk_lo, int* blk_hi, hipStream_t st);
// the class segments of order 2, for the walks that go class by class (fuse.hip, nms_soft.hip): seg[b][bucket] = {first row, one past
// the last row} of the bucket's run in sorted2, for agnostic != 0 seg[b][0] = {0, nvalid[b]}; seg (b, CLASS_BUCKETS, 2) zeroed before
int nms_class_segments(const unsigned long long* sorted2, const int* nvalid, int b, int n, int agnostic, int* seg, hipStream_t st);
// nms_mask.hip: mask[b][i][cb], and row_any[b][rb] ORed (zeroed before)
int nms_mask_plain(const SBox* sbox, const int* nvalid, int b, int n, int W, float thr, unsigned long long* mask, unsigned long long* row_any,
                   hipStream_t st);
int nms_mask_class_sorted(const SBox* sbox, const int* nvalid, const int* blk_lo, const int* blk_hi, int b, int n, int W, float thr,
                          unsigned long long* mask, unsigned long long* row_any, unsigned long long* near, hipStream_t st);
// nms_scan.hip: keep_idx[b][0 .. keep_count[b]) in the reference's order
int nms_scan_plain(const unsigned long long* mask, const int* order, const int* nvalid, const unsigned long long* row_any, int b, int n, int W,
                   int* keep_idx, int* keep_count, hipStream_t st);
int nms_class_scan_waves(int W);                         // waves per image the class scan's LDS holds at this W (at most 16); < 1: it cannot run
int nms_scan_class_sorted(const unsigned long long* mask, const unsigned long long* sorted1, const unsigned long long* sorted2, const int* nvalid,
                          const unsigned long long* row_any, const int* blk_lo, const int* blk_hi, const int* grank, const unsigned long long* near,
                          int b, int n, int W, int* keep_idx, int* keep_count, hipStream_t st);

}  // namespace yolo
