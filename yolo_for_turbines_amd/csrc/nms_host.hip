// nms_host.hip — batched non-max suppression: workspace, routing and yolo_nms.   BUILD WITH -ffp-contract=off.
//
// Replaces (reference file:line): non_max_suppression code/utils.py:150-191 with calc_iou :38-84. Kept set and order are
// identical to the reference for any fp32 input: a stable descending order of the objectness scores, the objectness threshold
// compared as Python floats (double), the reference's fp32 IoU (nms_mask.hip). All images of the batch are in flight at once
// and nothing goes back to the host. Three stages, one unit each (nms.h): order -> mask -> scan. Which kernels run them depends
// on the size, n boxes per image (W = ceil(n / 64) mask words per row) and b images:
//
//   n                    b         order                          mask            scan
//   < 2,048              any       counting rank                  plain           plain
//   any                  > 2,047   counting rank                  plain           plain
//   2,048 .. 163,456     <= 2,047  chunk sort + rank merge, x 2   class-sorted    per class range
//   163,457 .. 491,392   <= 2,047  one library sort               plain           plain
//   > 491,392            any       YOLO_ERR_UNSUPPORTED
//
// The cuts follow from the constants: 2,048 = SC, one chunk (below it the O(n^2) rank is cheaper than any sort); b <= 2,047 is
// the image field of the sort keys; the class scan holds one removed[] array of W words per wave beside 16 W + 128 bytes in 60 KiB
// of LDS, so it has at least one wave while 24 W + 128 <= 61,440: W <= 2,554, n <= 163,456 (nms_class_scan_waves); the plain scan
// holds W + 2 words in the same 60 KiB: W <= 7,678, n <= 491,392.
// Data is tiny (n x 24 B in, <= n x 4 B out); the bound is VALU pair work and the serial scan, not HBM.
#include "nms.h"

namespace yolo {

enum class NmsPath { Rank, ClassSorted, LibrarySort };

static NmsPath nms_path(int b, int n) {
    const bool key_fields = n < (1 << 20) && b <= 2047;     // the sort keys' index field has 20 bits, their image field 11
    if (n < SC || !key_fields) return NmsPath::Rank;         // small n: counting is cheaper than sorting
    return nms_class_scan_waves(ceil_div(n, 64)) >= 1 ? NmsPath::ClassSorted : NmsPath::LibrarySort;
}

// zero_bytes: nvalid + row_any + chunk_valid lead the workspace, zeroed by one memset per call on the two paths that need it
struct NmsWs { int* nvalid; unsigned long long* row_any; int* order; SBox* sbox; unsigned long long* mask; size_t zero_bytes; size_t total;
               unsigned long long* keys_in; unsigned long long* keys_out; void* sort_tmp; size_t sort_tmp_bytes;
               int* grank; int* blk_lo; int* blk_hi; int* chunk_valid; unsigned long long* chunked;
               unsigned long long* sorted2; unsigned long long* near; };

static NmsWs carve(void* base, int b, int n) {
    const int W = ceil_div(n > 0 ? n : 1, 64);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return (char*)base + o; };
    NmsWs w;
    w.nvalid = (int*)take(sizeof(int) * (size_t)(b > 0 ? b : 1));
    w.row_any = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)(b > 0 ? b : 1) * W);
    w.chunk_valid = (int*)take(sizeof(int) * (size_t)(b > 0 ? b : 1) * SC_MAXCH);
    w.zero_bytes = off;
    w.order = (int*)take(sizeof(int) * (size_t)b * n);
    w.sbox = (SBox*)take(sizeof(SBox) * (size_t)b * n);
    w.mask = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * n * W);
    w.keys_in = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * n);
    w.keys_out = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)b * n);       // library sort: its output; class-sorted: order 1
    w.sort_tmp_bytes = (b > 0 && n > 0) ? nms_library_sort_tmp_bytes(b, n) : 0;
    w.sort_tmp = take(w.sort_tmp_bytes ? w.sort_tmp_bytes : 8);
    w.grank = (int*)take(sizeof(int) * (size_t)b * n);
    w.blk_lo = (int*)take(sizeof(int) * (size_t)(b > 0 ? b : 1) * W);
    w.blk_hi = (int*)take(sizeof(int) * (size_t)(b > 0 ? b : 1) * W);
    const bool chunks = b > 0 && n > 0 && nms_path(b, n) == NmsPath::ClassSorted;
    w.chunked = (unsigned long long*)take(chunks ? sizeof(unsigned long long) * (size_t)b * ceil_div(n, SC) * SC : 8);
    w.sorted2 = (unsigned long long*)take(chunks ? sizeof(unsigned long long) * (size_t)b * n : 8);
    w.near = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)(b > 0 ? b : 1) * W * (SCAN_NEAR + 1) * 64);
    w.total = off;
    return w;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

size_t yolo_nms_workspace_bytes(int b, int n) {
    if (b <= 0 || n < 0) return 0;
    return carve(nullptr, b, n).total;
}

int yolo_nms(const float* boxes, int b, int n, double iou_threshold, double obj_threshold, int center, int32_t* keep_idx,
             int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
    if (b <= 0 || n < 0 || !keep_count) return fail(YOLO_ERR_ARG, "nms: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(keep_count, 0, sizeof(int) * (size_t)b, st) != hipSuccess) return fail(YOLO_ERR_LAUNCH, "nms: memset");
        return YOLO_OK;
    }
    if (!boxes || !keep_idx || !workspace) return fail(YOLO_ERR_ARG, "nms: null pointer");
    const NmsWs w = carve(workspace, b, n);
    if (workspace_bytes < w.total) return fail(YOLO_ERR_WORKSPACE, "nms: workspace %zu < %zu bytes", workspace_bytes, w.total);
    const int W = ceil_div(n, 64);
    if ((size_t)(W + 2) * 8 > 60 * 1024) return fail(YOLO_ERR_UNSUPPORTED, "nms: n = %d too large", n);
    if (b > 65535 || W > 65535) return fail(YOLO_ERR_UNSUPPORTED, "nms: grid too large");
    const float thr = (float)iou_threshold;
    const NmsPath path = nms_path(b, n);
    int rc;
    if (path == NmsPath::ClassSorted) {                    // the ordering kernels zero what they need
        rc = nms_order_class_sorted(boxes, b, n, W, obj_threshold, center, w.chunked, w.chunk_valid, w.keys_out, w.sorted2, w.nvalid,
                                    w.row_any, w.grank, w.sbox, w.blk_lo, w.blk_hi, st);
        if (!rc) rc = nms_mask_class_sorted(w.sbox, w.nvalid, w.blk_lo, w.blk_hi, b, n, W, thr, w.mask, w.row_any, w.near, st);
        if (!rc) rc = nms_scan_class_sorted(w.mask, w.keys_out, w.sorted2, w.nvalid, w.row_any, w.blk_lo, w.blk_hi, w.grank, w.near, b, n, W,
                                            keep_idx, keep_count, st);
        return rc;
    }
    if (hipMemsetAsync(w.nvalid, 0, w.zero_bytes, st) != hipSuccess) return fail(YOLO_ERR_LAUNCH, "nms: memset");
    if (path == NmsPath::LibrarySort)
        rc = nms_order_library_sort(boxes, b, n, obj_threshold, center, w.keys_in, w.keys_out, w.sort_tmp, w.sort_tmp_bytes, w.order, w.sbox,
                                    w.nvalid, st);
    else
        rc = nms_order_rank(boxes, b, n, obj_threshold, center, w.order, w.sbox, w.nvalid, st);
    if (!rc) rc = nms_mask_plain(w.sbox, w.nvalid, b, n, W, thr, w.mask, w.row_any, st);
    if (!rc) rc = nms_scan_plain(w.mask, w.order, w.nvalid, w.row_any, b, n, W, keep_idx, keep_count, st);
    return rc;
}

}  // extern "C"
