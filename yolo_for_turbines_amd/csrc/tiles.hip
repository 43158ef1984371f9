// tiles.hip — tiled detection of frames that are larger than the network input: the stages around forward + decode + NMS.
// Nothing of the reference is replaced: its dataset was cut into tiles offline (files named frame_row_column) and its
// demo only ever sees network-sized images. The frames this detector is used on are 5472 x 3648; the smallest anchors
// are 7 x 15 pixels of a 416 x 416 tile, which a letterbox of the whole frame shrinks to half a pixel.
//
//   yolo_tile_grid     host only: tile origins of one image (overlapping tiles, the last one flush with the edge)
//   yolo_tile_level_hw host only: the size of a frame's pyramid level at a scale (the rounding of resized_hw in resample.h)
//   tile_gather        one thread per output pixel: uint8 HWC frame -> fp32 CHW tiles, x (1/255), zero outside the frame
//   tile_gather_scaled the same on a resized level of the frame that is never materialised: every output pixel is resize_px of
//                      resample.h (OpenCV's fixed-point INTER_LINEAR, a 2 x 2 neighbourhood of the frame), zero outside the level
//   tile_count         per block of CT_ROWS decoded rows: how many pass the threshold and lie inside the frame
//   tile_scan          one workgroup: walks the block counts in order, one thread per image; hands every block the index of
//                      its first candidate and advances count[image]
//   tile_write         the same test again, rows remapped to the frame and stored at their index
// The order of an image's candidates is (call, tile, row): it comes from the counts and the scan, never from an atomic, and
// no workgroup waits for another (three launches). Built with -ffp-contract=off: the remap is fp32, every operation
// rounded once, and is tested bit for bit against numpy.
// yolo_tile_collect_ex runs the same three kernels (tile_count and tile_write as their EX instantiation): a tile names its
// pyramid level, the remap divides by the level's size, and a row that a tile's interior side has cut can be dropped.
#include "common.h"
#include "resample.h"

namespace yolo {

// grid (ceil(tile_h tile_w / 256), n_tiles)
__global__ __launch_bounds__(256) void tile_gather_kernel(const unsigned char* __restrict__ img, int h, int w, const int32_t* __restrict__ origins,
                                                          int tile_h, int tile_w, float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int plane = tile_h * tile_w;
    if (idx >= plane) return;
    const int t = blockIdx.y;
    const int ty = idx / tile_w;
    const int y = origins[2 * t] + ty, x = origins[2 * t + 1] + (idx - ty * tile_w);
    float v[3] = {0.f, 0.f, 0.f};
    if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) {
        const unsigned char* s = img + ((size_t)y * w + x) * 3;
        const float inv = 1.0f / 255.0f;                     // the normalisation of yolo_letterbox
        for (int c = 0; c < 3; ++c) v[c] = (float)s[c] * inv;
    }
    float* o = out + (size_t)t * 3 * plane + idx;
    for (int c = 0; c < 3; ++c) o[(size_t)c * plane] = v[c];
}

// grid as tile_gather. (y, x) is a pixel of the (lh, lw) level of the frame; with (lh, lw) == (h, w) resize_px copies the pixel.
__global__ __launch_bounds__(256) void tile_gather_scaled_kernel(const unsigned char* __restrict__ img, int h, int w, int lh, int lw,
                                                                 const int32_t* __restrict__ origins, int tile_h, int tile_w,
                                                                 float* __restrict__ out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int plane = tile_h * tile_w;
    if (idx >= plane) return;
    const int t = blockIdx.y;
    const int ty = idx / tile_w;
    const int y = origins[2 * t] + ty, x = origins[2 * t + 1] + (idx - ty * tile_w);
    float v[3] = {0.f, 0.f, 0.f};
    if ((unsigned)y < (unsigned)lh && (unsigned)x < (unsigned)lw) {
        unsigned char px[3];
        resize_px(img, h, w, lh, lw, y, x, px);
        const float inv = 1.0f / 255.0f;
        for (int c = 0; c < 3; ++c) v[c] = (float)px[c] * inv;
    }
    float* o = out + (size_t)t * 3 * plane + idx;
    for (int c = 0; c < 3; ++c) o[(size_t)c * plane] = v[c];
}

constexpr int CT_THREADS = 256;
constexpr int CT_PASSES = 4;
constexpr int CT_ROWS = CT_THREADS * CT_PASSES;              // decoded rows per block of tile_count / tile_write
constexpr int CT_WAVES = CT_THREADS / 64;
constexpr int SCAN_CHUNK = 1024;                             // block counts staged in LDS at a time by tile_scan

struct TileGeom { int image, y0, x0, H, W; };

// tiles[t] = {image, y0, x0, 0}; image outside [0, n_images) marks a tile that contributes nothing; (H, W) = hw[image].
// EX: tiles[t] = {image, y0, x0, level}; a level outside [0, n_levels) marks such a tile too; (H, W) = hw[level].
template <bool EX>
__device__ __forceinline__ bool tile_geom(const int32_t* __restrict__ tiles, const int32_t* __restrict__ hw, int n_images, int n_levels,
                                          int t, TileGeom& g) {
    g.image = tiles[4 * t];
    if ((unsigned)g.image >= (unsigned)n_images) return false;
    int at = g.image;
    if (EX) {
        at = tiles[4 * t + 3];
        if ((unsigned)at >= (unsigned)n_levels) return false;
    }
    g.y0 = tiles[4 * t + 1];
    g.x0 = tiles[4 * t + 2];
    g.H = hw[2 * at];
    g.W = hw[2 * at + 1];
    return true;
}

// The seam test, in tile pixels: the box reaches within edge_margin of a side of the tile that is not on the level's border, so
// it is (taken to be) a fragment of an object that the neighbouring tile or a coarser level sees whole. Equality is not cut,
// NaN coordinates compare false. Off for edge_margin < 0.
__device__ __forceinline__ bool tile_cut(const float* __restrict__ row, const TileGeom& g, int tile_h, int tile_w, float edge_margin) {
    if (edge_margin < 0.0f) return false;
    const float px = row[0] * (float)tile_w, pw = row[2] * (float)tile_w, hx = pw * 0.5f;
    const float left = px - hx, right = px + hx;
    const float py = row[1] * (float)tile_h, ph = row[3] * (float)tile_h, hy = ph * 0.5f;
    const float top = py - hy, bottom = py + hy;
    return (g.x0 > 0 && left < edge_margin) || ((long long)g.x0 + tile_w < g.W && right > (float)tile_w - edge_margin) ||
           (g.y0 > 0 && top < edge_margin) || ((long long)g.y0 + tile_h < g.H && bottom > (float)tile_h - edge_margin);
}

// A row is a candidate iff make_key of nms.h would rank it ((double) obj > threshold: NaN and equality are out)
// and its centre, remapped to the frame, is not in the zero padding of a tile that hangs over the edge.
// EX: and no interior side of its tile has cut it (tile_cut). tile_count and tile_write both decide here, nowhere else.
template <bool EX>
__device__ __forceinline__ bool tile_candidate(const float* __restrict__ row, const TileGeom& g, int tile_h, int tile_w, double obj_thr,
                                               float edge_margin, float& cx, float& cy) {
    if (!((double)row[4] > obj_thr)) return false;
    cx = (row[0] * (float)tile_w + (float)g.x0) / (float)g.W;
    cy = (row[1] * (float)tile_h + (float)g.y0) / (float)g.H;
    if (!(cx <= 1.0f && cy <= 1.0f)) return false;
    return !(EX && tile_cut(row, g, tile_h, tile_w, edge_margin));
}

// grid (blocks per tile, n_tiles); blk_count[tile * blocks per tile + block]
template <bool EX>
__global__ __launch_bounds__(CT_THREADS) void tile_count_kernel(const float* __restrict__ boxes, int n_per, const int32_t* __restrict__ tiles,
                                                                const int32_t* __restrict__ hw, int n_images, int n_levels, int tile_h,
                                                                int tile_w, double obj_thr, float edge_margin,
                                                                int* __restrict__ blk_count) {
    __shared__ int wave_n[CT_WAVES];
    const int t = blockIdx.y;
    TileGeom g;
    const bool live = tile_geom<EX>(tiles, hw, n_images, n_levels, t, g);      // uniform over the block
    int n = 0;
    if (live) {
        for (int p = 0; p < CT_PASSES; ++p) {
            const int r = blockIdx.x * CT_ROWS + p * CT_THREADS + threadIdx.x;
            float cx, cy;
            n += r < n_per && tile_candidate<EX>(boxes + ((size_t)t * n_per + r) * 6, g, tile_h, tile_w, obj_thr, edge_margin, cx, cy);
        }
    }
    for (int d = 32; d; d >>= 1) n += __shfl_down(n, d);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < CT_WAVES; ++k) s += wave_n[k];
        blk_count[blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// One workgroup. Thread f walks every block count in (tile, block) order and gives the blocks of image f their start:
// count[f] before the call, advanced by each of them; count[f] is left at the new total.
__global__ __launch_bounds__(256) void tile_scan_kernel(const int* __restrict__ blk_count, int* __restrict__ blk_start,
                                                        const int32_t* __restrict__ tiles, int n_blocks, int blocks_per_tile, int n_images,
                                                        int32_t* __restrict__ count) {
    __shared__ int s_cnt[SCAN_CHUNK], s_img[SCAN_CHUNK];
    for (int f0 = 0; f0 < n_images; f0 += 256) {
        const int f = f0 + threadIdx.x;
        int running = f < n_images ? count[f] : 0;
        for (int b0 = 0; b0 < n_blocks; b0 += SCAN_CHUNK) {
            const int m = n_blocks - b0 < SCAN_CHUNK ? n_blocks - b0 : SCAN_CHUNK;
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += 256) {
                s_cnt[i] = blk_count[b0 + i];
                s_img[i] = tiles[4 * ((b0 + i) / blocks_per_tile)];
            }
            __syncthreads();
            if (f < n_images) {
                for (int i = 0; i < m; ++i) {
                    if (s_img[i] == f) {
                        blk_start[b0 + i] = running;
                        running += s_cnt[i];
                    }
                }
            }
        }
        if (f < n_images) count[f] = running;
    }
}

// grid as tile_count. Rows at an index >= cap are dropped (count has already told the caller).
template <bool EX>
__global__ __launch_bounds__(CT_THREADS) void tile_write_kernel(const float* __restrict__ boxes, int n_per, const int32_t* __restrict__ tiles,
                                                                const int32_t* __restrict__ hw, int n_images, int n_levels, int tile_h,
                                                                int tile_w, double obj_thr, float edge_margin,
                                                                const int* __restrict__ blk_count, const int* __restrict__ blk_start,
                                                                float* __restrict__ cand, int cap) {
    __shared__ int wave_n[CT_PASSES][CT_WAVES];
    const int t = blockIdx.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
    TileGeom g;
    if (!tile_geom<EX>(tiles, hw, n_images, n_levels, t, g) || blk_count[blk] == 0) return;          // uniform over the block
    const int start = blk_start[blk];
    if (start >= cap) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool is[CT_PASSES];
    float cx[CT_PASSES], cy[CT_PASSES];
    int before[CT_PASSES];                                   // candidates of this pass in lower lanes of my wave
    for (int p = 0; p < CT_PASSES; ++p) {
        const int r = blockIdx.x * CT_ROWS + p * CT_THREADS + threadIdx.x;
        is[p] = r < n_per && tile_candidate<EX>(boxes + ((size_t)t * n_per + r) * 6, g, tile_h, tile_w, obj_thr, edge_margin, cx[p], cy[p]);
        const unsigned long long m = __ballot(is[p]);
        before[p] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_n[p][wave] = __popcll(m);
    }
    __syncthreads();
    int base = start;                                        // rows of a block are in (pass, wave, lane) order
    for (int p = 0; p < CT_PASSES; ++p) {
        for (int k = 0; k < CT_WAVES; ++k) {
            if (k == wave && is[p]) {
                const int at = base + before[p];
                if ((unsigned)at < (unsigned)cap) {
                    const int r = blockIdx.x * CT_ROWS + p * CT_THREADS + threadIdx.x;
                    const float* row = boxes + ((size_t)t * n_per + r) * 6;
                    float* o = cand + ((size_t)g.image * cap + at) * 6;
                    o[0] = cx[p];
                    o[1] = cy[p];
                    o[2] = (row[2] * (float)tile_w) / (float)g.W;
                    o[3] = (row[3] * (float)tile_h) / (float)g.H;
                    o[4] = row[4];
                    o[5] = row[5];
                }
            }
            base += wave_n[p][k];
        }
    }
}

// one axis of length len: the number of origins, and origin k of n
static int axis_count(int len, int tile, int overlap) {
    if (len <= tile) return 1;
    const int stride = tile - overlap;
    return (int)(((long long)len - tile + stride - 1) / stride) + 1;
}
static int axis_origin(int len, int tile, int overlap, int k, int n) {
    if (len <= tile) return 0;
    return k < n - 1 ? k * (tile - overlap) : len - tile;    // the last tile is flush with the edge
}

static size_t collect_blocks(int n_tiles, int n_per) { return (size_t)n_tiles * (size_t)ceil_div(n_per, CT_ROWS); }

// check_launch under the name of the entry that was called: "tile_collect (count)", "tile_collect_ex (count)", ...
static int collect_check(const char* who, const char* kernel) {
    char what[48];
    snprintf(what, sizeof what, "%s (%s)", who, kernel);
    return check_launch(what);
}

// the three launches of yolo_tile_collect (hw = img_hw) and yolo_tile_collect_ex (hw = level_hw)
template <bool EX>
static int collect_launch(const char* who, const float* boxes, int n_tiles, int n_per, const int32_t* tiles, const int32_t* hw, int n_images,
                          int n_levels, int tile_h, int tile_w, double obj_threshold, float edge_margin, float* cand, int cap, int32_t* count,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (n_tiles < 0 || n_per < 0 || n_images <= 0 || tile_h <= 0 || tile_w <= 0 || cap < 0) return fail(YOLO_ERR_ARG, "%s: bad sizes", who);
    if (n_tiles == 0 || n_per == 0) return YOLO_OK;
    if (!boxes || !tiles || !hw || !cand || !count) return fail(YOLO_ERR_ARG, "%s: null pointer", who);
    const size_t need = yolo_tile_collect_workspace_bytes(n_tiles, n_per);
    if (!workspace || workspace_bytes < need) return fail(YOLO_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    const size_t n_blocks = collect_blocks(n_tiles, n_per);
    if (n_tiles > 65535 || n_blocks > 0x7fffffffull || (size_t)n_tiles * n_per > 0x7fffffffull)
        return fail(YOLO_ERR_UNSUPPORTED, "%s: %d tiles of %d rows in one call", who, n_tiles, n_per);
    hipStream_t st = (hipStream_t)stream;
    int* blk_count = (int*)workspace;
    int* blk_start = blk_count + n_blocks;
    const int bpt = ceil_div(n_per, CT_ROWS);
    const dim3 grid(bpt, n_tiles);
    hipLaunchKernelGGL(tile_count_kernel<EX>, grid, dim3(CT_THREADS), 0, st, boxes, n_per, tiles, hw, n_images, n_levels, tile_h, tile_w,
                       obj_threshold, edge_margin, blk_count);
    int rc = collect_check(who, "count");
    if (rc) return rc;
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(256), 0, st, (const int*)blk_count, blk_start, tiles, (int)n_blocks, bpt, n_images, count);
    rc = collect_check(who, "scan");
    if (rc) return rc;
    hipLaunchKernelGGL(tile_write_kernel<EX>, grid, dim3(CT_THREADS), 0, st, boxes, n_per, tiles, hw, n_images, n_levels, tile_h, tile_w,
                       obj_threshold, edge_margin, (const int*)blk_count, (const int*)blk_start, cand, cap);
    return collect_check(who, "write");
}

}  // namespace yolo

using namespace yolo;

extern "C" {

int yolo_tile_grid(int h, int w, int tile_h, int tile_w, int overlap_h, int overlap_w, int32_t* origins_yx, int cap) {
    if (h <= 0 || w <= 0 || tile_h <= 0 || tile_w <= 0) return fail(YOLO_ERR_ARG, "tile_grid: sizes must be positive");
    if (overlap_h < 0 || overlap_h >= tile_h || overlap_w < 0 || overlap_w >= tile_w)
        return fail(YOLO_ERR_ARG, "tile_grid: 0 <= overlap < tile does not hold (%d of %d, %d of %d)", overlap_h, tile_h, overlap_w, tile_w);
    const int ny = axis_count(h, tile_h, overlap_h), nx = axis_count(w, tile_w, overlap_w);
    if ((long long)ny * nx > 0x7fffffffll) return fail(YOLO_ERR_ARG, "tile_grid: %d x %d tiles", ny, nx);
    if (!origins_yx) return ny * nx;
    if (cap < ny * nx) return fail(YOLO_ERR_ARG, "tile_grid: %d x %d tiles, room for %d", ny, nx, cap);
    for (int i = 0; i < ny; ++i) {
        const int y0 = axis_origin(h, tile_h, overlap_h, i, ny);
        for (int j = 0; j < nx; ++j) {
            origins_yx[2 * ((size_t)i * nx + j)] = y0;
            origins_yx[2 * ((size_t)i * nx + j) + 1] = axis_origin(w, tile_w, overlap_w, j, nx);
        }
    }
    return ny * nx;
}

int yolo_tile_gather(const unsigned char* img_hwc, int h, int w, const int32_t* origins_yx, int n_tiles, int tile_h, int tile_w, float* out,
                     void* stream) {
    if (h <= 0 || w <= 0 || tile_h <= 0 || tile_w <= 0 || n_tiles < 0) return fail(YOLO_ERR_ARG, "tile_gather: bad sizes");
    if (n_tiles == 0) return YOLO_OK;
    if (!img_hwc || !origins_yx || !out) return fail(YOLO_ERR_ARG, "tile_gather: null pointer");
    if ((long long)tile_h * tile_w > 0x7fffffffll - 256 || n_tiles > 65535) return fail(YOLO_ERR_UNSUPPORTED, "tile_gather: grid too large");
    hipLaunchKernelGGL(tile_gather_kernel, dim3(ceil_div(tile_h * tile_w, 256), n_tiles), dim3(256), 0, (hipStream_t)stream, img_hwc, h, w,
                       origins_yx, tile_h, tile_w, out);
    return check_launch("tile_gather");
}

int yolo_tile_level_hw(int h, int w, double scale, int* level_h, int* level_w) {
    if (h <= 0 || w <= 0 || !level_h || !level_w) return fail(YOLO_ERR_ARG, "tile_level_hw: bad sizes");
    if (!(scale > 0.0 && scale <= 8.0)) return fail(YOLO_ERR_ARG, "tile_level_hw: scale %g is not in (0, 8]", scale);      // NaN too
    const double lh = rint(h * scale), lw = rint(w * scale);                    // half to even, as resized_hw
    if (lh > 2147483647.0 || lw > 2147483647.0) return fail(YOLO_ERR_ARG, "tile_level_hw: %g x %g does not fit an int", lh, lw);
    *level_h = lh < 1.0 ? 1 : (int)lh;
    *level_w = lw < 1.0 ? 1 : (int)lw;
    return YOLO_OK;
}

int yolo_tile_gather_scaled(const unsigned char* img_hwc, int h, int w, int level_h, int level_w, const int32_t* origins_yx, int n_tiles,
                            int tile_h, int tile_w, float* out, void* stream) {
    if (h <= 0 || w <= 0 || level_h <= 0 || level_w <= 0 || tile_h <= 0 || tile_w <= 0 || n_tiles < 0)
        return fail(YOLO_ERR_ARG, "tile_gather_scaled: bad sizes");
    if (n_tiles == 0) return YOLO_OK;
    if (!img_hwc || !origins_yx || !out) return fail(YOLO_ERR_ARG, "tile_gather_scaled: null pointer");
    if ((long long)tile_h * tile_w > 0x7fffffffll - 256 || n_tiles > 65535)
        return fail(YOLO_ERR_UNSUPPORTED, "tile_gather_scaled: grid too large");
    hipLaunchKernelGGL(tile_gather_scaled_kernel, dim3(ceil_div(tile_h * tile_w, 256), n_tiles), dim3(256), 0, (hipStream_t)stream, img_hwc, h,
                       w, level_h, level_w, origins_yx, tile_h, tile_w, out);
    return check_launch("tile_gather_scaled");
}

size_t yolo_tile_collect_workspace_bytes(int n_tiles, int n_per) {
    if (n_tiles <= 0 || n_per <= 0) return 0;
    return 2 * sizeof(int) * collect_blocks(n_tiles, n_per);                    // blk_count, blk_start
}

int yolo_tile_collect(const float* boxes, int n_tiles, int n_per, const int32_t* tiles, const int32_t* img_hw, int n_images, int tile_h,
                      int tile_w, double obj_threshold, float* cand, int cap, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream) {
    return collect_launch<false>("tile_collect", boxes, n_tiles, n_per, tiles, img_hw, n_images, 0, tile_h, tile_w, obj_threshold, -1.0f, cand,
                                 cap, count, workspace, workspace_bytes, stream);
}

int yolo_tile_collect_ex(const float* boxes, int n_tiles, int n_per, const int32_t* tiles, const int32_t* level_hw, int n_levels,
                         int n_images, int tile_h, int tile_w, double obj_threshold, float edge_margin, float* cand, int cap,
                         int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_levels <= 0) return fail(YOLO_ERR_ARG, "tile_collect_ex: n_levels must be positive");
    if (edge_margin != edge_margin) return fail(YOLO_ERR_ARG, "tile_collect_ex: edge_margin is NaN");
    return collect_launch<true>("tile_collect_ex", boxes, n_tiles, n_per, tiles, level_hw, n_images, n_levels, tile_h, tile_w, obj_threshold,
                                edge_margin, cand, cap, count, workspace, workspace_bytes, stream);
}

}  // extern "C"
