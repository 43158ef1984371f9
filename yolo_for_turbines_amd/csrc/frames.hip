// frames.hip — the batched frame front end: a pool of RGB24 / BGR24 / NV12 frames and a device table of their places become the
// network's input in one launch (yolo_frames_letterbox), packed RGB at source resolution (yolo_frames_to_rgb), and the boxes of a
// letterboxed batch go back to their frames (yolo_boxes_to_frames). The contract is in include/yolo_mi355x.h and DESIGN.md 7.26.
//
// The pixels are "convert the frame to packed RGB uint8, then yolo_letterbox_hw it", to the bit: the sizes (resized_hw) and the
// coefficients (lin_coef) are those of resample.h; the two lines that blend four taps restate the body of its resize_px, which reads
// its taps from a packed image and so cannot take converted ones. PARITY UNPINNED, as for preprocess.hip: neither the resize nor the
// NV12 conversion was run against cv2; both follow OpenCV's published integer arithmetic and are tested against tests/frames_ref.py.
// Build with -ffp-contract=off (resample.h).
#include <climits>
#include <cstdint>
#include "common.h"
#include "resample.h"

namespace yolo {

constexpr int kFramesTileW = 64, kFramesTileH = 16;          // output pixels per workgroup: 16 lanes x 4 pixels across, 16 rows
constexpr int kFramesThreads = 256;
constexpr int kFramesMaxHW = 16384;                          // yolo_frames_to_rgb, the limit of yolo_draw_boxes

// Y'CbCr -> R'G'B' in 20-bit fixed point (OpenCV's form): y = max(0, Y - yoff) cy, R = clip((y + 2^19 + cvr v) >> 20), ...
struct Csc { int cy, cvr, cvg, cug, cub, yoff; };
// BT.601 limited: OpenCV's ITUR_BT_601_* literals. The others: round(c 2^20) of the exact coefficients from Kr, Kb.
static const Csc kCsc[4] = {
    {1220542, 1673527, -852492, -409993, 2116026, 16},       // YOLO_CSC_BT601
    {1048576, 1470104, -748826, -360853, 1858077, 0},        // YOLO_CSC_BT601_FULL
    {1220945, 1879825, -558796, -223607, 2215014, 16},       // YOLO_CSC_BT709
    {1048576, 1651297, -490864, -196424, 1945738, 0},        // YOLO_CSC_BT709_FULL
};

__device__ __forceinline__ int clip_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// pixel (y, x) of a frame as R, G, B in 0 .. 255; base: the frame's first byte
template <int FMT>
__device__ __forceinline__ void tap_rgb(const unsigned char* __restrict__ base, int h, int pitch, int y, int x, const Csc& k, int px[3]) {
    if constexpr (FMT == YOLO_FRAMES_NV12) {
        const unsigned char* uv = base + ((size_t)h + (size_t)(y >> 1)) * (size_t)pitch + (size_t)(x & ~1);
        const int Y = base[(size_t)y * (size_t)pitch + (size_t)x];
        const int u = (int)uv[0] - 128, v = (int)uv[1] - 128;
        const int yy = (Y > k.yoff ? Y - k.yoff : 0) * k.cy + (1 << 19);
        px[0] = clip_u8((yy + k.cvr * v) >> 20);
        px[1] = clip_u8((yy + k.cvg * v + k.cug * u) >> 20);
        px[2] = clip_u8((yy + k.cub * u) >> 20);
    } else {
        const unsigned char* p = base + (size_t)y * (size_t)pitch + (size_t)x * 3;
        px[0] = p[FMT == YOLO_FRAMES_BGR24 ? 2 : 0];
        px[1] = p[1];
        px[2] = p[FMT == YOLO_FRAMES_BGR24 ? 0 : 2];
    }
}

// One workgroup per 64 x 16 tile of one frame's canvas; blockIdx.x = frame * tiles_per_frame + tile. Lane l of a wave holds pixels
// 4 (l % 16) .. + 3 of row l / 16 of the wave's four rows, so a wave writes four 256-byte row segments per plane, 16 bytes a lane.
template <int FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_letterbox_kernel(const unsigned char* __restrict__ pool,
                                                                           const yolo_frame_row* __restrict__ table, int size, int CH, int CW,
                                                                           int tiles_x, int tiles_per_frame, Csc k, int vec,
                                                                           float* __restrict__ out, int32_t* __restrict__ meta_out) {
    __shared__ int sx0[kFramesTileW], sx1[kFramesTileW], sa[kFramesTileW];          // source columns; a0 | a1 << 16
    __shared__ int sy0[kFramesTileH], sy1[kFramesTileH], sb[kFramesTileH];          // source rows; b0 | b1 << 16
    const int tid = threadIdx.x;
    const int f = blockIdx.x / tiles_per_frame, t = blockIdx.x - f * tiles_per_frame;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int oy0 = ty * kFramesTileH, ox0 = tx * kFramesTileW;
    const yolo_frame_row row = table[f];
    const int h = row.h, w = row.w, pitch = row.pitch;
    int nh, nw;
    resized_hw(h, w, size, &nh, &nw);
    const int pad_top = (CH - nh) / 2, pad_left = (CW - nw) / 2;
    if (t == 0 && tid == 0 && meta_out) {
        int32_t* m = meta_out + (size_t)f * 6;
        m[0] = h; m[1] = w; m[2] = nh; m[3] = nw; m[4] = pad_top; m[5] = pad_left;
    }
    const int r = tid >> 4, oy = oy0 + r, ox = ox0 + (tid & 15) * 4;
    float* const o = out + ((size_t)f * 3 * CH + oy) * (size_t)CW + ox;
    const size_t plane = (size_t)CH * CW;
    const bool mine = oy < CH && ox < CW;
    // a tile wholly in the padding: zeros, nothing is read
    if (oy0 >= pad_top + nh || oy0 + kFramesTileH <= pad_top || ox0 >= pad_left + nw || ox0 + kFramesTileW <= pad_left) {
        if (!mine) return;
        for (int c = 0; c < 3; ++c) {
            if (vec) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{0.f, 0.f, 0.f, 0.f};
            else for (int e = 0; e < 4 && ox + e < CW; ++e) o[c * plane + e] = 0.f;
        }
        return;
    }
    const bool ident = nh == h && nw == w;                    // resize_px copies; lin_coef at scale 1 would give the same bytes
    if (tid < kFramesTileW) {
        const int x = ox0 + tid - pad_left;
        int x0 = 0, x1 = 0, a0 = 0, a1 = 0;
        if ((unsigned)x < (unsigned)nw) {
            if (ident) { x0 = x1 = x; }
            else lin_coef(x, (double)w / nw, w, &x0, &x1, &a0, &a1);
        }
        sx0[tid] = x0; sx1[tid] = x1; sa[tid] = a0 | (a1 << 16);
    } else if (tid < kFramesTileW + kFramesTileH) {
        const int i = tid - kFramesTileW, y = oy0 + i - pad_top;
        int y0 = 0, y1 = 0, b0 = 0, b1 = 0;
        if ((unsigned)y < (unsigned)nh) {
            if (ident) { y0 = y1 = y; }
            else lin_coef(y, (double)h / nh, h, &y0, &y1, &b0, &b1);
        }
        sy0[i] = y0; sy1[i] = y1; sb[i] = b0 | (b1 << 16);
    }
    __syncthreads();
    if (!mine) return;
    const unsigned char* base = pool + row.offset;
    const int y = oy - pad_top;
    const bool row_in = (unsigned)y < (unsigned)nh;
    const int y0 = sy0[r], y1 = sy1[r], b0 = sb[r] & 0xffff, b1 = sb[r] >> 16;
    float v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int x = ox + e - pad_left;
        v[0][e] = v[1][e] = v[2][e] = 0.f;
        if (!row_in || (unsigned)x >= (unsigned)nw) continue;
        const int j = (tid & 15) * 4 + e;
        int px[3];
        if (ident) {
            tap_rgb<FMT>(base, h, pitch, y0, sx0[j], k, px);
        } else {
            const int x0 = sx0[j], x1 = sx1[j], a0 = sa[j] & 0xffff, a1 = sa[j] >> 16;
            int p00[3], p01[3], p10[3], p11[3];
            tap_rgb<FMT>(base, h, pitch, y0, x0, k, p00);
            tap_rgb<FMT>(base, h, pitch, y0, x1, k, p01);
            tap_rgb<FMT>(base, h, pitch, y1, x0, k, p10);
            tap_rgb<FMT>(base, h, pitch, y1, x1, k, p11);
            for (int c = 0; c < 3; ++c) {                     // resize_px of resample.h on the converted taps
                const int r0 = p00[c] * a0 + p01[c] * a1;
                const int r1 = p10[c] * a0 + p11[c] * a1;
                const int s = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                px[c] = clip_u8(s);
            }
        }
        const float inv = 1.0f / 255.0f;                      // the normalisation of letterbox_kernel
        for (int c = 0; c < 3; ++c) v[c][e] = (float)px[c] * inv;
    }
    for (int c = 0; c < 3; ++c) {
        if (vec) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
        else for (int e = 0; e < 4 && ox + e < CW; ++e) o[c * plane + e] = v[c][e];
    }
}

// four consecutive pixels of a frame per thread, 12 bytes as three dwords where the destination allows it
template <int FMT>
__global__ __launch_bounds__(kFramesThreads) void frames_to_rgb_kernel(const unsigned char* __restrict__ pool,
                                                                        const yolo_frame_row* __restrict__ table, int h, int w,
                                                                        int blocks_per_frame, Csc k, unsigned char* __restrict__ out) {
    const int f = blockIdx.x / blocks_per_frame;
    const long long npx = (long long)h * w;
    const long long p0 = ((long long)(blockIdx.x - f * blocks_per_frame) * kFramesThreads + threadIdx.x) * 4;
    if (p0 >= npx) return;
    const yolo_frame_row row = table[f];
    const unsigned char* base = pool + row.offset;
    const int cnt = npx - p0 < 4 ? (int)(npx - p0) : 4;
    unsigned char b[12];
    for (int e = 0; e < cnt; ++e) {
        const long long p = p0 + e;
        const int y = (int)(p / w), x = (int)(p - (long long)y * w);
        int px[3];
        tap_rgb<FMT>(base, h, row.pitch, y, x, k, px);
        for (int c = 0; c < 3; ++c) b[3 * e + c] = (unsigned char)px[c];
    }
    unsigned char* dst = out + ((size_t)f * (size_t)npx + (size_t)p0) * 3;
    if (cnt == 4 && ((uintptr_t)dst & 3) == 0) {
        unsigned int* d = reinterpret_cast<unsigned int*>(dst);
        for (int q = 0; q < 3; ++q)
            d[q] = (unsigned)b[4 * q] | ((unsigned)b[4 * q + 1] << 8) | ((unsigned)b[4 * q + 2] << 16) | ((unsigned)b[4 * q + 3] << 24);
    } else {
        for (int q = 0; q < 3 * cnt; ++q) dst[q] = b[q];
    }
}

// unletterbox_boxes(..., meta=): fp64 on the fp32 inputs in the order of the Python expression, one rounding to fp32
__global__ __launch_bounds__(kFramesThreads) void boxes_to_frames_kernel(const float* boxes, long long rows, int n,
                                                                          const int32_t* __restrict__ meta, int CH, int CW,
                                                                          float* out) {          // out may be boxes
    const long long i = (long long)blockIdx.x * kFramesThreads + threadIdx.x;
    if (i >= rows) return;
    const int32_t* m = meta + (i / n) * 6;
    const int new_h = m[2], new_w = m[3], pad_h = m[4], pad_w = m[5];
    const float* b = boxes + i * 6;
    float* o = out + i * 6;
    o[0] = (float)(((double)b[0] * CW - pad_w) / new_w);
    o[1] = (float)(((double)b[1] * CH - pad_h) / new_h);
    o[2] = (float)(((double)b[2] * CW) / new_w);
    o[3] = (float)(((double)b[3] * CH) / new_h);
    o[4] = b[4];
    o[5] = b[5];
}

static int frames_args(const char* what, const void* pool, const void* table, int n, int format, int csc) {
    if (!pool || !table || ((uintptr_t)table & 7) || n < 1) return fail(YOLO_ERR_ARG, "%s: bad arguments", what);
    if (format != YOLO_FRAMES_RGB24 && format != YOLO_FRAMES_BGR24 && format != YOLO_FRAMES_NV12)
        return fail(YOLO_ERR_ARG, "%s: unknown format %d", what, format);
    if (csc < 0 || csc > YOLO_CSC_BT709_FULL) return fail(YOLO_ERR_ARG, "%s: unknown csc %d", what, csc);
    return YOLO_OK;
}

}  // namespace yolo

using namespace yolo;

extern "C" {

void yolo_frames_tile(int* w, int* h) {
    if (w) *w = kFramesTileW;
    if (h) *h = kFramesTileH;
}

int yolo_frames_csc_constants(int csc, int32_t* out6) {
    if (!out6 || csc < 0 || csc > YOLO_CSC_BT709_FULL) return fail(YOLO_ERR_ARG, "frames_csc_constants: bad arguments");
    const Csc& k = kCsc[csc];
    out6[0] = k.cy; out6[1] = k.cvr; out6[2] = k.cvg; out6[3] = k.cug; out6[4] = k.cub; out6[5] = k.yoff;
    return YOLO_OK;
}

int yolo_frames_letterbox(const uint8_t* pool, const yolo_frame_row* table, int n, int format, int csc, int size, int canvas_h,
                          int canvas_w, float* out, int32_t* meta_out, void* stream) {
    if (int rc = frames_args("frames_letterbox", pool, table, n, format, csc)) return rc;
    if (!out || size <= 0 || canvas_h <= 0 || canvas_w <= 0) return fail(YOLO_ERR_ARG, "frames_letterbox: bad arguments");
    const int tiles_x = ceil_div(canvas_w, kFramesTileW);
    const long long tiles = (long long)tiles_x * ceil_div(canvas_h, kFramesTileH);
    if (tiles * n > INT_MAX) return fail(YOLO_ERR_ARG, "frames_letterbox: %d frames of %d x %d exceed the grid", n, canvas_h, canvas_w);
    const int vec = canvas_w % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)(tiles * n)), block(kFramesThreads);
    const hipStream_t s = (hipStream_t)stream;
#define YOLO_FRAMES_LAUNCH(FMT)                                                                                                       \
    hipLaunchKernelGGL(frames_letterbox_kernel<FMT>, grid, block, 0, s, pool, table, size, canvas_h, canvas_w, tiles_x, (int)tiles, \
                       kCsc[csc], vec, out, meta_out)
    if (format == YOLO_FRAMES_NV12) YOLO_FRAMES_LAUNCH(YOLO_FRAMES_NV12);
    else if (format == YOLO_FRAMES_BGR24) YOLO_FRAMES_LAUNCH(YOLO_FRAMES_BGR24);
    else YOLO_FRAMES_LAUNCH(YOLO_FRAMES_RGB24);
#undef YOLO_FRAMES_LAUNCH
    return check_launch("frames_letterbox");
}

int yolo_frames_to_rgb(const uint8_t* pool, const yolo_frame_row* table, int n, int h, int w, int format, int csc, uint8_t* out,
                       void* stream) {
    if (int rc = frames_args("frames_to_rgb", pool, table, n, format, csc)) return rc;
    if (!out || h < 1 || w < 1 || h > kFramesMaxHW || w > kFramesMaxHW) return fail(YOLO_ERR_ARG, "frames_to_rgb: bad arguments");
    if (format == YOLO_FRAMES_NV12 && ((h | w) & 1)) return fail(YOLO_ERR_ARG, "frames_to_rgb: NV12 needs even sizes, got %d x %d", h, w);
    const long long bpf = ((long long)h * w + 4 * kFramesThreads - 1) / (4 * kFramesThreads);
    if (bpf * n > INT_MAX) return fail(YOLO_ERR_ARG, "frames_to_rgb: %d frames of %d x %d exceed the grid", n, h, w);
    const dim3 grid((unsigned)(bpf * n)), block(kFramesThreads);
    const hipStream_t s = (hipStream_t)stream;
#define YOLO_FRAMES_LAUNCH(FMT) \
    hipLaunchKernelGGL(frames_to_rgb_kernel<FMT>, grid, block, 0, s, pool, table, h, w, (int)bpf, kCsc[csc], out)
    if (format == YOLO_FRAMES_NV12) YOLO_FRAMES_LAUNCH(YOLO_FRAMES_NV12);
    else if (format == YOLO_FRAMES_BGR24) YOLO_FRAMES_LAUNCH(YOLO_FRAMES_BGR24);
    else YOLO_FRAMES_LAUNCH(YOLO_FRAMES_RGB24);
#undef YOLO_FRAMES_LAUNCH
    return check_launch("frames_to_rgb");
}

int yolo_boxes_to_frames(const float* boxes, int b, int n, const int32_t* meta, int canvas_h, int canvas_w, float* out, void* stream) {
    if (b < 1 || n < 0 || !meta || canvas_h <= 0 || canvas_w <= 0 || (n > 0 && (!boxes || !out)))
        return fail(YOLO_ERR_ARG, "boxes_to_frames: bad arguments");
    if (n == 0) return YOLO_OK;
    const long long rows = (long long)b * n, blocks = (rows + kFramesThreads - 1) / kFramesThreads;
    if (blocks > INT_MAX) return fail(YOLO_ERR_ARG, "boxes_to_frames: %d x %d rows exceed the grid", b, n);
    hipLaunchKernelGGL(boxes_to_frames_kernel, dim3((unsigned)blocks), dim3(kFramesThreads), 0, (hipStream_t)stream, boxes, rows, n, meta,
                       canvas_h, canvas_w, out);
    return check_launch("boxes_to_frames");
}

}  // extern "C"
