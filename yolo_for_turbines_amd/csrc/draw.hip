// Draws detections and tracks onto uint8 HWC frames (yolo_draw_boxes; the contract is in include/yolo_mi355x.h and DESIGN.md 7.25).
// Two launches. draw_commands: one thread per (frame, selected row) turns the row into one fixed-size command record (integer
// rectangles, colour, label text) and the rectangle that bounds everything the command paints. draw_tiles: one workgroup per
// DRAW_TW x DRAW_TH pixel tile gathers the commands that touch the tile into LDS, in command order, and every thread composites
// its own pixels in registers. So each pixel is read once and written at most once whatever the number of boxes, there are no
// atomics, the painter's order is the selection order, and the result does not depend on scheduling.
// Compiled with -ffp-contract=off: every fp32 operation of the geometry is rounded once.
#include "common.h"

namespace yolo {

constexpr int DRAW_TW = 128, DRAW_TH = 32;     // the pixel tile of one workgroup (yolo_draw_tile)
constexpr int DRAW_THREADS = 256;              // 32 runs of 4 pixels across x 8 rows; a thread owns one run in each of 4 row groups
constexpr int DRAW_RUNS = DRAW_TW / 4, DRAW_ROWS = DRAW_THREADS / DRAW_RUNS, DRAW_GROUPS = DRAW_TH / DRAW_ROWS;
constexpr int DRAW_CHUNK = DRAW_THREADS;       // commands tested per round, one per thread (yolo_draw_chunk)
constexpr int DRAW_BATCH = 32;                 // hits composited per round: their records are staged in LDS
constexpr int DRAW_TEXT = 32;                  // characters a record holds
constexpr int DRAW_REC = 24;                   // 32-bit words of a record
constexpr int DRAW_MAX_HW = 16384, DRAW_MAX_B = 65535, DRAW_MAX_N = 1 << 24, DRAW_MAX_T = 64, DRAW_MAX_S = 8;
constexpr float DRAW_CLAMP = 1048576.f;        // 2^20: the edges are clamped to +-2^20 pixels before they become integers
static_assert(DRAW_RUNS * 4 == DRAW_TW && DRAW_ROWS * DRAW_GROUPS == DRAW_TH && DRAW_RUNS * DRAW_ROWS == DRAW_THREADS, "tile shape");
static_assert(DRAW_THREADS == 256 && DRAW_CHUNK == DRAW_THREADS, "four waves, one command per thread and round");
static_assert(DRAW_BATCH * (DRAW_REC / 4) + DRAW_BATCH <= DRAW_THREADS, "six threads stage a record, the last DRAW_BATCH threads the rectangles");

// A record, 24 words: 0..3 outer x0 y0 x1 y1 (x1, y1 exclusive), 4..7 inner, 8..11 plate, 12 colour r | g << 8 | b << 16,
// 13 line_alpha | fill_alpha << 8, 14 text length | font_scale << 8, 15 zero, 16..23 the text. All zero: draws nothing.
enum { R_OUTER = 0, R_INNER = 4, R_PLATE = 8, R_COLOUR = 12, R_ALPHA = 13, R_TEXT_LEN = 14, R_TEXT = 16 };

// the workspace: [nsel: b int32, padded to 16 bytes][bounds: b n int4][records: b n 24 int32]
static size_t draw_header_bytes(int b) { return ((size_t)b * sizeof(int) + 15) & ~(size_t)15; }

static const unsigned char hFont[95][8] = {
#include "draw_font.inc"
};
__device__ __attribute__((aligned(16))) const unsigned char dFont[96][8] = {
#include "draw_font.inc"
};

struct DrawArgs {
    const float* boxes;
    const int* keep;
    const int* count;
    const int* ids;
    const int* meta;
    const unsigned char* names;
    const unsigned char* palette;
    int* nsel;
    int4* bounds;
    int* recs;
    int n, center, h, w, canvas_h, canvas_w;
    int thickness, scale, line_alpha, fill_alpha, labels, scores, by_id;
    int n_classes, name_width, n_colors;
};

__device__ __forceinline__ bool draw_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }       // false for NaN
__device__ __forceinline__ int draw_edge(float v) {
    v = fminf(fmaxf(v, -DRAW_CLAMP), DRAW_CLAMP);
    return (int)floorf(v + 0.5f);
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_commands_kernel(const DrawArgs a) {
    const int b = blockIdx.y, j = blockIdx.x * DRAW_THREADS + threadIdx.x, n = a.n;
    int cnt = n;
    if (a.count) cnt = min(max(a.count[b], 0), n);
    if (j == 0) a.nsel[b] = cnt;
    if (j >= cnt) return;
    const size_t slot = (size_t)b * n + j;
    int4* rec4 = reinterpret_cast<int4*>(a.recs + slot * DRAW_REC);
    const int4 zero = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < DRAW_REC / 4; ++q) rec4[q] = zero;
    a.bounds[slot] = zero;

    const int row = a.keep ? a.keep[slot] : j;
    if (row < 0 || row >= n) return;
    const float* p = a.boxes + ((size_t)b * n + row) * 6;
    float a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
    const float score = p[4], cls = p[5];
    const float W = (float)a.w, H = (float)a.h;
    if (a.meta) {                              // unletterbox_boxes(..., meta=): letterboxed canvas -> the original frame
        const int* m = a.meta + (size_t)b * 6;
        const float nh = (float)m[2], nw = (float)m[3], pt = (float)m[4], pl = (float)m[5];
        const float cw = (float)a.canvas_w, ch = (float)a.canvas_h;
        a0 = (a0 * cw - pl) / nw;
        a1 = (a1 * ch - pt) / nh;
        if (a.center) {
            a2 = (a2 * cw) / nw;
            a3 = (a3 * ch) / nh;
        } else {
            a2 = (a2 * cw - pl) / nw;
            a3 = (a3 * ch - pt) / nh;
        }
    }
    float l, t, r, bt;
    if (a.center) {
        const float hw = a2 / 2.f, hh = a3 / 2.f;
        l = (a0 - hw) * W;
        r = (a0 + hw) * W;
        t = (a1 - hh) * H;
        bt = (a1 + hh) * H;
    } else {
        l = a0 * W;
        t = a1 * H;
        r = a2 * W;
        bt = a3 * H;
    }
    if (!draw_finite(l) || !draw_finite(t) || !draw_finite(r) || !draw_finite(bt) || r < l || bt < t) return;
    const int x0 = draw_edge(l), y0 = draw_edge(t), x1 = draw_edge(r), y1 = draw_edge(bt);

    const int id = a.ids ? a.ids[(size_t)b * n + row] : 0;
    const int ci = fabsf(cls) <= 1073741824.f ? (int)cls : -1;           // NaN, Inf and beyond 2^30: no class
    const bool named = a.labels && a.names;
    if (named && (ci < 0 || ci >= a.n_classes)) return;
    int k = (a.by_id ? id : ci) % a.n_colors;
    if (k < 0) k += a.n_colors;
    const unsigned char* pal = a.palette + 3 * k;
    const int colour = pal[0] | pal[1] << 8 | pal[2] << 16;

    const int grow = a.thickness / 2, shrink = a.thickness - grow;
    const int ox0 = x0 - grow, oy0 = y0 - grow, ox1 = x1 + grow, oy1 = y1 + grow;
    if (ox0 >= ox1 || oy0 >= oy1 || ox0 >= a.w || oy0 >= a.h || ox1 <= 0 || oy1 <= 0) return;   // nothing of the box is in the frame

    // the label: name, " #id", " NN%"
    unsigned char* txt = reinterpret_cast<unsigned char*>(a.recs + slot * DRAW_REC + R_TEXT);
    int len = 0;
    auto put = [&](int c) { if (len < DRAW_TEXT) txt[len++] = (unsigned char)c; };
    if (a.labels) {
        if (named) {
            const unsigned char* nm = a.names + (size_t)ci * a.name_width;
            for (int q = 0; q < a.name_width && nm[q]; ++q) put(nm[q] < 0x20 || nm[q] > 0x7E ? '?' : nm[q]);
        }
        if (a.ids && id > 0) {
            if (len) put(' ');
            put('#');
            bool started = false;
            for (int d = 1000000000; d > 0; d /= 10) {
                const int q = id / d % 10;
                if (q || started || d == 1) { put('0' + q); started = true; }
            }
        }
        if (a.scores) {
            const float v = floorf(score * 100.f + 0.5f);
            const int pct = !(v >= 0.f) ? 0 : v > 100.f ? 100 : (int)v;
            if (len) put(' ');
            if (pct == 100) put('1');
            put('0' + pct / 10 % 10);
            put('0' + pct % 10);
            put('%');
        }
    }
    int px0 = 0, py0 = 0, px1 = 0, py1 = 0;
    int bx0 = ox0, by0 = oy0, bx1 = ox1, by1 = oy1;
    if (len) {
        const int pw = 6 * a.scale * len, ph = 8 * a.scale;
        px0 = ox0;
        if (px0 + pw > a.w) px0 = max(0, a.w - pw);
        py0 = oy0 - ph;
        if (py0 < 0) py0 = oy0;
        px1 = px0 + pw;
        py1 = py0 + ph;
        bx0 = min(bx0, px0); by0 = min(by0, py0); bx1 = max(bx1, px1); by1 = max(by1, py1);
    }
    rec4[0] = make_int4(ox0, oy0, ox1, oy1);
    rec4[1] = make_int4(x0 + shrink, y0 + shrink, x1 - shrink, y1 - shrink);
    rec4[2] = make_int4(px0, py0, px1, py1);
    rec4[3] = make_int4(colour, a.line_alpha | a.fill_alpha << 8, len | a.scale << 8, 0);
    a.bounds[slot] = make_int4(max(bx0, 0), max(by0, 0), min(bx1, a.w), min(by1, a.h));
}

// out = (src (255 - a) + colour a + 127) / 255 per channel; pixels are r | g << 8 | b << 16
__device__ __forceinline__ unsigned draw_blend(unsigned src, unsigned colour, unsigned alpha) {
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 24; c += 8) out |= (((src >> c) & 255u) * (255u - alpha) + ((colour >> c) & 255u) * alpha + 127u) / 255u << c;
    return out;
}

// one command over the four pixels (x .. x + 3, y) of a run; rec: words 0 .. 15 of the record in registers, text: its words 16 .. 23 in LDS
__device__ __forceinline__ void draw_apply(unsigned (&px)[4], int x, int y, const int (&rec)[R_TEXT], const int* text, const unsigned char* font) {
    const int colour = rec[R_COLOUR], alpha = rec[R_ALPHA], tl = rec[R_TEXT_LEN];
    if (y >= rec[R_OUTER + 1] && y < rec[R_OUTER + 3]) {
        const bool in_rows = y >= rec[R_INNER + 1] && y < rec[R_INNER + 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = x + i;
            if (xx >= rec[R_OUTER] && xx < rec[R_OUTER + 2]) {
                const bool inner = in_rows && xx >= rec[R_INNER] && xx < rec[R_INNER + 2];
                px[i] = draw_blend(px[i], colour, inner ? (alpha >> 8) & 255 : alpha & 255);
            }
        }
    }
    if ((tl & 255) && y >= rec[R_PLATE + 1] && y < rec[R_PLATE + 3]) {
        const int s = tl >> 8, cv = (y - rec[R_PLATE + 1]) / s;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = x + i;
            if (xx >= rec[R_PLATE] && xx < rec[R_PLATE + 2]) {
                const int u = (xx - rec[R_PLATE]) / s, cell = u / 6, cu = u - cell * 6;
                const int ch = (text[cell >> 2] >> ((cell & 3) * 8)) & 255;
                const bool on = cu < 5 && ((font[(ch - 0x20) * 8 + cv] >> (4 - cu)) & 1);
                px[i] = on ? 0xFFFFFFu : colour;
            }
        }
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void draw_load(unsigned (&px)[4], const unsigned char* p, int x, int w) {
    if constexpr (ALIGNED) {
        const unsigned* q = reinterpret_cast<const unsigned*>(p);
        const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
        px[0] = d0 & 0xFFFFFFu;
        px[1] = d0 >> 24 | (d1 & 0xFFFFu) << 8;
        px[2] = d1 >> 16 | (d2 & 0xFFu) << 16;
        px[3] = d2 >> 8;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < w) px[i] = p[3 * i] | p[3 * i + 1] << 8 | p[3 * i + 2] << 16;
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void draw_store(const unsigned (&px)[4], unsigned char* p, int x, int w) {
    if constexpr (ALIGNED) {
        unsigned* q = reinterpret_cast<unsigned*>(p);
        q[0] = px[0] | px[1] << 24;
        q[1] = px[1] >> 8 | px[2] << 16;
        q[2] = px[2] >> 16 | px[3] << 8;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < w) {
                p[3 * i] = (unsigned char)px[i];
                p[3 * i + 1] = (unsigned char)(px[i] >> 8);
                p[3 * i + 2] = (unsigned char)(px[i] >> 16);
            }
    }
}

// ALIGNED: both frame bases and 3 w are multiples of 4, so every run is three whole dwords; else byte by byte. Same bytes either way.
// in == out: in place; a tile that no command touches is then neither read nor written. Out of place the pixels are requested
// before the first bounding rectangles, and the rectangles of the next chunk before the hits of this one are composited, so a
// chunk costs one dependent trip to memory (the records of its hits), and the LDS list holds DRAW_BATCH records at a time.
template <bool ALIGNED>
__global__ __launch_bounds__(DRAW_THREADS) void draw_tiles_kernel(const unsigned char* in, unsigned char* out, int h, int w, int n,
                                                                  const int* nsel, const int4* bounds, const int* recs) {
    __shared__ unsigned short s_hit[DRAW_CHUNK];               // the chunk's hits, as indices into the chunk, in command order
    __shared__ int4 s_box[DRAW_BATCH];
    __shared__ __attribute__((aligned(16))) int s_rec[DRAW_BATCH * DRAW_REC];
    __shared__ __attribute__((aligned(16))) unsigned char s_font[96 * 8];
    __shared__ int s_wave[DRAW_THREADS / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.z;
    const int tx0 = blockIdx.x * DRAW_TW, ty0 = blockIdx.y * DRAW_TH, tx1 = min(tx0 + DRAW_TW, w), ty1 = min(ty0 + DRAW_TH, h);
    const int x = tx0 + 4 * (tid % DRAW_RUNS), yb = ty0 + tid / DRAW_RUNS;
    const size_t frame = (size_t)b * h * w * 3, cmd0 = (size_t)b * n;
    const bool copy = in != out;
    unsigned px[DRAW_GROUPS][4];
    bool loaded = false;

    auto load_all = [&]() {
#pragma unroll
        for (int g = 0; g < DRAW_GROUPS; ++g) {
            const int y = yb + g * DRAW_ROWS;
            if (x < w && y < h) draw_load<ALIGNED>(px[g], in + frame + ((size_t)y * w + x) * 3, x, w);
        }
    };

    const int cnt = nsel[b];
    const int4 none = make_int4(0, 0, 0, 0);
    int4 bb = tid < cnt ? bounds[cmd0 + tid] : none;
    if (copy) {
        load_all();
        loaded = true;
    }
    bool font_ready = false;
    for (int c0 = 0; c0 < cnt; c0 += DRAW_CHUNK) {
        const bool hit = bb.x < tx1 && bb.z > tx0 && bb.y < ty1 && bb.w > ty0;      // an empty rectangle (0, 0, 0, 0) meets no tile
        const int cn = c0 + DRAW_CHUNK + tid;
        bb = cn < cnt ? bounds[cmd0 + cn] : none;                                   // the next chunk's, in flight during this one
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int base = 0, nhit = 0;
#pragma unroll
        for (int v = 0; v < DRAW_THREADS / 64; ++v) {
            const int k = s_wave[v];
            if (v < wave) base += k;
            nhit += k;
        }
        if (hit) s_hit[base + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)tid;   // order-preserving
        if (nhit && !loaded) {                 // nhit is the same in every thread
            load_all();
            loaded = true;
        }
        if (nhit && !font_ready) {
            if (tid < 96 * 8 / 16) reinterpret_cast<int4*>(s_font)[tid] = reinterpret_cast<const int4*>(&dFont[0][0])[tid];
            font_ready = true;
        }
        __syncthreads();
        for (int k0 = 0; k0 < nhit; k0 += DRAW_BATCH) {
            const int m = min(DRAW_BATCH, nhit - k0);
            if (tid < m * (DRAW_REC / 4)) {    // six threads per record, one int4 each
                const int k = tid / (DRAW_REC / 4), q = tid % (DRAW_REC / 4);
                const size_t c = cmd0 + c0 + s_hit[k0 + k];
                reinterpret_cast<int4*>(s_rec)[tid] = reinterpret_cast<const int4*>(recs + c * DRAW_REC)[q];
            } else if (tid >= DRAW_THREADS - DRAW_BATCH && tid - (DRAW_THREADS - DRAW_BATCH) < m) {
                const int k = tid - (DRAW_THREADS - DRAW_BATCH);
                s_box[k] = bounds[cmd0 + c0 + s_hit[k0 + k]];
            }
            __syncthreads();
            if (x < w) {
                for (int k = 0; k < m; ++k) {  // hits outside, rows inside: a hit's rectangle and record are read from LDS once per thread
                    const int4 kb = s_box[k];
                    if (x + 4 <= kb.x || x >= kb.z || yb + (DRAW_GROUPS - 1) * DRAW_ROWS < kb.y || yb >= kb.w) continue;
                    int rec[R_TEXT];
#pragma unroll
                    for (int q = 0; q < R_TEXT / 4; ++q) {
                        const int4 v = reinterpret_cast<const int4*>(s_rec + k * DRAW_REC)[q];
                        rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
                    }
#pragma unroll
                    for (int g = 0; g < DRAW_GROUPS; ++g) {
                        const int y = yb + g * DRAW_ROWS;
                        if (y < h && y >= kb.y && y < kb.w) draw_apply(px[g], x, y, rec, s_rec + k * DRAW_REC + R_TEXT, s_font);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (!loaded) return;
#pragma unroll
    for (int g = 0; g < DRAW_GROUPS; ++g) {
        const int y = yb + g * DRAW_ROWS;
        if (x < w && y < h) draw_store<ALIGNED>(px[g], out + frame + ((size_t)y * w + x) * 3, x, w);
    }
}

static bool draw_dims_ok(int b, int n) { return b >= 1 && b <= DRAW_MAX_B && n >= 0 && n <= DRAW_MAX_N; }

}  // namespace yolo

using namespace yolo;

extern "C" {

void yolo_draw_tile(int* w, int* h) {
    if (w) *w = DRAW_TW;
    if (h) *h = DRAW_TH;
}

int yolo_draw_chunk(void) { return DRAW_CHUNK; }

int yolo_draw_text_capacity(void) { return DRAW_TEXT; }

void yolo_draw_font(unsigned char* rows) {
    if (rows) memcpy(rows, hFont, sizeof(hFont));
}

size_t yolo_draw_workspace_bytes(int b, int n) {
    if (!draw_dims_ok(b, n)) return 0;
    return draw_header_bytes(b) + (size_t)b * n * (sizeof(int4) + DRAW_REC * sizeof(int));
}

int yolo_draw_boxes(const uint8_t* frames_in, uint8_t* frames_out, int b, int h, int w, const float* boxes, int n, int center,
                    const int32_t* keep_idx, const int32_t* keep_count, const int32_t* ids, const int32_t* meta, const int32_t* canvas_hw,
                    const YoloDrawParams* p, const uint8_t* class_names, int n_classes, int name_width, const uint8_t* palette,
                    int n_colors, void* workspace, size_t workspace_bytes, void* stream) {
    if (!draw_dims_ok(b, n) || h < 1 || h > DRAW_MAX_HW || w < 1 || w > DRAW_MAX_HW)
        return fail(YOLO_ERR_UNSUPPORTED, "draw_boxes: b = %d (1 .. %d), h = %d, w = %d (1 .. %d) or n = %d (0 .. %d) outside the limits", b,
                    DRAW_MAX_B, h, w, DRAW_MAX_HW, n, DRAW_MAX_N);
    if (!frames_in || !frames_out || !p || !palette || (n > 0 && !boxes)) return fail(YOLO_ERR_ARG, "draw_boxes: null pointer");
    if (keep_idx && !keep_count) return fail(YOLO_ERR_ARG, "draw_boxes: keep_idx without keep_count");
    if (p->thickness < 1 || p->thickness > DRAW_MAX_T || p->font_scale < 1 || p->font_scale > DRAW_MAX_S)
        return fail(YOLO_ERR_ARG, "draw_boxes: thickness %d outside [1, %d] or font_scale %d outside [1, %d]", p->thickness, DRAW_MAX_T,
                    p->font_scale, DRAW_MAX_S);
    if (p->line_alpha < 0 || p->line_alpha > 255 || p->fill_alpha < 0 || p->fill_alpha > 255)
        return fail(YOLO_ERR_ARG, "draw_boxes: line_alpha %d or fill_alpha %d outside [0, 255]", p->line_alpha, p->fill_alpha);
    if (p->color_by_id && !ids) return fail(YOLO_ERR_ARG, "draw_boxes: colour by id without ids");
    if (n_colors < 1) return fail(YOLO_ERR_ARG, "draw_boxes: a palette of %d colours", n_colors);
    if (class_names && (n_classes < 1 || name_width < 1))
        return fail(YOLO_ERR_ARG, "draw_boxes: a name table of %d names of %d bytes", n_classes, name_width);
    if (meta && (!canvas_hw || canvas_hw[0] < 1 || canvas_hw[1] < 1)) return fail(YOLO_ERR_ARG, "draw_boxes: meta without a canvas size");
    const size_t need = yolo_draw_workspace_bytes(b, n);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)
        return fail(YOLO_ERR_UNSUPPORTED, "draw_boxes: workspace missing, not 16-byte aligned or %zu < %zu bytes", workspace_bytes, need);

    char* ws = static_cast<char*>(workspace);
    DrawArgs a;
    a.boxes = boxes; a.keep = keep_idx; a.count = keep_count; a.ids = ids; a.meta = meta;
    a.names = class_names; a.palette = palette;
    a.nsel = reinterpret_cast<int*>(ws);
    a.bounds = reinterpret_cast<int4*>(ws + draw_header_bytes(b));
    a.recs = reinterpret_cast<int*>(ws + draw_header_bytes(b) + (size_t)b * n * sizeof(int4));
    a.n = n; a.center = center != 0; a.h = h; a.w = w;
    a.canvas_h = meta ? canvas_hw[0] : 0; a.canvas_w = meta ? canvas_hw[1] : 0;
    a.thickness = p->thickness; a.scale = p->font_scale; a.line_alpha = p->line_alpha; a.fill_alpha = p->fill_alpha;
    a.labels = p->labels != 0; a.scores = p->scores != 0; a.by_id = p->color_by_id != 0;
    a.n_classes = n_classes; a.name_width = name_width; a.n_colors = n_colors;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(draw_commands_kernel, dim3(n ? ceil_div(n, DRAW_THREADS) : 1, b), dim3(DRAW_THREADS), 0, s, a);
    int rc = check_launch("draw commands");
    if (rc != YOLO_OK) return rc;
    const dim3 grid(ceil_div(w, DRAW_TW), ceil_div(h, DRAW_TH), b);
    const bool aligned = !(((uintptr_t)frames_in | (uintptr_t)frames_out) & 3) && w % 4 == 0;
    if (aligned)
        hipLaunchKernelGGL(draw_tiles_kernel<true>, grid, dim3(DRAW_THREADS), 0, s, frames_in, frames_out, h, w, n, a.nsel, a.bounds, a.recs);
    else
        hipLaunchKernelGGL(draw_tiles_kernel<false>, grid, dim3(DRAW_THREADS), 0, s, frames_in, frames_out, h, w, n, a.nsel, a.bounds, a.recs);
    return check_launch("draw tiles");
}

}  // extern "C"
