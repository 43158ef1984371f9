// h16.h — what the bf16 / fp16 convolution units share (fp32 accumulation; BASELINE configs 4-5: bf16 fine-tune forward,
// fp16 inference, which the reference reaches through torch.autocast, code/train.py:53).
//   conv_patch_h16.hip   register-staged patch kernel: every shape, and the tap subsets of the stride-2 input gradient
//   conv3_dma_h16.hip    3x3 stride 1, more than 64 output channels: every operand by LDS-DMA
//   conv1_dma_h16.hip    1x1 (and, with gathered rows, 3x3 stride 2 and the fused stride-2 input gradient) on the same machinery
//   conv3_ws_h16.hip     3x3 with <= 64 input and output channels: weights in registers, persistent workgroups
//   stem_h16.hip         the first block (3 -> 32 channels) on the matrix cores
//   pack_h16.hip         fp32 OIHW weights -> the 16-bit MFMA-fragment streams those kernels read
//   conv_h16.hip         host side: which kernel runs a convolution, and with which ConvHArgs
// All of them: activations NHWC 16-bit, v_mfma_f32_32x32x16_{bf16,f16}, accumulators and epilogue (folded BatchNorm scale /
// shift, LeakyReLU / Mish, residual) in fp32, one rounding to 16-bit at the store.
#pragma once
#include "common.h"

namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int H_PIX_BYTES = 80;          // 32 channels x 2 B + 16 B pad per patch pixel in LDS
constexpr int H_NI = 8;                  // staged pixels per 4-lane group -> patch <= 512 pixels
constexpr int H_PATCH_CAP = 64 * H_NI;
constexpr int D_NI = 4;                          // conv3_dma_h16: patch DMA rounds of 64 pixels
constexpr int D_PATCH_PIX = 64 * D_NI;           // 256 pixels

struct ConvHArgs {
    const unsigned short* x;
    const unsigned short* wf;
    const float* scale;
    const float* shift;
    const unsigned short* res;
    void* y;
    int* nan_flag;
    int H, W, Hin, Win, rows_total;      // output tiling view (1x1: H = 1, W = M); input dims
    int Cin, Cout;
    int x_ld, x_off, y_ld, y_off, r_ld, r_off;
    int TH, TW, PC, patch_cap;
    int bufmask, mtab_off;   // bufmask 1: two patch buffers; 0: one (stride-2 3x3, see launch_h). mtab_off: byte offset of mtab in LDS
    int tiles_w, tiles_n, nblocks;
    int KT, nchunks;
    int act, out_mode, flags, nc5;       // flags: YOLO_FLAG_* of the descriptor, and H_FLAG_VEC_EPILOGUE from the patch kernel's launchers
    int Ho, Wo;
    int first_wave, stagger;
    int prio;                            // conv3_dma_h16: prologue / epilogue at s_setprio 2 (A/B switch YOLO_DMA_PRIO=0)
    unsigned qperm;                      // conv3_dma_h16: nibble q = pixel quad of lane quad q within a 32-pixel m-tile
    int cls_ph, cls_pw;                  // MASK kernels (stride-2 input gradient): output pixel (2r+ph, 2c+pw)
    float* stats = nullptr;              // DMA kernels, training: per-wave BatchNorm partial sums [row][2][stats_ld] (null: ordinary epilogue)
    int stats_ld = 0;
    // backward statistics (input-gradient launches): the block that PRODUCED this convolution's input - its conv output z and
    // BatchNorm tables. Non-null: the epilogue (identity [+ residual]) also sums du = dx * act'(bn(z)) and du * (z - mean) per channel
    const unsigned short* bz = nullptr;
    const float* bmean = nullptr;
    const float* bscale = nullptr;
    const float* bshift = nullptr;
    int bz_ld = 0, bz_off = 0, bact = 0;
    // magic multipliers of the prologue's index divisions (a wave64 integer division is ~40 VALU instructions;
    // ~20 of them per thread were most of a 10k-cycle prologue in front of 9k cycles of matrix work)
    unsigned mg_H, mg_TW, mg_PC, mg_tn, mg_tw, mg_Hp;
};

// conv_patch_h16 only, a bit of ConvHArgs::flags above the public YOLO_FLAG_*: the epilogue may move 8 channels per 16-byte
// load / store. Decided on the host (patch_vec_epilogue), because it depends on the alignment of every address the epilogue
// forms and not on the channel count alone; without it the element-wise path runs.
constexpr int H_FLAG_VEC_EPILOGUE = 1 << 30;

// x / d for 0 <= x < 2^31 with mg = ceil(2^32 / d) (d >= 2) or 0 (d == 1): the estimate is q or q + 1, one fix-up
__device__ __forceinline__ int fdiv(int x, unsigned mg, int d) {
    if (!mg) return x;
    const unsigned q = __umulhi((unsigned)x, mg);
    return (int)(q * (unsigned)d > (unsigned)x ? q - 1 : q);       // q*d <= x + d < 2^32: no 64-bit multiply needed
}
inline unsigned magic_of(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }

template <typename T> struct HTraits;
template <> struct HTraits<__bf16> {
    typedef bf16x8 vec;
    static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float to_f32(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ unsigned short from_f32(float f) { __bf16 h = (__bf16)f; return *reinterpret_cast<unsigned short*>(&h); }
};
template <> struct HTraits<_Float16> {
    typedef f16x8 vec;
    static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float to_f32(unsigned short v) { _Float16 h = *reinterpret_cast<_Float16*>(&v); return (float)h; }
    static __device__ __forceinline__ unsigned short from_f32(float f) { _Float16 h = (_Float16)f; return *reinterpret_cast<unsigned short*>(&h); }
};

// two fp32 -> one dword of two 16-bit values (low half = a): ONE v_cvt_pk_{bf16,f16}_f32 instead of two conversions + shift + or
template <typename T> __device__ __forceinline__ unsigned pack2(float a, float b);
template <> __device__ __forceinline__ unsigned pack2<__bf16>(float a, float b) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const f2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
}
template <> __device__ __forceinline__ unsigned pack2<_Float16>(float a, float b) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const f2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h2));
}

// Halo pixels outside the image are read from a page of zeros instead of being masked. The library is built without
// relocatable device code, so every unit that reads the page carries its own copy of it.
static __device__ __attribute__((aligned(256))) unsigned int g_zero_page[1024 + 16];   // 4 KiB + 64 B of zeros: Cin <= 2048

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
__device__ __forceinline__ void glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// v of the lane that DPP control CTRL names (row_mirror, quad_perm ...): the reduce-scatter butterflies of the statistics epilogues
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// ---- tap subsets (stride-2 input gradient, see cls_mask below) ----------------------------------------
// MASK selects taps of the 3x3 window (bit kh*3+kw); the K loop runs over the set bits only. The ring slot
// must be compile-time, so three chunks are unrolled (R = running K-step index mod 3, see h_kstep_m).
constexpr int mask_count(int m) { int n = 0; for (int b = 0; b < 9; ++b) n += (m >> b) & 1; return n; }
constexpr int mask_nth(int m, int n) { for (int b = 0; b < 9; ++b) if ((m >> b) & 1) { if (n == 0) return b; --n; } return 0; }

// ---- stride-2 input gradient (transposed conv) as four stride-1 tap-subset convolutions over dz -------------
//   dx[n, 2r+ph, 2c+pw, ci] = sum_{dh <= ph, dw <= pw, co} dz[n, r+dh, c+dw, co] * W[co, ci, ph+1-2dh, pw+1-2dw]
// In the 3x3 window of the patch kernel (pad 1) the offset (dh, dw) is tap (1+dh, 1+dw): class (ph, pw) uses the
// taps {1, 1+ph} x {1, 1+pw} — 1, 2, 2 and 4 of them, 9 in total, so no matrix work is spent on structural zeros.
constexpr int cls_mask(int ph, int pw) {
    int m = 0;
    for (int dh = 0; dh <= ph; ++dh)
        for (int dw = 0; dw <= pw; ++dw) m |= 1 << ((1 + dh) * 3 + 1 + dw);
    return m;
}
inline size_t cls_frag_elems(int cin, int cout, int cls) {       // N = cin (dx channels), K = cout
    const int nt = mask_count(cls_mask(cls >> 1, cls & 1));
    return (size_t)(round_up(cin, 128) / 32) * (cout / 32) * nt * 1024;
}

// ------------------------------------------------------------------------------ host side
inline void fill_magics(ConvHArgs& a) {
    a.mg_H = magic_of(a.H); a.mg_TW = magic_of(a.TW); a.mg_PC = magic_of(a.PC);
    a.mg_tn = magic_of(a.tiles_n); a.mg_tw = magic_of(a.tiles_w); a.mg_Hp = magic_of(a.Hin + 2);
}

// what the launchers of the patch-tiled kernels (conv_patch_h16, conv3_dma_h16) share: the block grid, the prologue's magic
// multipliers and the stagger of the first wave of blocks
inline void tile_grid_h(ConvHArgs& a, int bn) {
    a.tiles_n = ceil_div(a.Cout, bn);
    const int tiles_r = ceil_div(a.rows_total, a.TH);
    a.nblocks = a.tiles_n * a.tiles_w * tiles_r;
    fill_magics(a);
    a.first_wave = 2 * 256;
    const long mfma_cycles = (long)a.KT * 8 * (bn / 64) / 2 * 32;      // one block's matrix cycles per wave
    a.stagger = !switches().no_stagger ? (int)((mfma_cycles + 1024) / 2048) : 0;   // s_sleep 32 = 2048 cycles
}

// ---- one launcher per kernel family; conv_h16.hip fills the ConvHArgs and picks one
// conv_patch_h16.hip (bn = 64 / 128 output channels per block)
void pick_tile_h(int Hin, int Hout, int Wout, int ks, int stride, int* th, int* tw, int* prmax, int patch_cap = H_PATCH_CAP);
int launch_h(ConvHArgs& a, int ks, int stride, int bn, int dtype, hipStream_t s);
int dgrad_s2_classes(ConvHArgs& a, const unsigned short* wf, int cin, int cout, int bn, int dtype, hipStream_t s);
// conv3_dma_h16.hip
int launch_dma(ConvHArgs& a, int dtype, hipStream_t s);
// conv1_dma_h16.hip (gath 0: 1x1; 1: 3x3 stride 2 forward; 2: fused stride-2 input gradient)
int launch_dma1(ConvHArgs& a, int gath, int dtype, hipStream_t s);
// conv3_ws_h16.hip (ws_stats_rows: partial-sum rows of a train-mode launch, 0 = too many tiles for this kernel)
bool ws_eligible(const yolo_conv_desc* d, const void* residual);
int ws_stats_rows(const yolo_conv_desc* d);
int conv_ws_launch(const yolo_conv_desc* d, const void* x, const void* wf, const float* scale, const float* shift, const void* residual,
                   void* y, int32_t* nan_flag, hipStream_t s, float* stats = nullptr, int stats_ld = 0);
// pack_h16.hip: is the fused stride-2 input gradient (conv1_dma_h16, gath 2) packed for this layer?
bool s2g_ok(int cout, int cin);

}  // namespace yolo
