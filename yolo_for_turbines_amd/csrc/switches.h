// switches.h — the A/B environment switches of the library (INTEGRATION.md has the table): every one is read ONCE, when the
// library is loaded, by switches.hip, and the code asks this struct. A field keeps the sense of its variable's name: no_dma is
// true when YOLO_NO_DMA switches the DMA kernels off. yolo_switches_describe() prints what was read.
#pragma once

namespace yolo {

struct Switches {
    // on when the variable exists at all, whatever its value ("0" and "" included)
    bool no_dma;                    // YOLO_NO_DMA          16-bit: conv_patch_h16 instead of the LDS-DMA kernels
    bool no_s2_dma;                 // YOLO_NO_S2_DMA       16-bit 3x3 stride 2: conv_patch_h16 instead of the gathered-row GEMM
    bool no_s2g;                    // YOLO_NO_S2G          16-bit stride-2 input gradient: four tap-subset launches instead of one GEMM
    bool no_stagger;                // YOLO_NO_STAGGER      conv_f32_v2 / the patch-tiled 16-bit kernels: no stagger of the first wave of blocks
    bool no_winograd;               // YOLO_NO_WINOGRAD     fp32 3x3 stride 1: the direct kernels instead of F(4x4) / F(2x2)
    bool no_conv3_ws;               // YOLO_NO_CONV3_WS     16-bit 3x3 with <= 64 channels: not conv3_ws_h16
    bool no_conv1_rs;               // YOLO_NO_CONV1_RS     fp32 1x1: conv_igemm_f32 instead of conv1_rs_f32
    bool no_wgrad_dma;              // YOLO_NO_WGRAD_DMA    16-bit 3x3 stride-1 weight gradient: wgrad_h16 instead of wgrad3_dma_h16
    bool no_stem_wgrad;             // YOLO_NO_STEM_WGRAD   16-bit weight gradient of the first block: not wgrad_stem_h16
    bool stem_valu;                 // YOLO_STEM_VALU       16-bit first block: the vector kernel instead of stem_h16
    // on by default, off only when the value's first character is '0'
    bool f32_prio;                  // YOLO_F32_PRIO        conv_f32_v2: prologue / epilogue at raised wave priority
    bool dma_prio;                  // YOLO_DMA_PRIO        conv3_dma_h16 / conv1_dma_h16: the same
    // integers (atoi / atoll of the value)
    int wgrad_la;                   // YOLO_WGRAD_LA (3)              wgrad3_dma_h16: 5 = fragment look-ahead of 5, else 3
    int wgrad_prio;                 // YOLO_WGRAD_PRIO (0)            wgrad3_dma_h16: non-zero raises the later-dispatched waves' priority
    int stem_wgrad_blocks;          // YOLO_STEM_WGRAD_BLOCKS (256)   wgrad_stem_h16: cap of the grid
    long long wino2_maxpix;         // YOLO_WINO2_MAXPIX (256)        conv_wino2_f32 for maps of at most this many pixels (0: never)
};

extern const Switches g_switches;                                  // switches.hip
inline const Switches& switches() { return g_switches; }

}  // namespace yolo
