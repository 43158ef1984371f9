// wino4_planes.h — layout of the bf16 planes that the Winograd F(4x4) transform pass writes for conv_wino4s_f32.hip
// (YOLO_FLAG_WINO_SPLIT_BF16): every fp32 value of V4 and U4 as hi / mid / lo (split3.h).
//
//     [xi 36][chunk of 32 input channels][block of 64 rows][plane hi / mid / lo][row 64][64 bytes]
//
// A row is a tile (V planes) or an output channel (U planes); its 64 bytes are 32 channels as four 16-byte slots of 8, slot s of
// row r stored at s ^ g((r >> 2) & 3), g = (0, 2, 3, 1). The 12 KiB of one (xi, chunk, block) are what a workgroup of the GEMM
// stages for one operand: contiguous, and byte for byte its LDS image (twelve LDS-DMA pieces of 1 KiB).
// The fragment of v_mfma_f32_16x16x32_bf16 is row l & 15 of a 16-row block, channels 8 (l >> 4) .. + 7: one ds_read_b128 per lane.
// That read is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, each over 64 banks
// of 4 bytes = 256 bytes = four rows. Group 0 holds rows 0-3 and 12-15 with slot 0 and rows 4-11 with slot 1. The rows of a group
// that share r & 3 (the 64-byte quarter of the bank row) are one from each row quad q = r >> 2, and their stored slots are
// g(0), g(3), 1 ^ g(1), 1 ^ g(2) = 0, 1, 3, 2: all four, so the 16 lanes cover the 64 banks once. Group 1 has g(1), g(2), 1 ^ g(0),
// 1 ^ g(3) = 2, 3, 1, 0; groups 2 and 3 are groups 0 and 1 with every slot ^ 2. No bank conflict; plain q instead of g(q) (the
// swizzle of conv_split3_f32, whose fragments are 32 rows of one slot) would put rows 0-3 and 4-7 of group 0 on the same banks.
#pragma once

namespace yolo {

constexpr int W4S_PLANE = 4096;              // bytes of one plane of one (xi, chunk, block): 64 rows x 64 bytes
constexpr int W4S_PIECE = 3 * W4S_PLANE;     // hi, mid, lo

// the stored 16-byte slot of channels 8 s .. 8 s + 7 of row r
__host__ __device__ constexpr int w4s_slot(int r, int s) { return (s ^ (0x78 >> (2 * ((r >> 2) & 3)))) & 3; }

// byte offset, inside a plane, of channel c (0 .. 31) of row r (0 .. 63)
__host__ __device__ constexpr int w4s_row_off(int r, int c) { return r * 64 + w4s_slot(r, c >> 3) * 16 + (c & 7) * 2; }

// byte offset of (xi, input channel ci, row, plane) in a plane buffer of nkc chunks and nblk row blocks
__host__ __device__ constexpr size_t w4s_offset(int xi, int ci, int row, int plane, int nkc, int nblk) {
    return (((size_t)xi * nkc + (ci >> 5)) * nblk + (row >> 6)) * W4S_PIECE + (size_t)plane * W4S_PLANE + w4s_row_off(row & 63, ci & 31);
}

}  // namespace yolo
