// LDS image of a streamed [rows][128 x bf16] attention tile, and the lane
// addressing of everything that touches it. Pure integer constexpr
// functions in BYTES from the tile's 16-byte-aligned base; they compile for
// the host (tests/test_attn_lds_image.py runs the bank model over them) and
// for the device (attention.hip, debug_kernels.hip).
//
// One copy of the tile serves the two reads of the 32x32x16 operand:
//  * the ROW read (ds_read_b128): lane 32*hi + l32 takes the 16-byte chunk
//    2s + hi (d = 16s + 8hi .. +7) of row 32t + l32, k-step s = 0..7;
//  * the TRANSPOSED read (ds_read_b64_tr_b16): lane 32*hi + l32 receives
//    rows 16ks + 8hi + 4u + (0..3) at d column 32n + l32, u = 0, 1 the two
//    reads of one fragment. Per 16-lane group the hardware gathers a 4-row
//    x 16-column block: lane 4q + p of the group supplies the address of
//    row q, columns 4p .. 4p+3, i.e. off(r0 + q, c0 + (p >> 1)) + 8*(p & 1).
//
// off(row, ch) is the byte offset of 16-byte chunk ch (0..15) of a row.
// Every address goes through it: the XOR can swap the two chunks of a
// row's 32 bytes, so "base + 8p + stride*q" reads wrong rows on some lanes
// with no fault.
//
// Image A (8-row x 32-column subtiles of 512 B) is what the train kernels
// use. Both reads and the staging writes below are what the bank rules
// make of it (LDS-array cycles relative to conflict-free, 64-row tile):
//                  row read  transposed read  stage16  stage_walk
//   panel [8][R][16]   2x          2x            4x        2x
//   image A            1x          1x            2x        2x
//   image B            1x          1x            1x        2x
// A needs 2 lane bases for the 8 row reads and 2 for the 16 transposed
// reads of a 64-row tile, everything else being instruction immediates
// (B needs 8 and 8): dK/dV sits at the 256-VGPR limit.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDSIMG_FN __host__ __device__ constexpr
#else
#define LDSIMG_FN constexpr
#endif

namespace lds_img {

// ---- the images ----
LDSIMG_FN int off_a(int row, int ch) {
  return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7)
         + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

LDSIMG_FN int off_b(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// the 16-wide panel layout of append.hip and the layout probe
// (stage_panel / frag8_panel / tr_load_bfrags in attention.hip), here so
// the bank model can be checked against its measured conflict figures
LDSIMG_FN int off_panel(int rows, int row, int ch) {
  return (ch >> 1) * rows * 32 + row * 32 + (ch & 1) * 16;
}

// ---- image A, row read ----
// address = row_base_a(lane, s & 1) + row_imm_a(t, s) == off_a(32t + l32,
// 2s + hi): the chunk's low two bits meet the XOR key (l32 >> 2) & 3, a
// lane constant, so the parity of s picks one of two lane bases.
LDSIMG_FN int row_base_a(int lane, int s_odd) {
  return off_a(lane & 31, 2 * s_odd + (lane >> 5));
}
LDSIMG_FN int row_imm_a(int t, int s) { return 8192 * t + 512 * (s >> 1); }
LDSIMG_FN int row_addr_a(int lane, int t, int s) {
  return row_base_a(lane, s & 1) + row_imm_a(t, s);
}

// ---- image A, transposed read ----
// address = tr_base_a(lane, u) + tr_imm_a(ks, n) == off_a(16ks + 8hi + 4u
// + q, 4n + 2g + (p >> 1)) + 8*(p & 1) with q = (lane >> 2) & 3, p = lane
// & 3, g = (lane >> 4) & 1: rows 16ks + 8hi .. +7 are one 8-row subtile
// group, so ks and n only move whole 4096- and 512-byte steps.
LDSIMG_FN int tr_base_a(int lane, int u) {
  return off_a(8 * (lane >> 5) + 4 * u + ((lane >> 2) & 3),
               2 * ((lane >> 4) & 1) + ((lane & 3) >> 1))
         + 8 * (lane & 1);
}
LDSIMG_FN int tr_imm_a(int ks, int n) { return 4096 * ks + 512 * n; }
LDSIMG_FN int tr_addr_a(int lane, int ks, int n, int u) {
  return tr_base_a(lane, u) + tr_imm_a(ks, n);
}

// ---- staging writes (ds_write_b128 of one 16-byte chunk) ----
// 16 threads per row (forward, dQ): slot idx = 0 .. rows*16 - 1 is chunk
// idx % 16 of row idx / 16
LDSIMG_FN int stage16_row(int idx) { return idx >> 4; }
LDSIMG_FN int stage16_ch(int idx) { return idx & 15; }
LDSIMG_FN int stage16_addr_a(int idx) {
  return off_a(stage16_row(idx), stage16_ch(idx));
}
// lanes walk rows (dK/dV, the probe): slot idx is chunk idx / rows of row
// idx % rows
LDSIMG_FN int stage_walk_row(int rows, int idx) { return idx % rows; }
LDSIMG_FN int stage_walk_ch(int rows, int idx) { return idx / rows; }
LDSIMG_FN int stage_walk_addr_a(int rows, int idx) {
  return off_a(stage_walk_row(rows, idx), stage_walk_ch(rows, idx));
}

}  // namespace lds_img
