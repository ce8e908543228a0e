// tr_layout.h — the LDS layout of the kernels whose contraction index is the SLOW index of both operands
// (gemm_tn.hip and the weight gradients of conv_bwd.hip and stem_train.hip): where the fill stores a tile and where
// the transposed reads find it.  Plain integer arithmetic, no device code, so that tests/test_tr_layout_host.py can
// check on the CPU that fill and read agree and that the reads are free of bank conflicts.
//
// A tile is staged as it is stored, [rows m][n] fp16 with ROWB bytes per row, and the MFMA fragments are read
// TRANSPOSED: ds_read_b64_tr_b16 hands lane i of a 16-lane group column i of a 4-row x 16-column block, i.e. 4
// consecutive m for one n.  Lane 16 g + 4 q + p supplies bytes 8 p .. 8 p + 7 of one 32-B chunk (16 columns) of row
// 8 g + q, and two such reads, rows + 0 (hf = 0) and + 4 (hf = 1), are one 16x16x32 operand over the 32 rows of
// substep ks (cdna_hip_programming.md T10).
//
// Banks: a half-wave (lanes 0..31: g = 0, 1) touches rows {0..3, 8..11} + 4 hf + 32 ks, the same 32-B chunk of each,
// and the LDS is 256 B wide per clock: eight groups of 32 B (cdna_hip_programming.md §2).  The 32-B chunks of a row
// are therefore XORed with a key that sends those eight rows to the eight groups:
//   ROWB >= 256: every row starts on group 0, so the key has three bits, (row & 3) | ((row >> 3) & 1) << 2;
//   ROWB == 128: the row's parity already picks the lower or upper four groups, and rows {0, 2, 8, 10} (+ 1) need the
//                two bits ((row >> 1) & 1) | ((row >> 3) & 1) << 1.
// The fill stores 16-B chunks; the two halves of a 32-B chunk stay together.  XOR is an involution, so tr_fill_off also
// answers "which logical chunk does physical slot ch16 hold" (gemm_tn.hip's LDS-DMA lands linearly and swizzles its
// source instead).
#pragma once

#if defined(__HIPCC__)
#define TR_HD __host__ __device__ __forceinline__
#else
#define TR_HD static inline
#endif

// XOR key of the 32-B chunks of row `row` of a tile with ROWB bytes per row
template <int ROWB>
TR_HD int tr_key(int row) {
  static_assert(ROWB == 128 || ROWB == 256 || ROWB == 512, "tr_layout: rows of 128, 256 or 512 bytes");
  return ROWB >= 256 ? ((row & 3) | (((row >> 3) & 1) << 2)) : (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
}

// byte offset at which the fill stores 16-B chunk `ch16` of row `row`
template <int ROWB>
TR_HD int tr_fill_off(int row, int ch16) {
  return row * ROWB + ((((ch16 >> 1) ^ tr_key<ROWB>(row)) << 5) | ((ch16 & 1) << 4));
}

// byte offset a lane hands to the transposed read: 32-B chunk (16 columns) `c32` of row `row`, 8-B piece `p4`
template <int ROWB>
TR_HD int tr_read_off(int row, int c32, int p4) {
  return row * ROWB + ((c32 ^ tr_key<ROWB>(row)) << 5) + 8 * p4;
}

// lane = 16 g16 + 4 q4 + p4, decomposed once per kernel: g16 is also the accumulator row group of the kernels'
// epilogues, and a row formula that shifted `lane` itself would be folded on its own, before it is inlined, into other
// (and, in conv_bwd.hip and stem_train.hip, a few more) address instructions than one that shares g16 with them.
struct TrLane {
  int g16, q4, p4;
};
TR_HD TrLane tr_lane(int lane) { return TrLane{lane >> 4, (lane >> 2) & 3, lane & 3}; }
// the row a lane supplies to read `hf` (0, 1) of 32-row substep `ks`; its 8-B piece of the chunk is p4
TR_HD int tr_lane_row(const TrLane& l, int ks, int hf) { return 32 * ks + 8 * l.g16 + 4 * hf + l.q4; }
