// gemm_stage_addr.h — address arithmetic of the persistent GEMM kernels' stage issuer (gemm.hip, GemmStages<G>): the
// order in which a workgroup walks its tiles, and where the 16-B LDS-DMA pieces of a stage are read from.  Plain
// integer C++ that compiles for the host as well (tests/gemm_stage_addr_emul.cpp enumerates every thread and piece
// against a transcription of the per-piece formulas this replaced).
//
// A stage is TN W rows then TM activation rows of 128 B; thread `tid` of NT moves piece i = 0 .. NLOAD-1, which is
// row (tid >> 3) + (NT / 8) i of the stage and 16-B chunk (tid & 7) ^ ((row >> 1) & 7) of that row's 128 B (the XOR
// swizzle of the LDS image).  NT / 8 is a multiple of 16, so the swizzle term - and with it the chunk - is the same
// for every piece of a thread, and NT * NW == TN * 8, so pieces i < NW are W rows and the others activation rows.
// The source address of a piece therefore splits into
//   * a per-lane byte offset that no tile changes: gemm_lane_off(tid, ld) = (tid >> 3) ld 2 + chunk 16, one for W
//     (ld = ldw) and one for the activation rows (ld = lda), computed once per kernel, and
//   * a wave-uniform base: the operand's tile origin + issue_kc 128 + gemm_piece_base(j, ld), j = the piece's index
//     within its operand, which goes into the scalar base register of the transfer.
// The W rows never need a clamp (N % TN == 0 on every route that reaches these kernels).  The activation rows do on
// the last row of tiles only, where m0 + TM > M: there the offset of a piece is gemm_ragged_off(), rows clamped to
// `last` = M - 1 - m0 counted from the TILE's first row, on the base WITHOUT the piece term.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GEMM_ADDR_FN __host__ __device__ __forceinline__
#define GEMM_ADDR_FN_M __host__ __device__ __forceinline__
#else
#define GEMM_ADDR_FN static inline
#define GEMM_ADDR_FN_M inline
#endif

constexpr int kGemmNGroup = 3;      // tools/ab_gemm.py, batch 880: fc1 908 -> 890 us, qkv 574 -> 568 us against n
                                    // fastest over the whole N
constexpr int kGemmNGroupWide = 6;  // group size when it divides tiles_n (fc1: 12 n-tiles): the activation panels are
                                    // then fetched by two XCD sets instead of four (PMC: fc1 reads x5.3 -> see DESIGN);
                                    // time flat against 3 (profiles/r3_diag_ab_gemm_ngroup.txt), fabric bytes -20 %

// XCD-aware tile order: consecutive workgroup ids are dealt round-robin over the 8
// XCDs (MI355X_MICROARCH.md §Workgroup dispatch); remap so that one XCD walks a
// contiguous run of tiles and re-uses the W panel / A panel from its own L2.
GEMM_ADDR_FN int gemm_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, j = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// Origin (first W row n0, first activation row m0) of the ti-th tile of workgroup `wg` of `grid`.
template <bool N_GROUPED, int TN, int TM>
GEMM_ADDR_FN void gemm_tile_origin(int wg, int grid, int ti, int tiles_n, int tiles_m, int& n0, int64_t& m0) {
  const int t = gemm_xcd_remap(wg + ti * grid, tiles_n * tiles_m);
  if (N_GROUPED) {
    // n-grouped order: the W panels of one group of n-tiles stay in the XCD's L2 while every m-tile streams past
    // them (a W set wider than the 4 MB L2 - fc1: 12 panels, 4.7 MB - is otherwise re-fetched for every row of tiles)
    const int ngrp = (tiles_n % kGemmNGroupWide == 0 && tiles_n > kGemmNGroupWide) ? kGemmNGroupWide : kGemmNGroup;
    if (tiles_n % ngrp == 0 && tiles_n > ngrp) {
      const int per = ngrp * tiles_m;
      const int grp = t / per, rem = t - grp * per;
      n0 = (grp * ngrp + rem % ngrp) * TN;
      m0 = (int64_t)(rem / ngrp) * TM;
      return;
    }
  }
  n0 = (t % tiles_n) * TN;
  m0 = (int64_t)(t / tiles_n) * TM;
}

// 16-B chunk (swizzled) of every piece of thread tid
GEMM_ADDR_FN int gemm_lane_chunk(int tid) { return (tid & 7) ^ ((tid >> 4) & 7); }

// Tile-invariant per-lane byte offset of a thread's pieces of one operand with row pitch ld (elements of 2 B)
GEMM_ADDR_FN uint32_t gemm_lane_off(int tid, int64_t ld) {
  return (uint32_t)(((int64_t)(tid >> 3) * ld + gemm_lane_chunk(tid) * 8) * 2);
}

// Wave-uniform byte offset of piece j of an operand (j = i for W, i - NW for the activation rows): its NT / 8 rows
template <int NT>
GEMM_ADDR_FN int64_t gemm_piece_base(int j, int64_t ld) {
  return (int64_t)j * (NT / 8) * ld * 2;
}

// Ragged tile (last < TM - 1): per-lane byte offset of activation piece j from the tile's first row, the row clamped
// to `last` = M - 1 - m0.  The row is below TM, the 32-bit product wraps exactly as the 64-bit one truncates.
template <int NT>
GEMM_ADDR_FN uint32_t gemm_ragged_off(int tid, int j, int last, int64_t ld) {
  int mr = (tid >> 3) + (NT / 8) * j;
  mr = mr > last ? last : mr;
  return ((uint32_t)mr * (uint32_t)ld + (uint32_t)gemm_lane_chunk(tid) * 8u) * 2u;
}

// Last valid activation row of the tile at m0, counted from m0 and capped at TM - 1; below TM - 1: the tile is ragged
template <int TM>
GEMM_ADDR_FN int gemm_tile_last_row(int64_t m, int64_t m0) {
  const int64_t last = m - 1 - m0;
  return last < TM - 1 ? (int)last : TM - 1;
}

// Source of piece i of a stage: `base`, the wave-uniform bytes on top of (the operand's tile origin + issue_kc 128),
// and the lane's byte offset `off`.  RAGGED: the form a ragged tile takes for its activation pieces (tid, a_last and
// lda are read by that form only); woff / aoff: gemm_lane_off(tid, ldw / lda).
template <int NT, int NW, bool RAGGED>
GEMM_ADDR_FN void gemm_piece_source(int i, int tid, int a_last, int64_t lda, int64_t ldw, uint32_t woff, uint32_t aoff,
                                    int64_t& base, uint32_t& off) {
  if (i < NW) {
    base = gemm_piece_base<NT>(i, ldw);
    off = woff;
  } else if (RAGGED) {
    base = 0;
    off = gemm_ragged_off<NT>(tid, i - NW, a_last, lda);
  } else {
    base = gemm_piece_base<NT>(i - NW, lda);
    off = aoff;
  }
}

// Origins of the last three tiles the issuer reached, newest first, as (first W row, first activation row / TM).
// The issuer runs ahead of the MFMA loop: when the epilogue of tile ti is due it stands at tile ti + 1, or at ti + 2
// when a tile is ONE k-step (the stage issued in a tile's only step is already the next tile's, and the issuer moves
// on behind it).  push() is called every time the issuer moves on, past the last tile as well.
struct GemmTileOrigins {
  int n0[3] = {0, 0, 0};
  int mt[3] = {0, 0, 0};
  GEMM_ADDR_FN_M void shift() {
    n0[2] = n0[1];
    mt[2] = mt[1];
    n0[1] = n0[0];
    mt[1] = mt[0];
  }
  GEMM_ADDR_FN_M void set(int n0_, int mt_) {
    n0[0] = n0_;
    mt[0] = mt_;
  }
  // ahead = issue_ti - ti, 1 or 2
  GEMM_ADDR_FN_M void get(int ahead, int& n0_, int& mt_) const {
    n0_ = ahead == 2 ? n0[2] : n0[1];
    mt_ = ahead == 2 ? mt[2] : mt[1];
  }
};
