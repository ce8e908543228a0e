// Host build of csrc/gemm_stage_addr.h for tests/test_gemm_stage_addr_host.py: the source address of every LDS-DMA
// piece of a stage and the tile walk of the persistent GEMM kernels, against a transcription of the per-piece
// formulas the header replaced (GemmStages::set_sources / tile_origin / xcd_remap as they stood before it).
// With -DGEMM_ADDR_MAIN the same checks run as a stand-alone program (for a sanitizer build of plain host code).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../hair-centric-image-retrieval_amd/csrc/gemm_stage_addr.h"

namespace {

struct G256 {
  static constexpr int NT = 512, TN = 256, TM = 256, NLOAD = 8, NW = 4;
  static constexpr bool N_GROUPED = true;
};
struct GMid {
  static constexpr int NT = 256, TN = 128, TM = 192, NLOAD = 10, NW = 4;
  static constexpr bool N_GROUPED = false;
};

// ---- the reference: the formulas as they were ----
int ref_xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, j = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

template <class G>
void ref_tile_origin(int wg, int grid, int ti, int tiles_n, int tiles_m, int& n0, int64_t& m0) {
  const int t = ref_xcd_remap(wg + ti * grid, tiles_n * tiles_m);
  if (G::N_GROUPED) {
    const int ngrp = (tiles_n % 6 == 0 && tiles_n > 6) ? 6 : 3;
    if (tiles_n % ngrp == 0 && tiles_n > ngrp) {
      const int per = ngrp * tiles_m;
      const int grp = t / per, rem = t - grp * per;
      n0 = (grp * ngrp + rem % ngrp) * G::TN;
      m0 = (int64_t)(rem / ngrp) * G::TM;
      return;
    }
  }
  n0 = (t % tiles_n) * G::TN;
  m0 = (int64_t)(t / tiles_n) * G::TM;
}

// byte address of piece i of thread tid, from the operand's first element; *is_w: which operand
template <class G>
int64_t ref_source(int tid, int i, int64_t m, int n, int64_t lda, int64_t ldw, int n0, int64_t m0, int issue_kc,
                   bool* is_w) {
  const int64_t wbase = (int64_t)n0 * ldw * 2, abase = m0 * lda * 2;
  const int piece = tid + G::NT * i;
  const int row = piece >> 3, chunk = (piece & 7) ^ ((row >> 1) & 7);
  uint32_t soff;
  if (row < G::TN) {
    const int nr = n0 + row > n - 1 ? n - 1 - n0 : row;
    soff = (uint32_t)(((int64_t)nr * ldw + chunk * 8) * 2);
    *is_w = true;
    return wbase + issue_kc * 128 + soff;
  }
  int64_t mr = row - G::TN;
  mr = m0 + mr > m - 1 ? m - 1 - m0 : mr;
  soff = (uint32_t)((mr * lda + chunk * 8) * 2);
  *is_w = false;
  return abase + issue_kc * 128 + soff;
}

// ---- what the kernels do now ----
template <class G>
int64_t new_source(int tid, int i, int64_t m, int64_t lda, int64_t ldw, int n0, int64_t m0, int issue_kc) {
  const int64_t wbase = (int64_t)n0 * ldw * 2, abase = m0 * lda * 2;
  const uint32_t woff = gemm_lane_off(tid, ldw), aoff = gemm_lane_off(tid, lda);
  const int a_last = gemm_tile_last_row<G::TM>(m, m0);
  int64_t base;
  uint32_t off;
  if (a_last < G::TM - 1)
    gemm_piece_source<G::NT, G::NW, true>(i, tid, a_last, lda, ldw, woff, aoff, base, off);
  else
    gemm_piece_source<G::NT, G::NW, false>(i, tid, a_last, lda, ldw, woff, aoff, base, off);
  return (i < G::NW ? wbase : abase) + issue_kc * 128 + base + off;
}

template <class G>
int64_t check_sources(int64_t m, int n, int64_t lda, int64_t ldw, int n0, int64_t m0, int issue_kc, int64_t* bad) {
  int64_t nbad = 0;
  for (int tid = 0; tid < G::NT; ++tid)
    for (int i = 0; i < G::NLOAD; ++i) {
      bool is_w;
      const int64_t want = ref_source<G>(tid, i, m, n, lda, ldw, n0, m0, issue_kc, &is_w);
      const int64_t got = new_source<G>(tid, i, m, lda, ldw, n0, m0, issue_kc);
      bool ok = want == got && is_w == (i < G::NW) && got >= 0;
      // inside the operand: W rows below n, activation rows below m
      ok = ok && got + 16 <= (is_w ? ((int64_t)(n - 1) * ldw + (int64_t)(issue_kc + 1) * 64) * 2
                                   : ((m - 1) * lda + (int64_t)(issue_kc + 1) * 64) * 2);
      if (!ok && nbad++ == 0 && bad) {
        bad[0] = tid;
        bad[1] = i;
        bad[2] = want;
        bad[3] = got;
      }
    }
  return nbad;
}

// every tile of every workgroup: the header's origin against the reference, and every tile exactly once
template <class G>
int64_t check_tiles(int tiles_n, int tiles_m, int grid) {
  const int ntiles = tiles_n * tiles_m;
  std::vector<int> seen((size_t)ntiles, 0);
  int64_t nbad = 0;
  for (int wg = 0; wg < grid; ++wg) {
    const int my_tiles = wg < ntiles ? (ntiles - wg + grid - 1) / grid : 0;
    for (int ti = 0; ti < my_tiles; ++ti) {
      int n0, rn0;
      int64_t m0, rm0;
      gemm_tile_origin<G::N_GROUPED, G::TN, G::TM>(wg, grid, ti, tiles_n, tiles_m, n0, m0);
      ref_tile_origin<G>(wg, grid, ti, tiles_n, tiles_m, rn0, rm0);
      if (n0 != rn0 || m0 != rm0) ++nbad;
      if (n0 < 0 || n0 % G::TN || n0 / G::TN >= tiles_n || m0 < 0 || m0 % G::TM || m0 / G::TM >= tiles_m) {
        ++nbad;
        continue;
      }
      ++seen[(size_t)(m0 / G::TM) * tiles_n + n0 / G::TN];
    }
  }
  for (int t = 0; t < ntiles; ++t) nbad += seen[t] != 1;
  return nbad;
}

// The walk of one workgroup as the kernels run it: the first stage before the loop, one stage issued per step while
// one is left, the issuer moving on behind it, the epilogue of tile ti behind its last k-step.  Returns how many
// epilogues got an origin from GemmTileOrigins that is not their tile's.
template <class G>
int64_t check_origin_queue(int tiles_n, int tiles_m, int grid, int wg, int nkc) {
  const int ntiles = tiles_n * tiles_m;
  const int my_tiles = wg < ntiles ? (ntiles - wg + grid - 1) / grid : 0;
  const int nsteps = my_tiles * nkc;
  GemmTileOrigins org;
  int issue_kc = 0, issue_ti = 0;
  auto next_tile = [&]() {
    org.shift();
    if (issue_ti < my_tiles) {
      int n0;
      int64_t m0;
      gemm_tile_origin<G::N_GROUPED, G::TN, G::TM>(wg, grid, issue_ti, tiles_n, tiles_m, n0, m0);
      org.set(n0, (int)(m0 / G::TM));
    }
  };
  auto advance = [&]() {
    if (++issue_kc == nkc) {
      issue_kc = 0;
      ++issue_ti;
      next_tile();
    }
  };
  if (nsteps > 0) {
    next_tile();
    advance();
  }
  int64_t nbad = 0;
  int kc = 0, ti = 0;
  for (int step = 0; step < nsteps; ++step) {
    if (step + 1 < nsteps) advance();
    if (++kc == nkc) {
      int n0, mt, rn0;
      int64_t rm0;
      const int ahead = issue_ti - ti;
      org.get(ahead, n0, mt);
      ref_tile_origin<G>(wg, grid, ti, tiles_n, tiles_m, rn0, rm0);
      nbad += (ahead != 1 && ahead != 2) || n0 != rn0 || (int64_t)mt * G::TM != rm0;
      kc = 0;
      ++ti;
    }
  }
  return nbad + (ti != my_tiles);
}

}  // namespace

extern "C" {

// geo 0: the 256 x 256 kernel, 1: the 128 x 192 kernel.  Returns the number of (thread, piece) pairs whose source
// differs from the reference or leaves the operand; bad[4] = (tid, piece, want, got) of the first.
int64_t emul_check_sources(int geo, int64_t m, int n, int64_t lda, int64_t ldw, int n0, int64_t m0, int issue_kc,
                           int64_t* bad) {
  return geo == 0 ? check_sources<G256>(m, n, lda, ldw, n0, m0, issue_kc, bad)
                  : check_sources<GMid>(m, n, lda, ldw, n0, m0, issue_kc, bad);
}

int64_t emul_check_tiles(int geo, int tiles_n, int tiles_m, int grid) {
  return geo == 0 ? check_tiles<G256>(tiles_n, tiles_m, grid) : check_tiles<GMid>(tiles_n, tiles_m, grid);
}

int64_t emul_check_origin_queue(int geo, int tiles_n, int tiles_m, int grid, int wg, int nkc) {
  return geo == 0 ? check_origin_queue<G256>(tiles_n, tiles_m, grid, wg, nkc)
                  : check_origin_queue<GMid>(tiles_n, tiles_m, grid, wg, nkc);
}

int emul_tile_rows(int geo) { return geo == 0 ? G256::TM : GMid::TM; }
int emul_tile_cols(int geo) { return geo == 0 ? G256::TN : GMid::TN; }

}  // extern "C"

#ifdef GEMM_ADDR_MAIN
// the cases of tests/test_gemm_stage_addr_host.py, in one run
int main() {
  int64_t nbad = 0, ncase = 0;
  for (int geo = 0; geo < 2; ++geo) {
    const int tm = emul_tile_rows(geo), tn = emul_tile_cols(geo);
    const int lefts[] = {tm, 1, 63, 64, 65, tm - 1};
    for (int k : {64, 768})
      for (int pitched = 0; pitched < 2; ++pitched) {
        const int64_t lda = k + (pitched ? 8 : 0), ldw = k + (pitched ? 16 : 0);
        for (int64_t mtile : {(int64_t)0, (int64_t)3, ((int64_t)1 << 31) / lda / tm})
          for (int left : lefts)
            for (int kc : {0, k / 64 - 1})
              for (int n0 : {0, 2 * tn}) {
                const int64_t m0 = mtile * tm;
                nbad += emul_check_sources(geo, m0 + left, 3 * tn, lda, ldw, n0, m0, kc, nullptr);
                ++ncase;
              }
      }
    for (int tiles_n : {1, 3, 6, 9, 12})
      for (int tiles_m : {4, 5, 678})
        for (int grid : {7, 8, 255, 256}) {
          nbad += emul_check_tiles(geo, tiles_n, tiles_m, grid);
          for (int nkc : {1, 2, 3, 12})
            for (int wg : {0, 1, grid - 1}) nbad += emul_check_origin_queue(geo, tiles_n, tiles_m, grid, wg, nkc);
          ++ncase;
        }
  }
  printf("gemm_stage_addr: %lld cases, %lld mismatches\n", (long long)ncase, (long long)nbad);
  return nbad != 0;
}
#endif
