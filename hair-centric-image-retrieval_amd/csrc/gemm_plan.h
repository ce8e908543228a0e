// gemm_plan.h — host-side route decision of hcir_gemm_f16 and its fused forms (gemm.hip): which kernel a launch takes
// and, on the tail split, how many rows stay on the 256 x 256 kernel.  Plain C++, no device code, so that the
// arithmetic can be read (and asked for: hcir_gemm_route) without the kernels.
#pragma once
#include <stdint.h>

#include "../../include/hcir.h"

constexpr int GEMM_BIG_TN = 256, GEMM_BIG_TM = 256;   // G256 tile
constexpr int GEMM_MID_TN = 128, GEMM_MID_TM = 192;   // GMid tile
constexpr int GEMM_BIG_GRID = 256;                    // persistent: one workgroup per CU
constexpr int GEMM_MID_GRID = 512;                    // persistent: two workgroups per CU

struct GemmPlan {
  int route;     // hcir_gemm_route_kind
  int tn, tm;    // tiles of the route's (first) kernel: 128 x 128, 128 x 192 or 256 x 256
  int tm1;       // split: m-tiles of the whole rounds on the 256 x 256 kernel
  int64_t m1;    // rows on the 256 x 256 kernel (split: tm1 * 256; big: m; else 0)
};

static inline int64_t gemm_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Which kernel a launch takes, callee first: launch_gemm -> launch_gemm_big -> launch_big_tiles / launch_gemm_mid.
static inline bool gemm_takes_big(int64_t m, int n, int k) { return k % 64 == 0 && m >= 1024 && n % 256 == 0; }

// `dual`: hcir_gemm_f16_gelu_dual, which stays on the 256 x 256 kernel whatever the tile count.
static inline GemmPlan gemm_plan(int64_t m, int n, int k, bool dual) {
  GemmPlan p;
  p.tm1 = 0;
  p.m1 = 0;
  if (!gemm_takes_big(m, n, k)) {
    p.route = HCIR_GEMM_ROUTE_SMALL;
    p.tn = (int)gemm_cdiv(n, 128);
    p.tm = (int)gemm_cdiv(m, 128);
    return p;
  }
  const int tn = (int)gemm_cdiv(n, GEMM_BIG_TN), tm = (int)gemm_cdiv(m, GEMM_BIG_TM);
  if (!dual) {
    // Tail split: when the last round of 256 x 256 tiles would be less than half full (64 images: fc1 = 600 tiles = 2.34
    // rounds; ViT-L/14 at 128 images: 516 / 1548 / 2064 tiles = 2.02 / 6.05 / 8.06 rounds - a whole round for a sliver),
    // the m-tiles that fill whole rounds run on the 256 x 256 kernel and the remaining ROWS go to the 128 x 192 kernel
    // as a second launch (pointers advanced to the row range; the per-row statistics keep the full matrix's slice pitch).
    const int ntiles = tn * tm;
    const int tm1 = (ntiles / GEMM_BIG_GRID) * GEMM_BIG_GRID / tn;  // m-tiles of the whole rounds
    const int tail_tiles = ntiles - tm1 * tn;
    const int64_t m1 = (int64_t)tm1 * GEMM_BIG_TM;
    if (ntiles > GEMM_BIG_GRID && tm1 > 0 && tm1 < tm && tail_tiles < 128 && n % GEMM_MID_TN == 0 &&
        (n / GEMM_MID_TN) * gemm_cdiv(m - m1, GEMM_MID_TM) <= GEMM_MID_GRID) {
      p.route = HCIR_GEMM_ROUTE_SPLIT;
      p.tn = tn;
      p.tm = tm1;
      p.tm1 = tm1;
      p.m1 = m1;
      return p;
    }
    // Small M: a launch whose 256 x 256 tiles fill less than 0.7 of ONE round of the 256 CUs (64 images: proj / fc2
    // give 150 tiles) runs on the 128 x 192 kernel at two workgroups per CU instead - 2.7 x the tiles, every CU busy;
    // its results are bit-identical (same k order).  12 % slower per flop on full rounds, which is why only these take it.
    if (tn * tm * 10 < GEMM_BIG_GRID * 7 && n % GEMM_MID_TN == 0 &&
        (n / GEMM_MID_TN) * gemm_cdiv(m, GEMM_MID_TM) <= GEMM_MID_GRID) {
      p.route = HCIR_GEMM_ROUTE_MID;
      p.tn = n / GEMM_MID_TN;
      p.tm = (int)gemm_cdiv(m, GEMM_MID_TM);
      return p;
    }
  }
  p.route = HCIR_GEMM_ROUTE_BIG;
  p.tn = tn;
  p.tm = tm;
  p.m1 = m;
  return p;
}
