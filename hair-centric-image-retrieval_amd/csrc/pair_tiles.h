// pair_tiles.h — the logits tile of the contrastive losses (ntxent.hip, supcon.hip, ntxent_bank.hip).
//
// The all-pairs losses multiply the [N, D] row matrix by itself, the memory-bank loss multiplies its [N, D] query rows
// by the [K, D] bank, on the sim_core.h engine: workgroup (x = column tile of
// 128, y = row block of 128), a lane owns one logits ROW and receives 16 column scores per MFMA tile.  What is
// shared lives here: the stage / MFMA main loop, the online (max, sum of exp2) merge of two partials, and the
// fixed-tree mean of the per-row loss terms.  The epilogues (which column is a positive) stay in the two files.
#pragma once
#include "sim_core.h"

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

template <typename T>
using PairCfg = SimCfg<T, 2, 2, 2>;  // 128 column rows streamed x 128 logits rows resident

// acc[ct][rt] = the 4 x (32 x 32) products of this wave: columns c0 + wave_c*64 + ct*32 + acc_row(i, h) of the
// [ncols, D] matrix `cols`, row r0 + wave_r*64 + rt*32 + (lane & 31) of the [nrows, D] matrix `rows`.  Columns past
// ncols - 1 read column ncols - 1, rows past nrows - 1 read row nrows - 1.  Ends on a barrier: the stage buffers are
// free for the caller's in-workgroup merge.
template <typename T, bool GLDS>
__device__ __forceinline__ void pair_tile_products(f32x16 (&acc)[2][2], char* lds, const T* __restrict__ cols,
                                                   int64_t c0, int64_t ncols, const T* __restrict__ rows, int64_t r0,
                                                   int64_t nrows, int d, int tid, int lane, int wave_c, int wave_r) {
  using Cfg = PairCfg<T>;
  constexpr int EPS = SimElem<T>::kPerStage;
  const int nkc = (d + EPS - 1) / EPS;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[x][y][i] = 0.f;

  if constexpr (GLDS) {
    sim_stage_glds<T, Cfg>(lds, cols, c0, ncols - 1, rows, r0, nrows - 1, d, 0, tid);
    for (int kc = 0; kc < nkc; ++kc) {
      const int cur = kc & 1;
      sim_glds_retire_and_sync();
      if (kc + 1 < nkc)
        sim_stage_glds<T, Cfg>(lds + (cur ^ 1) * Cfg::STAGE_BYTES, cols, c0, ncols - 1, rows, r0, nrows - 1, d, kc + 1, tid);
      sim_stage_mfma<T, Cfg, 2>(acc, lds + cur * Cfg::STAGE_BYTES, wave_c, wave_r, lane);
    }
  } else {
    u32x4 regs[Cfg::NLOAD];
    sim_stage_load<T, Cfg>(regs, cols, c0, ncols - 1, rows, r0, nrows - 1, d, 0, tid);
    sim_stage_store<Cfg>(regs, lds, tid);
    __syncthreads();
    for (int kc = 0; kc < nkc; ++kc) {
      const int cur = kc & 1;
      if (kc + 1 < nkc) sim_stage_load<T, Cfg>(regs, cols, c0, ncols - 1, rows, r0, nrows - 1, d, kc + 1, tid);
      sim_stage_mfma<T, Cfg, 2>(acc, lds + cur * Cfg::STAGE_BYTES, wave_c, wave_r, lane);
      if (kc + 1 < nkc) sim_stage_store<Cfg>(regs, lds + (cur ^ 1) * Cfg::STAGE_BYTES, tid);
      __syncthreads();
    }
  }
  __syncthreads();
}

// The all-pairs form: columns and rows of one [n, D] matrix.
template <typename T, bool GLDS>
__device__ __forceinline__ void pair_tile_products(f32x16 (&acc)[2][2], char* lds, const T* __restrict__ zn,
                                                   int64_t c0, int64_t r0, int64_t n, int d, int tid, int lane,
                                                   int wave_c, int wave_r) {
  pair_tile_products<T, GLDS>(acc, lds, zn, c0, n, zn, r0, n, d, tid, lane, wave_c, wave_r);
}

// (m, l) <- (m, l) merged with the partial (mp, lp) of an online log-sum-exp in the log2 domain; an empty partial
// (lp == 0) leaves the pair as it is
__device__ __forceinline__ void pair_lse_merge(float& m, float& l, float mp, float lp) {
  if (lp > 0.f) {
    const float mn = fmaxf(m, mp);
    l = l * __builtin_amdgcn_exp2f(m - mn) + lp * __builtin_amdgcn_exp2f(mp - mn);
    m = mn;
  }
}

// one workgroup: *loss = (sum of the n row terms, fixed order and tree) / n
static __global__ __launch_bounds__(1024) void pair_mean_reduce(const float* __restrict__ row_loss, int64_t n,
                                                                float* __restrict__ loss) {
  __shared__ float red[1024];
  float local = 0.f;
  for (int64_t row = threadIdx.x; row < n; row += 1024) local += row_loss[row];  // fixed order
  red[threadIdx.x] = local;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = red[0] / (float)n;
}
