// pair_tiles.h — the logits tile of the contrastive losses (ntxent.hip, supcon.hip, ntxent_bank.hip, msn.hip) and
// everything those four files would otherwise each state for themselves.
//
// The all-pairs losses (NT-Xent, SupCon) multiply the [N, D] row matrix by itself; the memory-bank loss multiplies its
// [N, D] query rows by the [K, D] bank, MSN its anchor or target rows by the [K, D] prototypes.  All run on the
// sim_core.h engine: workgroup (x = column tile of 128, y = row block of 128), a lane owns one logits ROW and receives
// 16 column scores per MFMA tile.
//
// Shared here, device side:
//   pair_tile_products   the stage / MFMA main loop
//   pair_fold16          16 masked scores of one MFMA tile into the lane's online (max, sum of exp2)
//   pair_meet_put/_store the four (wave_c, lane-half) partials of a row meet in LDS and leave as one per-tile partial
//   pair_write_image     the backward's fp16 image of the tile, four consecutive columns per store
//   pair_lse_merge       two online partials into one (hardware exp2 in the tile, libm exp2f in the row kernels)
//   pair_merge_tiles     a row's per-tile partials, in tile order
//   pair_row_inv_norm, pair_project_row   F.normalize of a row and its backward, one wave per row
//   pair_transpose_f16   the fp16 transpose that hcir_gemm_f16 takes as its "weight" operand
//   pair_mean_reduce     fixed-tree mean of the per-row loss terms
// Host side, in this device header because they need SimElem<T> and the tile geometry: pair_launch_tiles (LDS-DMA
// staging or not, by d) and pair_rows_cols_shape_ok.  The rest of the host glue (workspace carver, dtype dispatch,
// dtype and temperature checks) is the host-only host_util.h.
//
// What a loss keeps in its own file is what makes it that loss: which columns are live, which are positives and what
// is summed over them, the formula of one element of its backward image, its row kernel's last lines, its workspace.
#pragma once
#include "host_util.h"
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
// (lp == 0) leaves the pair as it is.
// Two flavours, because the two exponentials may round differently and every result is pinned to the bit: the tile
// kernels merge with the hardware's v_exp_f32 (LIBM = false), the one-thread-per-row kernels with libm's exp2f, which
// also scales denormal arguments (LIBM = true).  A call site never changes flavour.
// contract(off) is no requirement of the algorithm.  It pins what the four losses' own copies of this merge compiled to
// before they were folded into this one, two rounded products and an add (read in their ISA: v_pk_mul_f32, v_add_f32);
// left alone, the compiler fuses one product into the add or not depending on the code around the call, and the last
// bit of row_lse moves.  tools/loss_digest.py run on both sides of a change here is the check.
template <bool LIBM = false>
__device__ __forceinline__ void pair_lse_merge(float& m, float& l, float mp, float lp) {
#pragma clang fp contract(off)
  if (lp > 0.f) {
    const float mn = fmaxf(m, mp);
    if constexpr (LIBM)
      l = l * exp2f(m - mn) + lp * exp2f(mp - mn);
    else
      l = l * __builtin_amdgcn_exp2f(m - mn) + lp * __builtin_amdgcn_exp2f(mp - mn);
    m = mn;
  }
}

// The lane's 16 scores of one MFMA tile (log2 domain, -inf = masked out) folded into its online (m, l).
__device__ __forceinline__ void pair_fold16(float& m, float& l, const float (&x)[16]) {
  const float ninf = -__builtin_huge_valf();
  float tm = ninf;
#pragma unroll
  for (int i = 0; i < 16; ++i) tm = fmaxf(tm, x[i]);
  if (tm > ninf) {
    const float mn = fmaxf(m, tm);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += __builtin_amdgcn_exp2f(x[i] - mn);
    l = l * __builtin_amdgcn_exp2f(m - mn) + sum;
    m = mn;
  }
}

// Column of register i of column tile ct in this lane (h = lane >> 5).
__device__ __forceinline__ int64_t pair_col(int64_t c0, int wave_c, int ct, int i, int h) {
  return c0 + wave_c * 64 + ct * 32 + acc_row(i, h);
}

// The four (wave_c, lane-half) partials of a logits row meet in LDS as [128 rows][4 src] vectors of F fields (three
// fields take the room of four), each moved by one ds_write / ds_read.  Every lane puts the F values of its row tile
// rt, ...
template <int F>
using PairFields = float __attribute__((ext_vector_type(F)));
template <int F>
__device__ __forceinline__ void pair_meet_put(char* lds, int wave_c, int wave_r, int rt, int lane,
                                              const float (&v)[F]) {
  const int rl = wave_r * 64 + rt * 32 + (lane & 31), src = wave_c * 2 + (lane >> 5);
  PairFields<F> o;
#pragma unroll
  for (int f = 0; f < F; ++f) o[f] = v[f];
  reinterpret_cast<PairFields<F>*>(lds)[rl * 4 + src] = o;
}
// ... and after a barrier thread tid < 128 merges row r0 + tid's four in source order 0, 1, 2, 3 (deterministic) into
// part[f][blockIdx.x * n + row].  Fields 0 and 1 are an online (m, l); the others start at side0 and combine by
// `rule`.  LSE = false: fields 0 and 1 carry nothing, are not merged and not stored.
template <int F, bool LSE = true, typename Rule>
__device__ __forceinline__ void pair_meet_store(const char* lds, int tid, int64_t r0, int64_t n, float side0, Rule rule,
                                                float* const (&part)[F]) {
  __syncthreads();
  if (tid < 128 && r0 + tid < n) {
    const PairFields<F>* p = reinterpret_cast<const PairFields<F>*>(lds) + tid * 4;
    float v[F];
    v[0] = -__builtin_huge_valf();
    v[1] = 0.f;
#pragma unroll
    for (int f = 2; f < F; ++f) v[f] = side0;
    PairFields<F> q[4];  // all four reads in flight before the first merge waits for one
#pragma unroll
    for (int s = 0; s < 4; ++s) q[s] = p[s];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if constexpr (LSE) pair_lse_merge(v[0], v[1], q[s][0], q[s][1]);
#pragma unroll
      for (int f = 2; f < F; ++f) v[f] = rule(v[f], q[s][f]);
    }
    const int64_t o = (int64_t)blockIdx.x * n + r0 + tid;
#pragma unroll
    for (int f = LSE ? 0 : 2; f < F; ++f) part[f][o] = v[f];
  }
}
struct PairSum {
  __device__ float operator()(float a, float b) const { return a + b; }
};

// The backward's fp16 image [nrows][ncols] of this tile.  The lane owns logits row `row`; its 16 registers per MFMA
// tile are 4 groups of 4 consecutive columns -> 8-byte stores into img[row][col0 .. col0 + 3].  ncols is a multiple of
// 8, so a group of 4 is inside or outside.  row_fn(row) is the caller's per-row setup; what it returns is called once
// per group as (col0, dot), dot the raw products of columns col0 .. col0 + 3, and gives the four elements: whatever
// the caller loads per column, it loads once per group as one f32x4.
template <typename RowFn>
__device__ __forceinline__ void pair_write_image(const f32x16 (&acc)[2][2], _Float16* img, int64_t c0,
                                                 int64_t ncols, int64_t r0, int64_t nrows, int wave_c, int wave_r,
                                                 int lane, RowFn row_fn) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t row = r0 + wave_r * 64 + rt * 32 + r;
    if (row >= nrows) continue;
    const auto group = row_fn(row);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        const int64_t col0 = c0 + (wave_c * 64 + ct * 32 + 8 * grp + 4 * h);
        if (col0 >= ncols) continue;
        const f32x16& a = acc[ct][rt];
        const f32x4 w = group(col0, f32x4{a[4 * grp], a[4 * grp + 1], a[4 * grp + 2], a[4 * grp + 3]});
        f16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (_Float16)w[e];
        *reinterpret_cast<f16x4*>(img + row * ncols + col0) = o;
      }
    }
  }
}

// One thread per logits row: (m, l) <- the row's per-column-tile partials pm / pl [nparts][n] merged in tile order
// (deterministic); side(o) is called once per tile with the partial's offset for whatever else the loss sums.
template <typename Side>
__device__ __forceinline__ void pair_merge_tiles(float& m, float& l, const float* __restrict__ pm,
                                                 const float* __restrict__ pl, int64_t n, int nparts, int64_t row,
                                                 Side side) {
  m = -__builtin_huge_valf();
  l = 0.f;
  for (int p = 0; p < nparts; ++p) {
    const int64_t o = (int64_t)p * n + row;
    const float mp = pm[o], lp = pl[o];
    side(o);
    pair_lse_merge<true>(m, l, mp, lp);
  }
}

// inv[r] = 1 / max(||p[r]||, 1e-12) (F.normalize's eps) of R d-element rows read in one pass; the 64 lanes of one wave
// call it together.
template <int R, typename T>
__device__ __forceinline__ void pair_rows_inv_norm(const T* const (&p)[R], int d, int lane, float (&inv)[R]) {
  float s[R] = {};
  for (int k = lane; k < d; k += 64) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float v = (float)p[r][k];
      s[r] = __builtin_fmaf(v, v, s[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) inv[r] = 1.0f / fmaxf(sqrtf(wave_sum(s[r])), 1e-12f);
}
template <typename T>
__device__ __forceinline__ float pair_row_inv_norm(const T* p, int d, int lane) {
  float inv[1];
  pair_rows_inv_norm<1, T>({p}, d, lane, inv);
  return inv[0];
}

// The backward of u = x / ||x|| for one row, one wave: dx[k] = scale * (g(k) - (g.u) u(k)), scale = coef / ||x||.
template <typename T, typename G, typename U>
__device__ __forceinline__ void pair_project_row(T* __restrict__ dx, int d, int lane, float scale, G g, U u) {
  float gu = 0.f;
  for (int k = lane; k < d; k += 64) gu = __builtin_fmaf(g(k), u(k), gu);
  gu = wave_sum(gu);
  for (int k = lane; k < d; k += 64) dx[k] = (T)(scale * (g(k) - gu * u(k)));
}

// zt[k][i] = x[i][k] as fp16: the "weight" operand of g = W . X on hcir_gemm_f16.  The first n threads also run
// scalars(i), the per-row scalars the loss's backward tile reads (each loss's own).
template <typename T, typename RowScalars>
__global__ void pair_transpose_f16(const T* __restrict__ x, int64_t n, int d, _Float16* __restrict__ zt,
                                   RowScalars scalars) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) scalars(t);
  if (t < n * d) {
    const int64_t i = t / d;
    const int k = (int)(t - i * d);
    zt[(int64_t)k * n + i] = (_Float16)(float)x[t];
  }
}

// Launch a tile kernel on `grid`: its LDS-DMA instantiation where d is a whole number of stages, else the
// register-staged one.
template <typename T, typename Args>
void pair_launch_tiles(void (*glds)(Args), void (*staged)(Args), dim3 grid, const Args& a, hipStream_t st) {
  hipLaunchKernelGGL(a.d % SimElem<T>::kPerStage == 0 ? glds : staged, grid, dim3(256), 0, st, a);
}

// The two-matrix losses' shape rule: 128-row blocks ride on grid.y (<= 65535); the columns' pitch and the GEMM's K
// are 32-bit
static inline bool pair_rows_cols_shape_ok(int64_t n, int64_t k, int32_t d, float inv_t) {
  if (n <= 0 || k <= 0 || d <= 0 || (d & 7) || n > 65535 * (int64_t)128 || k > 0x7fffffff) return false;
  return hcir_inv_t_ok(inv_t);
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
