// supcon.hip — fused supervised contrastive loss (SupConLoss), forward and backward, without materialising the
// logits in the forward.
//
// Semantics: HairPretraining/utils/losses.py:8-101 (contrast_mode 'all', labels or none), as called by the
// simclr_supcon step at HairPretraining/src/pretrain_engine.py:76,390:
//   features [B, V, D]; row r = v*B + i is view v of sample i (cat(unbind(features, 1))), N = V*B;
//   y_r = labels[r mod B] (labels NULL: r mod B);  x_r the row, or x_r / max(||x_r||, 1e-12) with `normalize`;
//   s_ij = x_i.x_j / T;  lse_i = log sum_{j != i} exp(s_ij);  positives m_ij = [y_i == y_j, j != i], n_i = sum_j m_ij;
//   loss = mean_i (T / T_base) [n_i > 0] (lse_i - sum_j m_ij s_ij / max(n_i, 1)).
// Backward: p_ij = exp(s_ij - lse_i), G_ij = [n_i > 0] (p_ij - m_ij / n_i), W = G + G^T (diagonal 0, |W_ij| <= 2),
//   g = W.x,  dL/dx_i = grad_out / (T_base N) g_i, through the normalisation's projection with `normalize`.
//
// Kernels
//   supcon_prep       : one wave per row: gather [B, V, D] into row order [N, D] in the compute dtype, normalised when
//                       asked; the row's 64-bit label into y[N].
//   supcon_tiles      : pair_tiles.h main loop (the one NT-Xent runs); a lane owns one logits ROW and folds its 16
//                       scores per MFMA tile into an online (max, sum-of-exp2) pair plus the sum and the count of its
//                       positive logits.  The row's label is loaded once per lane, the tile's 128 column labels are
//                       staged in LDS once per workgroup.  BWD = true: the same body writes W as fp16 [N, N].
//   supcon_rows       : one thread per row merges the per-column-tile partials in tile order (deterministic), writes
//                       row_lse, row_npos and the row's loss term.
//   pair_mean_reduce  : (pair_tiles.h) fixed-tree mean of the N loss terms.
//   pair_transpose_f16: (pair_tiles.h) x^T as fp16 for hcir_gemm_f16; with it ScRowScalars: lse -> log2 domain (+inf
//                       for a row without positives, so that its softmax terms vanish), 2 / n_i.
//   supcon_bwd_finish : scale (and projection), scatter back to [B, V, D] in the input dtype.
// No atomics anywhere: the results are deterministic from run to run.
#include "pair_tiles.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void supcon_prep(const T* __restrict__ feat, const int64_t* __restrict__ labels,
                                                   int64_t b, int v, int d, int normalize, T* __restrict__ xn,
                                                   int64_t* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= b * v) return;
  const int64_t view = row / b, i = row - view * b;
  const T* p = feat + (i * v + view) * d;
  if (normalize) {
    const float inv = pair_row_inv_norm(p, d, lane);
    for (int k = lane; k < d; k += 64) xn[row * d + k] = (T)((float)p[k] * inv);
  } else {
    for (int k = lane; k < d; k += 64) xn[row * d + k] = p[k];
  }
  if (lane == 0) y[row] = labels ? labels[i] : i;
}

struct ScArgs {
  const void* xn;
  const int64_t* y;  // [N] label of every row
  float* pm;         // [nct][N] running max (log2 domain) per column tile
  float* pl;         // [nct][N] sum of exp2
  float* ps;         // [nct][N] sum of the positive logits (log2 domain)
  float* pc;         // [nct][N] number of positives (an integer <= 128, exact in fp32)
  int64_t n;
  int d;
  float scale_log2;  // inv_t * log2(e)
  // backward (BWD = true): W[i][j] = a_i p_ij + a_j p_ji - m_ij 2 / n_i, diagonal 0, fp16 [N][N]
  const float* lse2;  // [N] row log-sum-exp in the log2 domain, +inf where n_i == 0
  const float* twon;  // [N] 2 / n_i, 0 where n_i == 0
  _Float16* wmat;
};

constexpr int kRedBytes = 128 * 4 * 4 * 4;  // pair_meet's [128 rows][4 src][m, l, ps, pc]; the column labels follow

template <typename T, bool GLDS, bool BWD = false>
__global__ __launch_bounds__(256, 2) void supcon_tiles(ScArgs a) {
  using Cfg = PairCfg<T>;
  static_assert(Cfg::LDS_BYTES >= kRedBytes + 128 * 8, "merge area + labels fit the stage buffers");
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_c = wave >> 1, wave_r = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const T* xn = static_cast<const T*>(a.xn);
  const int64_t c0 = (int64_t)blockIdx.x * 128, r0 = (int64_t)blockIdx.y * 128;

  // the tile's column labels: loaded before the main loop, parked in LDS after it (columns past N read row N - 1;
  // those columns are never live)
  int64_t ycol = 0;
  if (tid < 128) {
    const int64_t c = c0 + tid;
    ycol = a.y[c < a.n ? c : a.n - 1];
  }

  f32x16 acc[2][2];
  pair_tile_products<T, GLDS>(acc, lds, xn, c0, r0, a.n, a.d, tid, lane, wave_c, wave_r);

  const int64_t* lab = reinterpret_cast<const int64_t*>(lds + kRedBytes);
  if (tid < 128) reinterpret_cast<int64_t*>(lds + kRedBytes)[tid] = ycol;
  __syncthreads();

  const float ninf = -__builtin_huge_valf();
  if constexpr (BWD) {
    pair_write_image(acc, a.wmat, c0, a.n, r0, a.n, wave_c, wave_r, lane, [&](int64_t row) {
      const int64_t yrow = a.y[row];
      const float lrow = a.lse2[row], tw = a.twon[row];
      return [=](int64_t col0, f32x4 dot) {
        const f32x4 lcol = *reinterpret_cast<const f32x4*>(a.lse2 + col0);
        const int cl = (int)(col0 - c0);
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = dot[e] * a.scale_log2;
          // lse2 = +inf for a row without positives: its exp2 is 0
          w[e] = __builtin_amdgcn_exp2f(x - lrow) + __builtin_amdgcn_exp2f(x - lcol[e]);
          w[e] = (lab[cl + e] == yrow) ? w[e] - tw : w[e];  // same class: n_col == n_row
          w[e] = (col0 + e == row) ? 0.f : w[e];
        }
        return w;
      };
    });
    return;
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t row = r0 + wave_r * 64 + rt * 32 + r;
    const int64_t yrow = a.y[row < a.n ? row : a.n - 1];
    float m = ninf, l = 0.f, ps = 0.f;
    int pc = 0;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      float x[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int cl = wave_c * 64 + ct * 32 + acc_row(i, h);
        const int64_t col = c0 + cl;
        const float v = acc[ct][rt][i] * a.scale_log2;
        const bool live = col < a.n && col != row;
        const bool posm = live && lab[cl] == yrow;
        x[i] = live ? v : ninf;
        ps += posm ? v : 0.f;
        pc += posm ? 1 : 0;
      }
      pair_fold16(m, l, x);
    }
    pair_meet_put(lds, wave_c, wave_r, rt, lane, {m, l, ps, (float)pc});
  }
  pair_meet_store<4>(lds, tid, r0, a.n, 0.f, PairSum(), {a.pm, a.pl, a.ps, a.pc});
}

// one thread per logits row: merge the per-column-tile partials in tile order, write row_lse, row_npos and the
// row's loss term (T/T_base) [n > 0] (lse - P / n)
__global__ __launch_bounds__(256) void supcon_rows(const float* __restrict__ pm, const float* __restrict__ pl,
                                                   const float* __restrict__ ps, const float* __restrict__ pc,
                                                   int64_t n, int nparts, float t_over_base,
                                                   float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                   int32_t* __restrict__ row_npos) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  float m, l, psum = 0.f;
  int32_t npos = 0;
  pair_merge_tiles(m, l, pm, pl, n, nparts, row, [&](int64_t o) {
    psum += ps[o];
    npos += (int32_t)pc[o];
  });
  const float lse2 = m + log2f(l);  // log2 domain; N >= 2: every row has a live column
  if (row_lse) row_lse[row] = lse2 * kLn2;
  if (row_npos) row_npos[row] = npos;
  row_loss[row] = npos > 0 ? t_over_base * ((lse2 - psum / (float)npos) * kLn2) : 0.f;
}

// the backward tile's per-row scalars: lse -> log2 domain, +inf for a row without positives; 2 / n_i
struct ScRowScalars {
  const float* row_lse;
  const int32_t* row_npos;
  float *lse2, *twon;
  __device__ void operator()(int64_t i) const {
    const int32_t np = row_npos[i];
    lse2[i] = np > 0 ? row_lse[i] * kLog2e : __builtin_huge_valf();
    twon[i] = np > 0 ? 2.0f / (float)np : 0.f;
  }
};

// dx_i = coef * g_i, or with `normalize` coef * rn_i * (g_i - (g_i . u_i) u_i); one wave per row, scattered back to
// [B, V, D]; g = W.X (fp32), u = normalised row
template <typename T>
__global__ __launch_bounds__(256) void supcon_bwd_finish(const float* __restrict__ g, const T* __restrict__ xn,
                                                         const T* __restrict__ feat, int64_t b, int v, int d,
                                                         int normalize, float coef, T* __restrict__ dfeat) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= b * v) return;
  const int64_t view = row / b, i = row - view * b;
  const T* x = feat + (i * v + view) * d;
  T* dx = dfeat + (i * v + view) * d;
  if (!normalize) {
    for (int k = lane; k < d; k += 64) dx[k] = (T)(coef * g[row * d + k]);
    return;
  }
  const float rn = pair_row_inv_norm(x, d, lane);
  pair_project_row(dx, d, lane, coef * rn, [&](int k) { return g[row * d + k]; },
                   [&](int k) { return (float)xn[row * d + k]; });
}

struct ScWorkspace {
  void* xn;
  int64_t* y;
  float *pm, *pl, *ps, *pc, *row_loss;
  // backward only
  _Float16 *wmat, *zt;
  float *lse2, *twon, *g;
  size_t bytes;
};

ScWorkspace sc_carve(void* base, int64_t n64, int d, int dtype, bool bwd) {
  ScWorkspace w{};
  WsCarver c(base);
  const size_t n = (size_t)n64, nct = (size_t)hcir_cdiv(n64, 128);
  w.xn = c.take(n * d * hcir_dtype_bytes(dtype));
  w.y = c.take<int64_t>(n);
  if (!bwd) {
    w.pm = c.take<float>(nct * n);
    w.pl = c.take<float>(nct * n);
    w.ps = c.take<float>(nct * n);
    w.pc = c.take<float>(nct * n);
    w.row_loss = c.take<float>(n);
  } else {
    w.wmat = c.take<_Float16>(n * n);
    w.zt = c.take<_Float16>(n * d);
    w.lse2 = c.take<float>(n);
    w.twon = c.take<float>(n);
    w.g = c.take<float>(n * d);
  }
  w.bytes = c.off;
  return w;
}

template <typename T>
void sc_launch_prep(const void* feat, const int64_t* labels, int64_t b, int v, int d, int normalize,
                    const ScWorkspace& w, hipStream_t st) {
  hipLaunchKernelGGL(supcon_prep<T>, dim3((unsigned)hcir_cdiv(b * v, 4)), dim3(256), 0, st,
                     static_cast<const T*>(feat), labels, b, v, d, normalize, static_cast<T*>(w.xn), w.y);
}

template <typename T>
int sc_run(const void* feat, const int64_t* labels, int64_t b, int v, int d, float inv_t, float t_over_base,
           int normalize, float* loss, float* row_lse, int32_t* row_npos, const ScWorkspace& w, hipStream_t st) {
  const int64_t n = b * v;
  const int nct = (int)hcir_cdiv(n, 128);
  sc_launch_prep<T>(feat, labels, b, v, d, normalize, w, st);
  HCIR_LAUNCH_CHECK();
  ScArgs a{w.xn, w.y, w.pm, w.pl, w.ps, w.pc, n, d, inv_t * kLog2e, nullptr, nullptr, nullptr};
  pair_launch_tiles<T>(supcon_tiles<T, true>, supcon_tiles<T, false>, dim3(nct, nct), a, st);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(supcon_rows, dim3((unsigned)hcir_cdiv(n, 256)), dim3(256), 0, st, w.pm, w.pl, w.ps, w.pc, n,
                     nct, t_over_base, w.row_loss, row_lse, row_npos);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_mean_reduce, dim3(1), dim3(1024), 0, st, w.row_loss, n, loss);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

template <typename T>
int sc_run_bwd(const void* feat, const int64_t* labels, int64_t b, int v, int d, float inv_t, float inv_base,
               int normalize, const float* row_lse, const int32_t* row_npos, float grad_out, void* dfeat,
               const ScWorkspace& w, hipStream_t st) {
  const int64_t n = b * v;
  const int nct = (int)hcir_cdiv(n, 128);
  sc_launch_prep<T>(feat, labels, b, v, d, normalize, w, st);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL((pair_transpose_f16<T, ScRowScalars>), dim3((unsigned)hcir_cdiv(n * d, 256)), dim3(256), 0, st,
                     static_cast<const T*>(w.xn), n, d, w.zt, ScRowScalars{row_lse, row_npos, w.lse2, w.twon});
  HCIR_LAUNCH_CHECK();
  ScArgs a{w.xn, w.y, nullptr, nullptr, nullptr, nullptr, n, d, inv_t * kLog2e, w.lse2, w.twon, w.wmat};
  pair_launch_tiles<T>(supcon_tiles<T, true, true>, supcon_tiles<T, false, true>, dim3(nct, nct), a, st);
  HCIR_LAUNCH_CHECK();
  // g[N][D] = W[N][N] . X[N][D]  ==  hcir_gemm_f16(A = W, "weights" = X^T [D][N])
  const int rc = hcir_gemm_f16(w.wmat, n, w.zt, n, nullptr, nullptr, n, d, (int32_t)n, HCIR_EPI_BIAS_F32, w.g, d, st);
  if (rc != HCIR_OK) return rc;
  hipLaunchKernelGGL(supcon_bwd_finish<T>, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0, st, w.g,
                     static_cast<const T*>(w.xn), static_cast<const T*>(feat), b, v, d, normalize,
                     grad_out * inv_base / (float)n, static_cast<T*>(dfeat));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

bool sc_shape_ok(int64_t b, int32_t v, int32_t d, float inv_t) {
  if (b <= 0 || v <= 0 || d <= 0 || (d & 7) || b * v < 2 || b * v > 0x7fffffff) return false;
  return hcir_inv_t_ok(inv_t);
}

}  // namespace

extern "C" {

size_t hcir_supcon_workspace_bytes(int64_t b, int32_t v, int32_t d, int dtype, int backward) {
  if (b <= 0 || v <= 0 || d <= 0) return 0;
  return sc_carve(nullptr, b * v, d, dtype, backward != 0).bytes;
}

int hcir_supcon_fwd(const void* feat, const int64_t* labels, int64_t b, int32_t v, int32_t d, int dtype, float inv_t,
                    float t_over_base, int normalize, float* loss, float* row_lse, int32_t* row_npos,
                    void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!feat || !loss || !sc_shape_ok(b, v, d, inv_t)) return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const ScWorkspace w = sc_carve(workspace, b * v, d, dtype, false);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, sc_run, feat, labels, b, v, d, inv_t, t_over_base, normalize, loss, row_lse,
                             row_npos, w, st);
}

int hcir_supcon_bwd(const void* feat, const int64_t* labels, int64_t b, int32_t v, int32_t d, int dtype, float inv_t,
                    float inv_base, int normalize, const float* row_lse, const int32_t* row_npos, float grad_out,
                    void* dfeat, void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!feat || !row_lse || !row_npos || !dfeat || !sc_shape_ok(b, v, d, inv_t) || ((b * v) & 7))
    return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const ScWorkspace w = sc_carve(workspace, b * v, d, dtype, true);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, sc_run_bwd, feat, labels, b, v, d, inv_t, inv_base, normalize, row_lse, row_npos,
                             grad_out, dfeat, w, st);
}

}  // extern "C"
