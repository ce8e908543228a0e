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
//   supcon_bwd_prep   : x^T as fp16 for hcir_gemm_f16, lse -> log2 domain (+inf for a row without positives, so
//                       that its softmax terms vanish), 2 / n_i.
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
  float inv = 1.0f;
  if (normalize) {
    float s = 0.f;
    for (int k = lane; k < d; k += 64) {
      const float x = (float)p[k];
      s = __builtin_fmaf(x, x, s);
    }
    s = wave_sum(s);
    inv = 1.0f / fmaxf(sqrtf(s), 1e-12f);
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

constexpr int kRedBytes = 128 * 4 * 4 * 4;  // [128 rows][4 src][m, l, ps, pc]; the column labels follow

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
    // ---- backward tile: the lane owns logits row `row`; its 16 registers per MFMA tile are 4 groups
    //      of 4 consecutive columns -> 8-byte fp16 stores into W[row][col..col+3]
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int64_t row = r0 + wave_r * 64 + rt * 32 + r;
      if (row >= a.n) continue;
      const int64_t yrow = a.y[row];
      const float lrow = a.lse2[row], tw = a.twon[row];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
          const int cl = wave_c * 64 + ct * 32 + 8 * grp + 4 * h;
          const int64_t col0 = c0 + cl;
          if (col0 >= a.n) continue;  // n is a multiple of 8: a group of 4 is inside or outside
          const f32x4 lcol = *reinterpret_cast<const f32x4*>(a.lse2 + col0);
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int64_t col = col0 + e;
            const float x = acc[ct][rt][4 * grp + e] * a.scale_log2;
            // lse2 = +inf for a row without positives: its exp2 is 0
            float w = __builtin_amdgcn_exp2f(x - lrow) + __builtin_amdgcn_exp2f(x - lcol[e]);
            w = (lab[cl + e] == yrow) ? w - tw : w;  // same class: n_col == n_row
            w = (col == row) ? 0.f : w;
            o[e] = (_Float16)w;
          }
          *reinterpret_cast<f16x4*>(a.wmat + row * a.n + col0) = o;
        }
      }
    }
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
      float tm = ninf;
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
        tm = fmaxf(tm, x[i]);
      }
      if (tm > ninf) {
        const float mn = fmaxf(m, tm);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += __builtin_amdgcn_exp2f(x[i] - mn);
        l = l * __builtin_amdgcn_exp2f(m - mn) + sum;
        m = mn;
      }
    }
    // the four (wave_c, lane-half) partials of a row meet in LDS: [128 rows][4 src][m, l, ps, pc]
    {
      const int rl = wave_r * 64 + rt * 32 + r, src = wave_c * 2 + h;
      const f32x4 part = {m, l, ps, (float)pc};
      *reinterpret_cast<f32x4*>(lds + (rl * 4 + src) * 16) = part;
    }
  }
  __syncthreads();
  if (tid < 128 && r0 + tid < a.n) {
    const f32x4* red = reinterpret_cast<const f32x4*>(lds) + tid * 4;
    float m = ninf, l = 0.f, ps = 0.f, pc = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // fixed order: deterministic
      const f32x4 part = red[s];
      pair_lse_merge(m, l, part[0], part[1]);
      ps += part[2];
      pc += part[3];
    }
    const int64_t o = (int64_t)blockIdx.x * a.n + r0 + tid;
    a.pm[o] = m;
    a.pl[o] = l;
    a.ps[o] = ps;
    a.pc[o] = pc;
  }
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
  float m = -__builtin_huge_valf(), l = 0.f, psum = 0.f;
  int32_t npos = 0;
  for (int p = 0; p < nparts; ++p) {
    const float mp = pm[(int64_t)p * n + row], lp = pl[(int64_t)p * n + row];
    psum += ps[(int64_t)p * n + row];
    npos += (int32_t)pc[(int64_t)p * n + row];
    if (lp > 0.f) {
      const float mn = fmaxf(m, mp);
      l = l * exp2f(m - mn) + lp * exp2f(mp - mn);
      m = mn;
    }
  }
  const float lse2 = m + log2f(l);  // log2 domain; N >= 2: every row has a live column
  if (row_lse) row_lse[row] = lse2 * kLn2;
  if (row_npos) row_npos[row] = npos;
  row_loss[row] = npos > 0 ? t_over_base * ((lse2 - psum / (float)npos) * kLn2) : 0.f;
}

// zt[k][i] = xn[i][k] as fp16 (the "weight" operand of g = W . X on hcir_gemm_f16); lse -> log2 domain, +inf for a
// row without positives; 2 / n_i
template <typename T>
__global__ void supcon_bwd_prep(const T* __restrict__ xn, const float* __restrict__ row_lse,
                                const int32_t* __restrict__ row_npos, int64_t n, int d, _Float16* __restrict__ zt,
                                float* __restrict__ lse2, float* __restrict__ twon) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    const int32_t np = row_npos[t];
    lse2[t] = np > 0 ? row_lse[t] * kLog2e : __builtin_huge_valf();
    twon[t] = np > 0 ? 2.0f / (float)np : 0.f;
  }
  if (t < n * d) {
    const int64_t i = t / d;
    const int k = (int)(t - i * d);
    zt[(int64_t)k * n + i] = (_Float16)(float)xn[t];
  }
}

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
  float ss = 0.f, gu = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float xv = (float)x[k];
    ss = __builtin_fmaf(xv, xv, ss);
    gu = __builtin_fmaf(g[row * d + k], (float)xn[row * d + k], gu);
  }
  ss = wave_sum(ss);
  gu = wave_sum(gu);
  const float rn = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  for (int k = lane; k < d; k += 64)
    dx[k] = (T)(coef * rn * (g[row * d + k] - gu * (float)xn[row * d + k]));
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

ScWorkspace sc_carve(void* base, int64_t n, int d, int dtype, bool bwd) {
  ScWorkspace w{};
  char* c = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = c ? c + off : nullptr;
    off += (bytes + 255) & ~size_t(255);
    return r;
  };
  const int64_t nct = hcir_cdiv(n, 128);
  w.xn = take((size_t)n * d * (dtype == HCIR_F32 ? 4 : 2));
  w.y = reinterpret_cast<int64_t*>(take((size_t)n * 8));
  if (!bwd) {
    w.pm = reinterpret_cast<float*>(take((size_t)nct * n * 4));
    w.pl = reinterpret_cast<float*>(take((size_t)nct * n * 4));
    w.ps = reinterpret_cast<float*>(take((size_t)nct * n * 4));
    w.pc = reinterpret_cast<float*>(take((size_t)nct * n * 4));
    w.row_loss = reinterpret_cast<float*>(take((size_t)n * 4));
  } else {
    w.wmat = reinterpret_cast<_Float16*>(take((size_t)n * n * 2));
    w.zt = reinterpret_cast<_Float16*>(take((size_t)n * d * 2));
    w.lse2 = reinterpret_cast<float*>(take((size_t)n * 4));
    w.twon = reinterpret_cast<float*>(take((size_t)n * 4));
    w.g = reinterpret_cast<float*>(take((size_t)n * d * 4));
  }
  w.bytes = off;
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
  if (d % SimElem<T>::kPerStage == 0)
    hipLaunchKernelGGL((supcon_tiles<T, true>), dim3(nct, nct), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((supcon_tiles<T, false>), dim3(nct, nct), dim3(256), 0, st, a);
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
  hipLaunchKernelGGL(supcon_bwd_prep<T>, dim3((unsigned)hcir_cdiv(n * d, 256)), dim3(256), 0, st,
                     static_cast<const T*>(w.xn), row_lse, row_npos, n, d, w.zt, w.lse2, w.twon);
  HCIR_LAUNCH_CHECK();
  ScArgs a{w.xn, w.y, nullptr, nullptr, nullptr, nullptr, n, d, inv_t * kLog2e, w.lse2, w.twon, w.wmat};
  if (d % SimElem<T>::kPerStage == 0)
    hipLaunchKernelGGL((supcon_tiles<T, true, true>), dim3(nct, nct), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((supcon_tiles<T, false, true>), dim3(nct, nct), dim3(256), 0, st, a);
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
  return inv_t == inv_t && inv_t != 0.f;
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
  if (dtype != HCIR_F32 && dtype != HCIR_F16 && dtype != HCIR_BF16) return HCIR_ERR_UNSUPPORTED;
  const ScWorkspace w = sc_carve(workspace, b * v, d, dtype, false);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HCIR_F32)
    return sc_run<float>(feat, labels, b, v, d, inv_t, t_over_base, normalize, loss, row_lse, row_npos, w, st);
  if (dtype == HCIR_F16)
    return sc_run<_Float16>(feat, labels, b, v, d, inv_t, t_over_base, normalize, loss, row_lse, row_npos, w, st);
  return sc_run<__bf16>(feat, labels, b, v, d, inv_t, t_over_base, normalize, loss, row_lse, row_npos, w, st);
}

int hcir_supcon_bwd(const void* feat, const int64_t* labels, int64_t b, int32_t v, int32_t d, int dtype, float inv_t,
                    float inv_base, int normalize, const float* row_lse, const int32_t* row_npos, float grad_out,
                    void* dfeat, void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!feat || !row_lse || !row_npos || !dfeat || !sc_shape_ok(b, v, d, inv_t) || ((b * v) & 7))
    return HCIR_ERR_INVALID;
  if (dtype != HCIR_F32 && dtype != HCIR_F16 && dtype != HCIR_BF16) return HCIR_ERR_UNSUPPORTED;
  const ScWorkspace w = sc_carve(workspace, b * v, d, dtype, true);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HCIR_F32)
    return sc_run_bwd<float>(feat, labels, b, v, d, inv_t, inv_base, normalize, row_lse, row_npos, grad_out, dfeat,
                             w, st);
  if (dtype == HCIR_F16)
    return sc_run_bwd<_Float16>(feat, labels, b, v, d, inv_t, inv_base, normalize, row_lse, row_npos, grad_out,
                                dfeat, w, st);
  return sc_run_bwd<__bf16>(feat, labels, b, v, d, inv_t, inv_base, normalize, row_lse, row_npos, grad_out, dfeat, w,
                            st);
}

}  // extern "C"
