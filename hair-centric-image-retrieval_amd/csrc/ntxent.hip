// ntxent.hip — fused NT-Xent forward: normalise -> 2B x 2B cosine / T -> masked row
// log-sum-exp -> mean cross-entropy, without materialising the logits.
//
// Semantics: lightly.loss.NTXentLoss(temperature) as called at
// HP/src/pretrain_engine.py:93,725 (== experiments/DualViewHair/src/losses/ntxent_loss.py:30-57):
//   z = [normalize(z0); normalize(z1)], logits = z z^T / T, diagonal removed,
//   positive of row i is (i + B) mod 2B, loss = mean_i(logsumexp_j logits[i][j] - logits[i][pos]).
//
// Kernels
//   ntxent_prep   : one wave per row: x / max(||x||, 1e-12) (F.normalize eps) into the
//                   workspace, in the compute dtype.
//   ntxent_tiles  : sim_core.h tile engine; workgroup (x = column tile of 128, y = row block of
//                   128); a lane owns one logits ROW and folds its 16 scores per MFMA tile
//                   into an online (max, sum-of-exp2) pair; diagonal skipped, positive captured.
//                   BWD = true: the same products, written as W in fp16 [2B, 2B].
//   ntxent_rows   : one thread per row merges the per-column-tile partials in tile order
//                   (deterministic), writes row_lse and the row's loss term.
//   pair_mean_reduce (pair_tiles.h): one workgroup sums the 2B loss terms in a fixed tree -> mean loss.
// The main loop, the fold, the meeting of a row's partials, the image writer, the merges and the row helpers are
// pair_tiles.h, shared with supcon.hip, ntxent_bank.hip and msn.hip; here is what is NT-Xent's own.
#include "pair_tiles.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void ntxent_prep(const T* __restrict__ z0, const T* __restrict__ z1,
                                                   int64_t b, int d, T* __restrict__ zn) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * b) return;
  const T* p = row < b ? z0 + row * d : z1 + (row - b) * d;
  const float inv = pair_row_inv_norm(p, d, lane);
  for (int k = lane; k < d; k += 64) zn[row * d + k] = (T)((float)p[k] * inv);
}

struct NtArgs {
  const void* zn;
  float* pm;   // [nct][2B] running max (log2 domain) per column tile
  float* pl;   // [nct][2B] sum of exp2
  float* pp;   // [nct][2B] positive logit (log2 domain) or -inf
  int64_t n;   // 2B
  int64_t b;
  int d;
  float scale_log2;  // inv_t * log2(e)
  // backward (BWD = true): W[i][j] = p_ij + p_ji - 2*[j == pos(i)], diagonal 0, fp16 [2B][2B]
  const float* lse2;  // [2B] row log-sum-exp in the log2 domain
  _Float16* wmat;
};

template <typename T, bool GLDS, bool BWD = false>
__global__ __launch_bounds__(256, 2) void ntxent_tiles(NtArgs a) {
  using Cfg = PairCfg<T>;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_c = wave >> 1, wave_r = wave & 1;
  const int h = lane >> 5;
  const T* zn = static_cast<const T*>(a.zn);
  const int64_t c0 = (int64_t)blockIdx.x * 128, r0 = (int64_t)blockIdx.y * 128;

  f32x16 acc[2][2];
  pair_tile_products<T, GLDS>(acc, lds, zn, c0, r0, a.n, a.d, tid, lane, wave_c, wave_r);

  const float ninf = -__builtin_huge_valf();
  if constexpr (BWD) {
    pair_write_image(acc, a.wmat, c0, a.n, r0, a.n, wave_c, wave_r, lane, [&](int64_t row) {
      const int64_t pos = row < a.b ? row + a.b : row - a.b;
      const float lrow = a.lse2[row];
      return [=](int64_t col0, f32x4 dot) {
        const f32x4 lcol = *reinterpret_cast<const f32x4*>(a.lse2 + col0);
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t col = col0 + e;
          const float x = dot[e] * a.scale_log2;
          w[e] = __builtin_amdgcn_exp2f(x - lrow) + __builtin_amdgcn_exp2f(x - lcol[e]);
          w[e] = (col == pos) ? w[e] - 2.0f : w[e];
          w[e] = (col == row) ? 0.f : w[e];
        }
        return w;
      };
    });
    return;
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t row = r0 + wave_r * 64 + rt * 32 + (lane & 31);
    const int64_t pos = row < a.b ? row + a.b : row - a.b;
    float m = ninf, l = 0.f, pv = ninf;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      float x[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t col = pair_col(c0, wave_c, ct, i, h);
        const float v = acc[ct][rt][i] * a.scale_log2;
        const bool live = col < a.n && col != row;
        x[i] = live ? v : ninf;
        pv = (col == pos) ? v : pv;
      }
      pair_fold16(m, l, x);
    }
    pair_meet_put(lds, wave_c, wave_r, rt, lane, {m, l, pv});
  }
  pair_meet_store<3>(lds, tid, r0, a.n, ninf, [](float x, float y) { return fmaxf(x, y); }, {a.pm, a.pl, a.pp});
}

// one thread per logits row: merge the per-column-tile partials in tile order, write
// row_lse and the row's loss term (lse - positive logit)
__global__ __launch_bounds__(256) void ntxent_rows(const float* __restrict__ pm,
                                                   const float* __restrict__ pl,
                                                   const float* __restrict__ pp, int64_t n, int nparts,
                                                   float* __restrict__ row_loss,
                                                   float* __restrict__ row_lse) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  float m, l, pv = -__builtin_huge_valf();
  pair_merge_tiles(m, l, pm, pl, n, nparts, row, [&](int64_t o) { pv = fmaxf(pv, pp[o]); });
  const float lse2 = m + log2f(l);  // log2 domain
  if (row_lse) row_lse[row] = lse2 * kLn2;
  row_loss[row] = (lse2 - pv) * kLn2;
}

// the backward tile's per-row scalar: lse -> log2 domain
struct NtRowScalars {
  const float* row_lse;
  float* lse2;
  __device__ void operator()(int64_t i) const { lse2[i] = row_lse[i] * kLog2e; }
};

// dx_i = coef * rn_i * (g_i - (g_i . u_i) u_i), one wave per row; g = W.U (fp32), u = normalised row
template <typename T>
__global__ __launch_bounds__(256) void ntxent_bwd_finish(const float* __restrict__ g, const T* __restrict__ zn,
                                                         const T* __restrict__ z0, const T* __restrict__ z1,
                                                         int64_t b, int d, float coef, T* __restrict__ dz0,
                                                         T* __restrict__ dz1) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * b) return;
  const T* x = row < b ? z0 + row * d : z1 + (row - b) * d;
  T* dx = row < b ? dz0 + row * d : dz1 + (row - b) * d;
  const float rn = pair_row_inv_norm(x, d, lane);
  pair_project_row(dx, d, lane, coef * rn, [&](int k) { return g[row * d + k]; },
                   [&](int k) { return (float)zn[row * d + k]; });
}

struct NtWorkspace {
  void* zn;
  float *pm, *pl, *pp, *row_loss;
  // backward only
  _Float16 *wmat, *zt;
  float *lse2, *g;
  size_t bytes;
};

NtWorkspace nt_carve(void* base, int64_t b, int d, int dtype, bool bwd = false) {
  NtWorkspace w = {};
  WsCarver c(base);
  const size_t n = 2 * (size_t)b, nct = (size_t)hcir_cdiv(2 * b, 128);
  w.zn = c.take(n * d * hcir_dtype_bytes(dtype));
  w.pm = c.take<float>(nct * n);
  w.pl = c.take<float>(nct * n);
  w.pp = c.take<float>(nct * n);
  w.row_loss = c.take<float>(n);
  if (bwd) {
    w.wmat = c.take<_Float16>(n * n);
    w.zt = c.take<_Float16>(n * d);
    w.lse2 = c.take<float>(n);
    w.g = c.take<float>(n * d);
  }
  w.bytes = c.off;
  return w;
}

template <typename T>
int nt_run(const void* z0, const void* z1, int64_t b, int d, float inv_t, float* loss, float* row_lse,
           const NtWorkspace& w, hipStream_t st) {
  const int64_t n = 2 * b;
  const int nct = (int)hcir_cdiv(n, 128);
  hipLaunchKernelGGL(ntxent_prep<T>, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0, st,
                     static_cast<const T*>(z0), static_cast<const T*>(z1), b, d, static_cast<T*>(w.zn));
  HCIR_LAUNCH_CHECK();
  NtArgs a{w.zn, w.pm, w.pl, w.pp, n, b, d, inv_t * kLog2e, nullptr, nullptr};
  pair_launch_tiles<T>(ntxent_tiles<T, true>, ntxent_tiles<T, false>, dim3(nct, nct), a, st);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ntxent_rows, dim3((unsigned)hcir_cdiv(n, 256)), dim3(256), 0, st, w.pm, w.pl, w.pp, n,
                     nct, w.row_loss, row_lse);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_mean_reduce, dim3(1), dim3(1024), 0, st, w.row_loss, n, loss);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

template <typename T>
int nt_run_bwd(const void* z0, const void* z1, int64_t b, int d, float inv_t, const float* row_lse,
               float grad_out, void* dz0, void* dz1, const NtWorkspace& w, hipStream_t st) {
  const int64_t n = 2 * b;
  const int nct = (int)hcir_cdiv(n, 128);
  hipLaunchKernelGGL(ntxent_prep<T>, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0, st,
                     static_cast<const T*>(z0), static_cast<const T*>(z1), b, d, static_cast<T*>(w.zn));
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL((pair_transpose_f16<T, NtRowScalars>), dim3((unsigned)hcir_cdiv(n * d, 256)), dim3(256), 0, st,
                     static_cast<const T*>(w.zn), n, d, w.zt, NtRowScalars{row_lse, w.lse2});
  HCIR_LAUNCH_CHECK();
  NtArgs a{w.zn, w.pm, w.pl, w.pp, n, b, d, inv_t * kLog2e, w.lse2, w.wmat};
  pair_launch_tiles<T>(ntxent_tiles<T, true, true>, ntxent_tiles<T, false, true>, dim3(nct, nct), a, st);
  HCIR_LAUNCH_CHECK();
  // g[2B][D] = W[2B][2B] . U[2B][D]  ==  hcir_gemm_f16(A = W, "weights" = U^T [D][2B])
  const int rc = hcir_gemm_f16(w.wmat, n, w.zt, n, nullptr, nullptr, n, d, (int32_t)n, HCIR_EPI_BIAS_F32,
                               w.g, d, st);
  if (rc != HCIR_OK) return rc;
  hipLaunchKernelGGL(ntxent_bwd_finish<T>, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0, st, w.g,
                     static_cast<const T*>(w.zn), static_cast<const T*>(z0), static_cast<const T*>(z1), b, d,
                     grad_out * inv_t / (float)n, static_cast<T*>(dz0), static_cast<T*>(dz1));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // namespace

extern "C" {

size_t hcir_ntxent_bwd_workspace_bytes(int64_t b, int32_t d, int dtype) {
  if (b <= 0 || d <= 0) return 0;
  return nt_carve(nullptr, b, d, dtype, true).bytes;
}

int hcir_ntxent_bwd(const void* z0, const void* z1, int64_t b, int32_t d, int dtype, float inv_t,
                    const float* row_lse, float grad_out, void* dz0, void* dz1, void* workspace,
                    size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!z0 || !z1 || !row_lse || !dz0 || !dz1 || b <= 0 || d <= 0 || (d & 7) || (b & 3)) return HCIR_ERR_INVALID;
  if (!hcir_inv_t_ok(inv_t)) return HCIR_ERR_INVALID;  // as hcir_ntxent_fwd: no gradient of a loss it refuses
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const NtWorkspace w = nt_carve(workspace, b, d, dtype, true);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, nt_run_bwd, z0, z1, b, d, inv_t, row_lse, grad_out, dz0, dz1, w, st);
}

size_t hcir_ntxent_workspace_bytes(int64_t b, int32_t d, int dtype) {
  if (b <= 0 || d <= 0) return 0;
  return nt_carve(nullptr, b, d, dtype).bytes;
}

int hcir_ntxent_fwd(const void* z0, const void* z1, int64_t b, int32_t d, int dtype, float inv_t,
                    float* loss, float* row_lse, void* workspace, size_t workspace_bytes,
                    void* stream) {
  HCIR_ENTER();
  if (!z0 || !z1 || !loss || b <= 0 || d <= 0 || (d & 7)) return HCIR_ERR_INVALID;
  if (!hcir_inv_t_ok(inv_t)) return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const NtWorkspace w = nt_carve(workspace, b, d, dtype);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, nt_run, z0, z1, b, d, inv_t, loss, row_lse, w, st);
}

}  // extern "C"
