// ntxent_bank.hip — NT-Xent against a memory bank (the criterion of the DenseCL step), forward and backward, without
// materialising the N x (K + 1) logits in the forward.
//
// Semantics: lightly.loss.NTXentLoss(temperature, memory_bank_size=(K, D)).forward, as called by the DenseCL step at
// HairPretraining/src/pretrain_engine.py:85-87,309-312:
//   q_i = z0_i / max(||z0_i||, 1e-12),  k_i = z1_i / max(||z1_i||, 1e-12)                      i < N
//   logits_i = [ q_i.k_i , q_i.bank_0 , ... , q_i.bank_{K-1} ] * inv_t       bank rows as stored, not renormalised
//   loss = mean_i ( logsumexp(logits_i) - logits_i[0] )
// Backward: p_ij = exp(logit_ij - lse_i) (j = 0 the positive),
//   dq_i = c (sum_j p_ij bank_j + (p_i0 - 1) k_i),  dk_i = c (p_i0 - 1) q_i,  c = grad_out * inv_t / N,
//   through the normalisation's projection rn_i (g_i - (g_i.u_i) u_i).  The bank receives no gradient.
//
// Kernels
//   bank_prep        : one wave per row.  Rows < N: q_i and k_i normalised and rounded to the compute dtype into the
//                      workspace, k_i unrounded to k_unit (what the host enqueues), and the positive dot in fp32 from
//                      the rounded rows the MFMA reads.  Rows >= N: one bank row rounded to the compute dtype, and for
//                      the backward its fp16 transpose (the "weight" operand of P . bank on hcir_gemm_f16).
//   bank_tiles       : pair_tiles.h main loop in its two-matrix form: workgroup (x = bank tile of 128, y = row block of
//                      128); a lane owns one logits ROW and folds its 16 scores per MFMA tile into an online
//                      (max, sum-of-exp2) pair; bank columns >= K masked.  BWD = true: the same body writes
//                      P = exp(logit - lse) as fp16 [N][K].
//   bank_rows        : one thread per row merges the per-tile partials in tile order, then the positive as one more
//                      term; writes row_lse, row_pos and the row's loss term.
//   pair_mean_reduce : (pair_tiles.h) fixed-tree mean of the N loss terms.
//   bank_bwd_finish  : adds the positive's terms, scales, projects; dz1 == NULL skips the key's loads, sums and store
//                      (z1 is not read; the normalised key row still is: dq needs it).
// No atomics anywhere: the results are bit-identical from run to run.
#include "pair_tiles.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void bank_prep(const T* __restrict__ z0, const T* __restrict__ z1,
                                                 const float* __restrict__ bank, int64_t n, int64_t kb, int d,
                                                 T* __restrict__ qn, T* __restrict__ kn, T* __restrict__ bankc,
                                                 _Float16* __restrict__ bt, float* __restrict__ pos,
                                                 float* __restrict__ k_unit) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n + kb) return;
  if (row >= n) {
    const int64_t j = row - n;
    for (int k = lane; k < d; k += 64) {
      const float v = bank[j * d + k];
      bankc[j * d + k] = (T)v;
      if (bt) bt[(int64_t)k * kb + j] = (_Float16)v;
    }
    return;
  }
  const T* p0 = z0 + row * d;
  const T* p1 = z1 + row * d;
  float inv[2];
  pair_rows_inv_norm<2, T>({p0, p1}, d, lane, inv);
  const float inv0 = inv[0], inv1 = inv[1];
  float dot = 0.f;
  for (int k = lane; k < d; k += 64) {
    const float ku = (float)p1[k] * inv1;
    const T qr = (T)((float)p0[k] * inv0), kr = (T)ku;
    qn[row * d + k] = qr;
    kn[row * d + k] = kr;
    if (k_unit) k_unit[row * d + k] = ku;
    dot = __builtin_fmaf((float)qr, (float)kr, dot);
  }
  dot = wave_sum(dot);
  if (lane == 0) pos[row] = dot;
}

struct BkArgs {
  const void* qn;     // [N][D] normalised query rows, compute dtype
  const void* bankc;  // [K][D] bank rows, compute dtype
  float* pm;          // [nct][N] running max (log2 domain) per bank tile
  float* pl;          // [nct][N] sum of exp2
  int64_t n;
  int64_t kb;
  int d;
  float scale_log2;  // inv_t * log2(e)
  // backward (BWD = true): P[i][j] = exp(logit_ij - lse_i), fp16 [N][K]
  const float* row_lse;  // [N] natural-log domain, as the forward wrote it
  _Float16* pmat;
};

template <typename T, bool GLDS, bool BWD = false>
__global__ __launch_bounds__(256, 2) void bank_tiles(BkArgs a) {
  using Cfg = PairCfg<T>;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_c = wave >> 1, wave_r = wave & 1;
  const int h = lane >> 5;
  const int64_t c0 = (int64_t)blockIdx.x * 128, r0 = (int64_t)blockIdx.y * 128;

  f32x16 acc[2][2];
  pair_tile_products<T, GLDS>(acc, lds, static_cast<const T*>(a.bankc), c0, a.kb, static_cast<const T*>(a.qn), r0,
                              a.n, a.d, tid, lane, wave_c, wave_r);

  const float ninf = -__builtin_huge_valf();
  if constexpr (BWD) {
    pair_write_image(acc, a.pmat, c0, a.kb, r0, a.n, wave_c, wave_r, lane, [&](int64_t row) {
      const float lrow = a.row_lse[row] * kLog2e;
      return [=](int64_t, f32x4 dot) {
        f32x4 p;
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = __builtin_amdgcn_exp2f(dot[e] * a.scale_log2 - lrow);
        return p;
      };
    });
    return;
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    float m = ninf, l = 0.f;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      float x[16];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        x[i] = pair_col(c0, wave_c, ct, i, h) < a.kb ? acc[ct][rt][i] * a.scale_log2 : ninf;
      pair_fold16(m, l, x);
    }
    pair_meet_put(lds, wave_c, wave_r, rt, lane, {m, l});
  }
  pair_meet_store<2>(lds, tid, r0, a.n, 0.f, PairSum(), {a.pm, a.pl});
}

// one thread per logits row: merge the per-bank-tile partials in tile order, then the positive as one more term
__global__ __launch_bounds__(256) void bank_rows(const float* __restrict__ pm, const float* __restrict__ pl,
                                                 const float* __restrict__ pos, int64_t n, int nparts, float inv_t,
                                                 float scale_log2, float* __restrict__ row_loss,
                                                 float* __restrict__ row_lse, float* __restrict__ row_pos) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  float m, l;
  pair_merge_tiles(m, l, pm, pl, n, nparts, row, [](int64_t) {});
  const float pv = pos[row] * scale_log2;
  {  // not pair_lse_merge<true>(m, l, pv, 1): that one is compiled without contraction, this term is compiled with it
     // (pv - mn and the sum are fused), and the results are pinned to the bit
    const float mn = fmaxf(m, pv);
    l = l * exp2f(m - mn) + exp2f(pv - mn);
    m = mn;
  }
  const float lse2 = m + log2f(l);  // log2 domain
  if (row_lse) row_lse[row] = lse2 * kLn2;
  if (row_pos) row_pos[row] = pos[row] * inv_t;
  row_loss[row] = (lse2 - pv) * kLn2;
}

// g = P.bank (fp32) -> dz0_i = coef rn_i (gq_i - (gq_i.q_i) q_i), gq_i = g_i + (p_i0 - 1) k_i;
//                      dz1_i = coef rn_i (gk_i - (gk_i.k_i) k_i), gk_i = (p_i0 - 1) q_i.  One wave per row.
template <typename T>
__global__ __launch_bounds__(256) void bank_bwd_finish(const float* __restrict__ g, const T* __restrict__ qn,
                                                       const T* __restrict__ kn, const T* __restrict__ z0,
                                                       const T* __restrict__ z1, const float* __restrict__ row_lse,
                                                       const float* __restrict__ row_pos, int64_t n, int d,
                                                       float coef, T* __restrict__ dz0, T* __restrict__ dz1) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float c0 = __builtin_amdgcn_exp2f((row_pos[row] - row_lse[row]) * kLog2e) - 1.0f;
  const auto q = [&](int k) { return (float)qn[row * d + k]; };
  const auto kk = [&](int k) { return (float)kn[row * d + k]; };
  const float rn0 = pair_row_inv_norm(z0 + row * d, d, lane);
  pair_project_row(dz0 + row * d, d, lane, coef * rn0,
                   [&](int k) { return __builtin_fmaf(c0, kk(k), g[row * d + k]); }, q);
  if (!dz1) return;  // the key's norm and q.k are the key's gradient's alone
  const float rn1 = pair_row_inv_norm(z1 + row * d, d, lane);
  pair_project_row(dz1 + row * d, d, lane, coef * rn1 * c0, q, kk);
}

struct BkWorkspace {
  void *qn, *kn, *bankc;
  float *pm, *pl, *pos, *row_loss;
  // backward only
  _Float16 *pmat, *bt;
  float* g;
  size_t bytes;
};

BkWorkspace bk_carve(void* base, int64_t n64, int64_t kb64, int d, int dtype, bool bwd) {
  BkWorkspace w = {};
  WsCarver c(base);
  const size_t n = (size_t)n64, kb = (size_t)kb64, es = hcir_dtype_bytes(dtype), nct = (size_t)hcir_cdiv(kb64, 128);
  w.qn = c.take(n * d * es);
  w.kn = c.take(n * d * es);
  w.bankc = c.take(kb * d * es);
  w.pos = c.take<float>(n);
  if (bwd) {
    w.pmat = c.take<_Float16>(n * kb);
    w.bt = c.take<_Float16>(kb * d);
    w.g = c.take<float>(n * d);
  } else {
    w.pm = c.take<float>(nct * n);
    w.pl = c.take<float>(nct * n);
    w.row_loss = c.take<float>(n);
  }
  w.bytes = c.off;
  return w;
}

template <typename T>
void bk_launch_prep(const void* z0, const void* z1, const float* bank, int64_t n, int64_t kb, int d,
                    const BkWorkspace& w, float* k_unit, hipStream_t st) {
  hipLaunchKernelGGL(bank_prep<T>, dim3((unsigned)hcir_cdiv(n + kb, 4)), dim3(256), 0, st, static_cast<const T*>(z0),
                     static_cast<const T*>(z1), bank, n, kb, d, static_cast<T*>(w.qn), static_cast<T*>(w.kn),
                     static_cast<T*>(w.bankc), w.bt, w.pos, k_unit);
}

template <typename T>
int bk_run(const void* z0, const void* z1, const float* bank, int64_t n, int64_t kb, int d, float inv_t, float* loss,
           float* row_lse, float* row_pos, float* k_unit, const BkWorkspace& w, hipStream_t st) {
  const int nct = (int)hcir_cdiv(kb, 128), nrb = (int)hcir_cdiv(n, 128);
  bk_launch_prep<T>(z0, z1, bank, n, kb, d, w, k_unit, st);
  HCIR_LAUNCH_CHECK();
  BkArgs a{w.qn, w.bankc, w.pm, w.pl, n, kb, d, inv_t * kLog2e, nullptr, nullptr};
  pair_launch_tiles<T>(bank_tiles<T, true>, bank_tiles<T, false>, dim3(nct, nrb), a, st);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bank_rows, dim3((unsigned)hcir_cdiv(n, 256)), dim3(256), 0, st, w.pm, w.pl, w.pos, n, nct, inv_t,
                     inv_t * kLog2e, w.row_loss, row_lse, row_pos);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_mean_reduce, dim3(1), dim3(1024), 0, st, w.row_loss, n, loss);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

template <typename T>
int bk_run_bwd(const void* z0, const void* z1, const float* bank, int64_t n, int64_t kb, int d, float inv_t,
               const float* row_lse, const float* row_pos, float grad_out, void* dz0, void* dz1, const BkWorkspace& w,
               hipStream_t st) {
  const int nct = (int)hcir_cdiv(kb, 128), nrb = (int)hcir_cdiv(n, 128);
  bk_launch_prep<T>(z0, z1, bank, n, kb, d, w, nullptr, st);
  HCIR_LAUNCH_CHECK();
  BkArgs a{w.qn, w.bankc, nullptr, nullptr, n, kb, d, inv_t * kLog2e, row_lse, w.pmat};
  pair_launch_tiles<T>(bank_tiles<T, true, true>, bank_tiles<T, false, true>, dim3(nct, nrb), a, st);
  HCIR_LAUNCH_CHECK();
  // g[N][D] = P[N][K] . bank[K][D]  ==  hcir_gemm_f16(A = P, "weights" = bank^T [D][K])
  const int rc = hcir_gemm_f16(w.pmat, kb, w.bt, kb, nullptr, nullptr, n, d, (int32_t)kb, HCIR_EPI_BIAS_F32, w.g, d, st);
  if (rc != HCIR_OK) return rc;
  hipLaunchKernelGGL(bank_bwd_finish<T>, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0, st, w.g,
                     static_cast<const T*>(w.qn), static_cast<const T*>(w.kn), static_cast<const T*>(z0),
                     static_cast<const T*>(z1), row_lse, row_pos, n, d, grad_out * inv_t / (float)n,
                     static_cast<T*>(dz0), static_cast<T*>(dz1));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // namespace

extern "C" {

size_t hcir_ntxent_bank_workspace_bytes(int64_t n, int64_t k, int32_t d, int dtype, int backward) {
  if (n <= 0 || k <= 0 || d <= 0) return 0;
  return bk_carve(nullptr, n, k, d, dtype, backward != 0).bytes;
}

int hcir_ntxent_bank_fwd(const void* z0, const void* z1, const float* bank, int64_t n, int64_t k, int32_t d, int dtype,
                         float inv_t, float* loss, float* row_lse, float* row_pos, float* k_unit, void* workspace,
                         size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!z0 || !z1 || !bank || !loss || !pair_rows_cols_shape_ok(n, k, d, inv_t)) return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const BkWorkspace w = bk_carve(workspace, n, k, d, dtype, false);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, bk_run, z0, z1, bank, n, k, d, inv_t, loss, row_lse, row_pos, k_unit, w, st);
}

int hcir_ntxent_bank_bwd(const void* z0, const void* z1, const float* bank, int64_t n, int64_t k, int32_t d, int dtype,
                         float inv_t, const float* row_lse, const float* row_pos, float grad_out, void* dz0, void* dz1,
                         void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!z0 || !z1 || !bank || !row_lse || !row_pos || !dz0 || !pair_rows_cols_shape_ok(n, k, d, inv_t) || (k & 7))
    return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const BkWorkspace w = bk_carve(workspace, n, k, d, dtype, true);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, bk_run_bwd, z0, z1, bank, n, k, d, inv_t, row_lse, row_pos, grad_out, dz0, dz1, w,
                             st);
}

}  // extern "C"
