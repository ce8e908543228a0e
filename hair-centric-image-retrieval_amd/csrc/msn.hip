// msn.hip — the MSN criterion (lightly.loss.MSNLoss; HairPretraining/src/pretrain_engine.py:242-275), forward and
// backward, without materialising an [N, K] matrix in the forward.
//
// Semantics (V = N / B anchor views per target; row i of the anchors pairs with target i mod B):
//   a_i = anchors_i / max(||anchors_i||, 1e-12), t_j likewise, c_k = prototypes_k / max(||prototypes_k||, 1e-12)
//   p_ik = softmax_k(a_i.c_k * inv_t)
//   q_jk = softmax_k(t_j.c_k * inv_t_sharp)                 inv_t_sharp = 1 / (T * Ts): the sharpened softmax as ONE
//                                                            softmax, which does not underflow as softmax ** (1 / Ts)
//   Sinkhorn, iterations > 0, as two scaling vectors over the stored q:  v = 1;
//     repeat: u_k = 1 / (K sum_j q_jk v_j);  v_j = 1 / (B sum_k u_k q_jk)
//     q_jk <- u_k q_jk / sum_k u_k q_jk                       (= B u_k q_jk v_j of the last round; lightly's
//                                                              Q / sum(Q) cancels in the first u)
//   loss = mean_i sum_k -q_(i mod B)k log p_ik + w (sum_k pbar_k log pbar_k + log K),   pbar_k = mean_i p_ik
// Backward (anchors only; the prototypes are passed as data by the reference and receive no gradient):
//   G_ik = p_ik (sum_k tgt_ik + w (log pbar_k - e_i)) - tgt_ik,  e_i = sum_k p_ik log pbar_k
//   g_i = sum_k G_ik c_k,  danchors_i = grad_out * inv_t / N * rn_i (g_i - (g_i.a_i) a_i)
//
// Kernels
//   msn_prep      : one wave per row.  Anchor / target rows: the inverse norm (the MFMA reads the rows as they are
//                   given and the epilogue scales by it: 16-bit rows are never rounded a second time).  Prototype rows:
//                   normalised, rounded to the compute dtype and, for the backward, to the fp16 transpose that is the
//                   "weight" operand of G . c on hcir_gemm_f16.
//   msn_tiles     : pair_tiles.h main loop, rows against prototypes; a lane owns one logits ROW.  Five epilogues:
//                   LOGITS (the targets' scaled logits into q), LSE (online (max, sum of exp2), sum tgt x, sum tgt per
//                   prototype tile), PBAR (column sums of p per 128-row block), E (e_i and sum tgt per prototype tile),
//                   G (the fp16 image of G).
//   msn_softmax_rows, msn_col_scale, msn_row_scale : the targets' softmax and the Sinkhorn rounds: small launches
//                   (16 workgroups per column round at K = 1024), each sum in a fixed order.
//   msn_rows      : one thread per row merges the per-tile partials in tile order.
//   msn_finish    : one workgroup: the cross-entropy mean, pbar from the row-block partials in block order, the
//                   regulariser, the loss.
//   msn_bwd_finish: inv_t, grad_out, 1 / N and the normalisation's projection, one wave per row.
// No atomics anywhere: the results are bit-identical from run to run.
#include <float.h>

#include "pair_tiles.h"

namespace {

enum { MSN_LOGITS = 0, MSN_LSE, MSN_PBAR, MSN_E, MSN_G };

// rows < n: rinv[row] = 1 / max(||x_row||, 1e-12).  rows >= n: prototype row -> unit row in the compute dtype (cn) and
// its fp16 transpose (ct [D][K], may be NULL).
template <typename T>
__global__ __launch_bounds__(256) void msn_prep(const T* __restrict__ x, int64_t n, const float* __restrict__ protos,
                                                int64_t kp, int d, float* __restrict__ rinv, T* __restrict__ cn,
                                                _Float16* __restrict__ ct) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n + kp) return;
  if (row < n) {
    const float inv = pair_row_inv_norm(x + row * d, d, lane);
    if (lane == 0) rinv[row] = inv;
    return;
  }
  const int64_t j = row - n;
  const float inv = pair_row_inv_norm(protos + j * d, d, lane);
  for (int k = lane; k < d; k += 64) {
    const float v = protos[j * d + k] * inv;
    cn[j * d + k] = (T)v;
    if (ct) ct[(int64_t)k * kp + j] = (_Float16)v;
  }
}

struct MsnArgs {
  const void* rows;   // [N][D] anchor or target rows as given
  const void* cols;   // [K][D] unit prototypes, compute dtype
  const float* rinv;  // [N] inverse row norms
  int64_t n, kp, b;
  int d;
  int nct;
  float scale_log2;      // inv_t * log2(e)
  float w;               // regularization weight
  const float* q;        // [B][K] targets
  float* xout;           // LOGITS: [N][K] scaled logits, log2 domain
  float *pm, *pl, *pts;  // LSE: [nct][N] partials
  float* ptq;            // LSE, E: [nct][N] sum of the target row over the tile (read by G)
  float* pe;             // E: [nct][N] (read by G)
  const float* row_lse;  // [N] natural-log domain
  const float* pbar;     // [K]
  float* pbar_part;      // PBAR: [nrb][K]
  _Float16* gmat;        // G: [N][K]
};

__device__ __forceinline__ float msn_log_pbar(float pbar) {
  return __builtin_amdgcn_logf(fmaxf(pbar, FLT_MIN)) * kLn2;  // v_log_f32 is log2
}

template <typename T, bool GLDS, int MODE>
__global__ __launch_bounds__(256, 2) void msn_tiles(MsnArgs a) {
  using Cfg = PairCfg<T>;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_c = wave >> 1, wave_r = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int64_t c0 = (int64_t)blockIdx.x * 128, r0 = (int64_t)blockIdx.y * 128;

  f32x16 acc[2][2];
  pair_tile_products<T, GLDS>(acc, lds, static_cast<const T*>(a.cols), c0, a.kp, static_cast<const T*>(a.rows), r0,
                              a.n, a.d, tid, lane, wave_c, wave_r);
  const float ninf = -__builtin_huge_valf();

  if constexpr (MODE == MSN_LOGITS) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int64_t row = r0 + wave_r * 64 + rt * 32 + r;
      if (row >= a.n) continue;
      const float sc = a.rinv[row] * a.scale_log2;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t col = pair_col(c0, wave_c, ct, i, h);
          if (col < a.kp) a.xout[row * a.kp + col] = acc[ct][rt][i] * sc;
        }
    }
  } else if constexpr (MODE == MSN_LSE || MODE == MSN_E) {
    // per row and prototype tile: LSE (m, l, sum tgt x, sum tgt); E (-, -, sum p log pbar, sum tgt)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int64_t row = r0 + wave_r * 64 + rt * 32 + r;
      row = row < a.n ? row : a.n - 1;
      const float sc = a.rinv[row] * a.scale_log2;
      const float* qrow = a.q + (row % a.b) * a.kp;
      float lrow = 0.f;
      if constexpr (MODE == MSN_E) lrow = a.row_lse[row] * kLog2e;
      float m = ninf, l = 0.f, ts = 0.f, tq = 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        float x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t col = pair_col(c0, wave_c, ct, i, h);
          const bool in = col < a.kp;
          const float xv = acc[ct][rt][i] * sc;
          const float t = in ? qrow[col] : 0.f;
          tq += t;
          if constexpr (MODE == MSN_LSE) {
            x[i] = in ? xv : ninf;
            ts = __builtin_fmaf(t, in ? xv : 0.f, ts);
          } else {
            const float p = in ? __builtin_amdgcn_exp2f(xv - lrow) : 0.f;
            ts = __builtin_fmaf(p, in ? msn_log_pbar(a.pbar[col]) : 0.f, ts);
          }
        }
        if constexpr (MODE == MSN_LSE) pair_fold16(m, l, x);
      }
      pair_meet_put(lds, wave_c, wave_r, rt, lane, {m, l, ts, tq});
    }
    if constexpr (MODE == MSN_LSE)
      pair_meet_store<4>(lds, tid, r0, a.n, 0.f, PairSum(), {a.pm, a.pl, a.pts, a.ptq});
    else
      pair_meet_store<4, false>(lds, tid, r0, a.n, 0.f, PairSum(), {nullptr, nullptr, a.pe, a.ptq});
  } else if constexpr (MODE == MSN_PBAR) {
    // column sums of p over this block's rows: the two row tiles in the lane, the 32 rows of a lane half by a fixed
    // butterfly, the two row waves in LDS
    float* red = reinterpret_cast<float*>(lds);
    float s[2][16];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) s[ct][i] = 0.f;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int64_t row = r0 + wave_r * 64 + rt * 32 + r;
      const bool valid = row < a.n;
      const int64_t rc = valid ? row : a.n - 1;
      const float sc = a.rinv[rc] * a.scale_log2;
      const float lrow = a.row_lse[rc] * kLog2e;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          s[ct][i] += valid ? __builtin_amdgcn_exp2f(acc[ct][rt][i] * sc - lrow) : 0.f;
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v = s[ct][i];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
        if (r == 0) red[wave_r * 128 + wave_c * 64 + ct * 32 + acc_row(i, h)] = v;
      }
    __syncthreads();
    if (tid < 128 && c0 + tid < a.kp) a.pbar_part[(int64_t)blockIdx.y * a.kp + c0 + tid] = red[tid] + red[128 + tid];
  } else {
    // G.  1 / N and grad_out stay out of the fp16 image (p / N would be an fp16 subnormal at the workload's N)
    pair_write_image(acc, a.gmat, c0, a.kp, r0, a.n, wave_c, wave_r, lane, [&](int64_t row) {
      const float sc = a.rinv[row] * a.scale_log2;
      const float lrow = a.row_lse[row] * kLog2e;
      const float* qrow = a.q + (row % a.b) * a.kp;
      float tq = 0.f, e = 0.f;
      for (int p = 0; p < a.nct; ++p) {  // tile order
        tq += a.ptq[(int64_t)p * a.n + row];
        e += a.pe[(int64_t)p * a.n + row];
      }
      return [=](int64_t col0, f32x4 dot) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(qrow + col0);
        const f32x4 pb = *reinterpret_cast<const f32x4*>(a.pbar + col0);
        f32x4 g;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float p = __builtin_amdgcn_exp2f(dot[k] * sc - lrow);
          g[k] = p * (tq + a.w * (msn_log_pbar(pb[k]) - e)) - t[k];
        }
        return g;
      };
    });
  }
}

// one wave per target row: x (log2 domain) -> exp2(x - max) / sum
__global__ __launch_bounds__(256) void msn_softmax_rows(float* __restrict__ q, int64_t b, int64_t kp) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= b) return;
  float* p = q + row * kp;
  float m = -__builtin_huge_valf();
  for (int64_t k = lane; k < kp; k += 64) m = fmaxf(m, p[k]);
  m = wave_max(m);
  float s = 0.f;
  for (int64_t k = lane; k < kp; k += 64) s += __builtin_amdgcn_exp2f(p[k] - m);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int64_t k = lane; k < kp; k += 64) p[k] = __builtin_amdgcn_exp2f(p[k] - m) * inv;
}

// u_k = 1 / (K sum_j q_jk v_j) (v == NULL: v = 1).  64 columns x 4 row groups per workgroup; a group walks its rows in
// order, the four groups meet in LDS in order.
__global__ __launch_bounds__(256) void msn_col_scale(const float* __restrict__ q, const float* __restrict__ v,
                                                     int64_t b, int64_t kp, float* __restrict__ u) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + c;
  float s = 0.f;
  if (col < kp)
    for (int64_t j = g; j < b; j += 4) s = __builtin_fmaf(q[j * kp + col], v ? v[j] : 1.0f, s);
  red[g][c] = s;
  __syncthreads();
  if (g == 0 && col < kp) u[col] = 1.0f / ((float)kp * (((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]));
}

// one wave per target row: s_j = sum_k u_k q_jk.  LAST: q_jk <- u_k q_jk / s_j, else v_j = 1 / (B s_j).
template <bool LAST>
__global__ __launch_bounds__(256) void msn_row_scale(float* __restrict__ q, const float* __restrict__ u, int64_t b,
                                                     int64_t kp, float* __restrict__ v) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= b) return;
  float* p = q + row * kp;
  float s = 0.f;
  for (int64_t k = lane; k < kp; k += 64) s = __builtin_fmaf(u[k], p[k], s);
  s = wave_sum(s);
  if constexpr (LAST) {
    const float inv = 1.0f / s;
    for (int64_t k = lane; k < kp; k += 64) p[k] = u[k] * p[k] * inv;
  } else {
    if (lane == 0) v[row] = 1.0f / ((float)b * s);
  }
}

// one thread per anchor row: merge the per-tile partials in tile order
__global__ __launch_bounds__(256) void msn_rows(const float* __restrict__ pm, const float* __restrict__ pl,
                                                const float* __restrict__ pts, const float* __restrict__ ptq,
                                                int64_t n, int nparts, float* __restrict__ row_lse,
                                                float* __restrict__ row_ce) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  float m, l, ts = 0.f, tq = 0.f;
  pair_merge_tiles(m, l, pm, pl, n, nparts, row, [&](int64_t o) {
    ts += pts[o];
    tq += ptq[o];
  });
  const float lse2 = m + log2f(l);  // log2 domain
  row_lse[row] = lse2 * kLn2;
  row_ce[row] = (lse2 * tq - ts) * kLn2;  // sum_k -tgt_k (x_k - lse)
}

// one workgroup: ce = mean of the row terms; pbar_k from the row-block partials in block order; reg = sum_k pbar_k
// log pbar_k + log K; loss = ce + w reg.  Fixed order and tree.
__global__ __launch_bounds__(1024) void msn_finish(const float* __restrict__ row_ce, int64_t n,
                                                   const float* __restrict__ pbar_part, int nrb, int64_t kp, float w,
                                                   float* __restrict__ pbar, float* __restrict__ loss,
                                                   float* __restrict__ parts) {
  __shared__ float red[2][1024];
  float ce = 0.f, rg = 0.f;
  for (int64_t row = threadIdx.x; row < n; row += 1024) ce += row_ce[row];
  for (int64_t k = threadIdx.x; k < kp; k += 1024) {
    float s = 0.f;
    for (int p = 0; p < nrb; ++p) s += pbar_part[(int64_t)p * kp + k];
    s /= (float)n;
    pbar[k] = s;
    rg = __builtin_fmaf(s, msn_log_pbar(s), rg);
  }
  red[0][threadIdx.x] = ce;
  red[1][threadIdx.x] = rg;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float c = red[0][0] / (float)n, g = red[1][0] + logf((float)kp);
    *loss = c + w * g;
    if (parts) {
      parts[0] = c;
      parts[1] = g;
    }
  }
}

// g = G . c (fp32) -> danchors_i = coef rn_i (g_i - (g_i.a_i) a_i), a_i the unit row in fp32.  One wave per row.
template <typename T>
__global__ __launch_bounds__(256) void msn_bwd_finish(const float* __restrict__ g, const T* __restrict__ x,
                                                      const float* __restrict__ rinv, int64_t n, int d, float coef,
                                                      T* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float rn = rinv[row];
  pair_project_row(dx + row * d, d, lane, coef * rn, [&](int k) { return g[row * d + k]; },
                   [&](int k) { return (float)x[row * d + k] * rn; });
}

enum { WS_TARGETS = 0, WS_FWD = 1, WS_BWD = 2 };

struct MsnWorkspace {
  void* cn;
  float* rinv;
  float *u, *v;                                     // targets
  float *pm, *pl, *pts, *ptq, *row_ce, *pbar_part;  // forward
  float *row_lse, *pbar;                            // forward, where the caller keeps neither
  float *pe, *g;                                    // backward (with ptq)
  _Float16 *ct, *gmat;
  size_t bytes;
};

MsnWorkspace msn_carve(void* base, int64_t n64, int64_t kp64, int d, int dtype, int stage) {
  MsnWorkspace w = {};
  WsCarver c(base);
  const size_t n = (size_t)n64, kp = (size_t)kp64;
  const size_t nct = (size_t)hcir_cdiv(kp64, 128), nrb = (size_t)hcir_cdiv(n64, 128);
  w.cn = c.take(kp * d * hcir_dtype_bytes(dtype));
  w.rinv = c.take<float>(n);
  if (stage == WS_TARGETS) {
    w.u = c.take<float>(kp);
    w.v = c.take<float>(n);
  } else if (stage == WS_FWD) {
    w.pm = c.take<float>(nct * n);
    w.pl = c.take<float>(nct * n);
    w.pts = c.take<float>(nct * n);
    w.ptq = c.take<float>(nct * n);
    w.row_ce = c.take<float>(n);
    w.pbar_part = c.take<float>(nrb * kp);
    w.row_lse = c.take<float>(n);
    w.pbar = c.take<float>(kp);
  } else {
    w.ptq = c.take<float>(nct * n);
    w.pe = c.take<float>(nct * n);
    w.ct = c.take<_Float16>(kp * d);
    w.gmat = c.take<_Float16>(n * kp);
    w.g = c.take<float>(n * d);
  }
  w.bytes = c.off;
  return w;
}

template <typename T, int MODE>
void msn_launch_tiles(const MsnArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)hcir_cdiv(a.kp, 128), (unsigned)hcir_cdiv(a.n, 128));
  pair_launch_tiles<T>(msn_tiles<T, true, MODE>, msn_tiles<T, false, MODE>, grid, a, st);
}

template <typename T>
void msn_launch_prep(const void* x, int64_t n, const float* protos, int64_t kp, int d, const MsnWorkspace& w,
                     hipStream_t st) {
  hipLaunchKernelGGL(msn_prep<T>, dim3((unsigned)hcir_cdiv(n + kp, 4)), dim3(256), 0, st, static_cast<const T*>(x), n,
                     protos, kp, d, w.rinv, static_cast<T*>(w.cn), w.ct);
}

template <typename T>
int msn_run_targets(const void* targets, const float* protos, int64_t b, int64_t kp, int d, float inv_t_sharp,
                    int iterations, float* q, const MsnWorkspace& w, hipStream_t st) {
  msn_launch_prep<T>(targets, b, protos, kp, d, w, st);
  HCIR_LAUNCH_CHECK();
  MsnArgs a = {};
  a.rows = targets;
  a.cols = w.cn;
  a.rinv = w.rinv;
  a.n = b;
  a.kp = kp;
  a.b = b;
  a.d = d;
  a.scale_log2 = inv_t_sharp * kLog2e;
  a.xout = q;
  msn_launch_tiles<T, MSN_LOGITS>(a, st);
  HCIR_LAUNCH_CHECK();
  const dim3 rows((unsigned)hcir_cdiv(b, 4)), cols((unsigned)hcir_cdiv(kp, 64));
  hipLaunchKernelGGL(msn_softmax_rows, rows, dim3(256), 0, st, q, b, kp);
  HCIR_LAUNCH_CHECK();
  for (int it = 0; it < iterations; ++it) {
    hipLaunchKernelGGL(msn_col_scale, cols, dim3(256), 0, st, q, it ? w.v : nullptr, b, kp, w.u);
    HCIR_LAUNCH_CHECK();
    if (it + 1 < iterations)
      hipLaunchKernelGGL(msn_row_scale<false>, rows, dim3(256), 0, st, q, w.u, b, kp, w.v);
    else
      hipLaunchKernelGGL(msn_row_scale<true>, rows, dim3(256), 0, st, q, w.u, b, kp, w.v);
    HCIR_LAUNCH_CHECK();
  }
  return HCIR_OK;
}

template <typename T>
int msn_run_fwd(const void* anchors, const float* protos, const float* q, int64_t n, int64_t b, int64_t kp, int d,
                float inv_t, float weight, float* loss, float* parts, float* row_lse, float* pbar,
                const MsnWorkspace& w, hipStream_t st) {
  const int nct = (int)hcir_cdiv(kp, 128), nrb = (int)hcir_cdiv(n, 128);
  row_lse = row_lse ? row_lse : w.row_lse;
  pbar = pbar ? pbar : w.pbar;
  msn_launch_prep<T>(anchors, n, protos, kp, d, w, st);
  HCIR_LAUNCH_CHECK();
  MsnArgs a = {};
  a.rows = anchors;
  a.cols = w.cn;
  a.rinv = w.rinv;
  a.n = n;
  a.kp = kp;
  a.b = b;
  a.d = d;
  a.nct = nct;
  a.scale_log2 = inv_t * kLog2e;
  a.w = weight;
  a.q = q;
  a.pm = w.pm;
  a.pl = w.pl;
  a.pts = w.pts;
  a.ptq = w.ptq;
  a.row_lse = row_lse;
  a.pbar_part = w.pbar_part;
  msn_launch_tiles<T, MSN_LSE>(a, st);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(msn_rows, dim3((unsigned)hcir_cdiv(n, 256)), dim3(256), 0, st, w.pm, w.pl, w.pts, w.ptq, n, nct,
                     row_lse, w.row_ce);
  HCIR_LAUNCH_CHECK();
  msn_launch_tiles<T, MSN_PBAR>(a, st);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(msn_finish, dim3(1), dim3(1024), 0, st, w.row_ce, n, w.pbar_part, nrb, kp, weight, pbar, loss,
                     parts);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

template <typename T>
int msn_run_bwd(const void* anchors, const float* protos, const float* q, int64_t n, int64_t b, int64_t kp, int d,
                float inv_t, float weight, const float* row_lse, const float* pbar, float grad_out, void* danchors,
                const MsnWorkspace& w, hipStream_t st) {
  msn_launch_prep<T>(anchors, n, protos, kp, d, w, st);
  HCIR_LAUNCH_CHECK();
  MsnArgs a = {};
  a.rows = anchors;
  a.cols = w.cn;
  a.rinv = w.rinv;
  a.n = n;
  a.kp = kp;
  a.b = b;
  a.d = d;
  a.nct = (int)hcir_cdiv(kp, 128);
  a.scale_log2 = inv_t * kLog2e;
  a.w = weight;
  a.q = q;
  a.ptq = w.ptq;
  a.pe = w.pe;
  a.row_lse = row_lse;
  a.pbar = pbar;
  a.gmat = w.gmat;
  msn_launch_tiles<T, MSN_E>(a, st);
  HCIR_LAUNCH_CHECK();
  msn_launch_tiles<T, MSN_G>(a, st);
  HCIR_LAUNCH_CHECK();
  // g[N][D] = G[N][K] . c[K][D]  ==  hcir_gemm_f16(A = G, "weights" = c^T [D][K])
  const int rc = hcir_gemm_f16(w.gmat, kp, w.ct, kp, nullptr, nullptr, n, d, (int32_t)kp, HCIR_EPI_BIAS_F32, w.g, d, st);
  if (rc != HCIR_OK) return rc;
  hipLaunchKernelGGL(msn_bwd_finish<T>, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0, st, w.g,
                     static_cast<const T*>(anchors), w.rinv, n, d, grad_out * inv_t / (float)n,
                     static_cast<T*>(danchors));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // namespace

extern "C" {

size_t hcir_msn_workspace_bytes(int64_t n, int64_t k, int32_t d, int dtype, int stage) {
  if (n <= 0 || k <= 0 || d <= 0 || stage < WS_TARGETS || stage > WS_BWD) return 0;
  return msn_carve(nullptr, n, k, d, dtype, stage).bytes;
}

int hcir_msn_targets(const void* targets, const float* prototypes, int64_t b, int64_t k, int32_t d, int dtype,
                     float inv_t_sharp, int32_t iterations, float* q, void* workspace, size_t workspace_bytes,
                     void* stream) {
  HCIR_ENTER();
  if (!targets || !prototypes || !q || !pair_rows_cols_shape_ok(b, k, d, inv_t_sharp) || iterations < 0)
    return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const MsnWorkspace w = msn_carve(workspace, b, k, d, dtype, WS_TARGETS);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, msn_run_targets, targets, prototypes, b, k, d, inv_t_sharp, iterations, q, w, st);
}

int hcir_msn_fwd(const void* anchors, const float* prototypes, const float* q, int64_t n, int64_t b, int64_t k,
                 int32_t d, int dtype, float inv_t, float reg_weight, float* loss, float* loss_parts, float* row_lse,
                 float* pbar, void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!anchors || !prototypes || !q || !loss || !pair_rows_cols_shape_ok(n, k, d, inv_t) || b <= 0 || n % b ||
      reg_weight != reg_weight)
    return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const MsnWorkspace w = msn_carve(workspace, n, k, d, dtype, WS_FWD);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, msn_run_fwd, anchors, prototypes, q, n, b, k, d, inv_t, reg_weight, loss,
                             loss_parts, row_lse, pbar, w, st);
}

int hcir_msn_bwd(const void* anchors, const float* prototypes, const float* q, int64_t n, int64_t b, int64_t k,
                 int32_t d, int dtype, float inv_t, float reg_weight, const float* row_lse, const float* pbar,
                 float grad_out, void* danchors, void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!anchors || !prototypes || !q || !row_lse || !pbar || !danchors || !pair_rows_cols_shape_ok(n, k, d, inv_t) ||
      (k & 7) || b <= 0 || n % b || reg_weight != reg_weight)
    return HCIR_ERR_INVALID;
  if (!hcir_float_dtype_ok(dtype)) return HCIR_ERR_UNSUPPORTED;
  const MsnWorkspace w = msn_carve(workspace, n, k, d, dtype, WS_BWD);
  if (!workspace || workspace_bytes < w.bytes) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return HCIR_DISPATCH_DTYPE(dtype, msn_run_bwd, anchors, prototypes, q, n, b, k, d, inv_t, reg_weight, row_lse, pbar,
                             grad_out, danchors, w, st);
}

}  // extern "C"
