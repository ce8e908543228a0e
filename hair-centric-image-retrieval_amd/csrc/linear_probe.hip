// linear_probe.hip — the reference's linear probe and class-variance analytics on the device.
//
//   hcir_softmax_xent_fwd_bwd  loss and gradient of the multinomial logistic regression that
//                              LogisticRegression(solver="lbfgs").fit minimises (HP/src/classification_engine.py:107-110):
//                              sum_i (logsumexp_c z_ic - z_i,y_i), gW = (P - Y)^T X, gb = colsum(P - Y), z = X W^T + b.
//   hcir_linear_argmax         LogisticRegression.predict (:111): arg-max of the logits, first maximum on ties.
//   hcir_class_sums_f64        per-class row counts and column sums   (:244,250-251: np.mean over the class / all rows)
//   hcir_class_scatter_f64     per-class sum_i ||x_i - m_c||^2        (:254)
//
// Shape of the loss/gradient kernel (DESIGN.md "Linear probe"): persistent workgroups of 4 waves walk row tiles of
// 32 * RT rows in a fixed order.  Per tile
//   1. logits: v_mfma_f32_32x32x2_f32 (exact fp32), the 4 waves split the k range, their partial tiles are added in
//      wave order into the LDS tile z[rows][classes];
//   2. row softmax in LDS, z <- P - Y in place, loss and gb partials in fp64 registers;
//   3. (P - Y)^T X with the same MFMA, x re-read from L2, added into THIS workgroup's [c, d] partial.
// The [n, c] probabilities never reach HBM.  A second kernel adds the per-workgroup partials in workgroup order in
// fp64: the same inputs give the same bits on every run (no floating-point atomics anywhere in this file).
#include "common.h"

namespace {

constexpr int kThreads = 256;  // 4 waves
constexpr int kWaves = 4;
constexpr int kMaxClasses = 1024;
constexpr int kMaxGroups = 512;                            // two workgroups per CU
constexpr size_t kPartialBudget = (size_t)128 << 20;       // bytes of [c, d] partials at most

__host__ __device__ inline int pad32(int c) { return (c + 31) & ~31; }

inline int row_tiles_per_pass(int64_t n, int32_t c) { return (c <= 64 && n >= 32768) ? 4 : 1; }

inline int xent_groups(int64_t n, int32_t d, int32_t c) {
  const int64_t tiles = hcir_cdiv(n, 32 * row_tiles_per_pass(n, c));
  int64_t cap = (int64_t)(kPartialBudget / ((size_t)c * d * sizeof(float)));
  cap = cap < 1 ? 1 : (cap > kMaxGroups ? kMaxGroups : cap);
  return (int)(tiles < cap ? tiles : cap);
}

struct XentWorkspace {
  size_t gw_off, gb_off, loss_off, bytes;
};
inline XentWorkspace xent_layout(int groups, int32_t d, int32_t c) {
  XentWorkspace w;
  w.gw_off = 0;
  w.gb_off = ((size_t)groups * c * d * sizeof(float) + 255) & ~(size_t)255;
  w.loss_off = w.gb_off + (((size_t)groups * c * sizeof(double) + 255) & ~(size_t)255);
  w.bytes = w.loss_off + (((size_t)groups * sizeof(double) + 255) & ~(size_t)255);
  return w;
}

// z[32 * RT][cpad] (LDS) = x[row0 .. row0 + 32 * RT) . w^T, rows past n and classes past c give 0.
// Wave v takes the k steps v, v + 4, ... of 8 columns each; lane (r = lane & 31, h = lane >> 5) loads columns
// 8 s + 4 h .. + 3 of row r of BOTH operands, so that the four MFMAs of a step see matching k on A and B.
// The partial tiles are added into z in wave order 0, 1, 2, 3.
template <int RT>
__device__ __forceinline__ void tile_logits(const float* __restrict__ x, int64_t ldx, int64_t n, int32_t d,
                                            const float* __restrict__ w, int32_t c, int32_t cpad, int64_t row0,
                                            float* z) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int ksteps = d >> 3;
  for (int c0 = 0; c0 < cpad; c0 += 32) {
    f32x16 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    const bool cls_ok = c0 + r < c;
    const float* wrow = w + (int64_t)(cls_ok ? c0 + r : 0) * d + 4 * h;
    const float* xrow[RT];
    bool row_ok[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int64_t row = row0 + 32 * t + r;
      row_ok[t] = row < n;
      xrow[t] = x + (row_ok[t] ? row : 0) * ldx + 4 * h;
    }
    for (int s = wave; s < ksteps; s += kWaves) {
      f32x4 wb = *reinterpret_cast<const f32x4*>(wrow + 8 * s);
      if (!cls_ok) wb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        f32x4 xa = *reinterpret_cast<const f32x4*>(xrow[t] + 8 * s);
        if (!row_ok[t]) xa = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j], wb[j], acc[t], 0, 0, 0);
      }
    }
    for (int v = 0; v < kWaves; ++v) {
      if (wave == v) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float* p = z + (32 * t + acc_row(i, h)) * cpad + c0 + r;
            *p = v == 0 ? acc[t][i] : *p + acc[t][i];
          }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int RT>
__global__ __launch_bounds__(kThreads) void xent_kernel(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                        int32_t d, const int64_t* __restrict__ labels,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        int32_t c, float* __restrict__ gw_part,
                                                        double* __restrict__ gb_part, double* __restrict__ loss_part,
                                                        int32_t* __restrict__ bad) {
  extern __shared__ float z[];  // [32 * RT][cpad]
  __shared__ double wave_loss[kWaves];
  constexpr int TM = 32 * RT;
  const int cpad = pad32(c);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int64_t tiles = (n + TM - 1) / TM;
  float* part = gw_part + (int64_t)blockIdx.x * c * d;
  const int dblocks = (d + 31) >> 5;
  const int out_tiles = (cpad >> 5) * dblocks;
  double loss = 0.0;     // wave-uniform
  double gb[4] = {0.0, 0.0, 0.0, 0.0};  // classes threadIdx.x + 256 k
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * TM;
    tile_logits<RT>(x, ldx, n, d, w, c, cpad, row0, z);
    // softmax of row rr by one wave; z <- P - Y
    for (int rr = wave; rr < TM; rr += kWaves) {
      const int64_t row = row0 + rr;
      float* zr = z + rr * cpad;
      int64_t y = -1;
      if (row < n) {
        y = labels[row];
        if (y < 0 || y >= c) {
          if (lane == 0) *bad = 1;
          y = -1;
        }
      }
      if (y < 0) {  // wave-uniform: a row past n or a bad label contributes nothing
        for (int cl = lane; cl < cpad; cl += 64) zr[cl] = 0.f;
        continue;
      }
      const float zy = zr[y] + b[y];
      float m = -INFINITY;
      for (int cl = lane; cl < c; cl += 64) m = fmaxf(m, zr[cl] + b[cl]);
      m = wave_max(m);
      float s = 0.f;
      for (int cl = lane; cl < c; cl += 64) s += expf(zr[cl] + b[cl] - m);
      s = wave_sum(s);
      for (int cl = lane; cl < cpad; cl += 64) {
        float v = 0.f;
        if (cl < c) v = expf(zr[cl] + b[cl] - m) / s - (cl == y ? 1.f : 0.f);
        zr[cl] = v;
      }
      loss += ((double)m + log((double)s)) - (double)zy;  // one fp64 log per row: no rounding common to all rows
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cl = threadIdx.x + kThreads * k;
      if (cl < c) {
        double s = 0.0;
        for (int rr = 0; rr < TM; ++rr) s += (double)z[rr * cpad + cl];
        gb[k] += s;
      }
    }
    // part[class][col] += sum_rows (P - Y)[row][class] * x[row][col]:  A[i = class][k = row], B[k = row][j = col]
    for (int ot = wave; ot < out_tiles; ot += kWaves) {
      const int cc = ot / dblocks, db = ot - cc * dblocks;
      const int col = 32 * db + r;
      const bool col_ok = col < d;
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const float* za = z + 32 * cc + r;
      const float* xb = x + (col_ok ? col : 0);
#pragma unroll 8
      for (int kk = 0; kk < TM / 2; ++kk) {
        const int rl = 2 * kk + h;
        const int64_t row = row0 + rl;
        const float a = za[rl * cpad];
        float bv = xb[(row < n ? row : 0) * ldx];
        if (!col_ok || row >= n) bv = 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
      }
      if (col_ok) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int cl = 32 * cc + acc_row(i, h);
          if (cl < c) {
            float* p = part + (int64_t)cl * d + col;
            *p = first ? acc[i] : *p + acc[i];
          }
        }
      }
    }
    first = false;
    __syncthreads();  // z is rewritten by the next tile
  }
  if (lane == 0) wave_loss[wave] = loss;
  __syncthreads();
  if (threadIdx.x == 0)
    loss_part[blockIdx.x] = ((wave_loss[0] + wave_loss[1]) + wave_loss[2]) + wave_loss[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cl = threadIdx.x + kThreads * k;
    if (cl < c) gb_part[(int64_t)blockIdx.x * c + cl] = gb[k];
  }
}

// element e < c * d: gw[e]; c * d <= e < c * d + c: gb; e == c * d + c: loss.  Partials in workgroup order, fp64.
__global__ void xent_reduce_kernel(const float* __restrict__ gw_part, const double* __restrict__ gb_part,
                                   const double* __restrict__ loss_part, int groups, int64_t cd, int32_t c,
                                   float* __restrict__ gw, float* __restrict__ gb, double* __restrict__ loss) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < cd) {
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += (double)gw_part[(int64_t)g * cd + e];
    gw[e] = (float)s;
  } else if (e < cd + c) {
    const int cl = (int)(e - cd);
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += gb_part[(int64_t)g * c + cl];
    gb[cl] = (float)s;
  } else if (e == cd + c) {
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += loss_part[g];
    *loss = s;
  }
}

__global__ __launch_bounds__(kThreads) void argmax_kernel(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                          int32_t d, const float* __restrict__ w,
                                                          const float* __restrict__ b, int32_t c,
                                                          int64_t* __restrict__ pred, float* __restrict__ logits) {
  extern __shared__ float z[];  // [32][cpad]
  const int cpad = pad32(c);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t tiles = (n + 31) / 32;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 32;
    tile_logits<1>(x, ldx, n, d, w, c, cpad, row0, z);
    for (int rr = wave; rr < 32; rr += kWaves) {
      const int64_t row = row0 + rr;
      if (row >= n) break;
      float best = -INFINITY;
      int bi = 0x7fffffff;
      for (int cl = lane; cl < c; cl += 64) {  // ascending cl per lane: strict > keeps the first maximum
        const float v = z[rr * cpad + cl] + b[cl];
        if (logits) logits[row * c + cl] = v;
        if (v > best || bi == 0x7fffffff) {
          best = v;
          bi = cl;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) {
          best = ov;
          bi = oi;
        }
      }
      if (lane == 0) pred[row] = bi;
    }
    __syncthreads();
  }
}

// ---- class moments -------------------------------------------------------------------------------------------------
// Split s of the rows, 64 columns per block: each thread owns ONE column of ONE split's [c, d] fp64 partial and adds its
// rows to it in row order, so no two threads ever touch the same address and the order of the sum is fixed.
__global__ __launch_bounds__(64) void class_sums_kernel(const float* __restrict__ x, int64_t n, int32_t d, int64_t ldx,
                                                        const int64_t* __restrict__ labels, int32_t c,
                                                        int64_t rows_per_split, double* __restrict__ part,
                                                        unsigned long long* __restrict__ counts,
                                                        int32_t* __restrict__ bad) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  const int64_t s = blockIdx.y;
  const int64_t i0 = s * rows_per_split;
  const int64_t i1 = i0 + rows_per_split < n ? i0 + rows_per_split : n;
  const bool counter = blockIdx.x == 0 && threadIdx.x == 0;
  double* mine = part + s * (int64_t)c * d + col;
  for (int64_t i = i0; i < i1; ++i) {
    const int64_t y = labels[i];
    if (y < 0 || y >= c) {
      if (counter) *bad = 1;
      continue;
    }
    if (counter) atomicAdd(counts + y, 1ull);
    if (col < d) mine[y * d] += (double)x[i * ldx + col];
  }
}

__global__ void class_sums_reduce_kernel(const double* __restrict__ part, int splits, int64_t cd,
                                         double* __restrict__ sums) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cd) return;
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += part[(int64_t)k * cd + e];
  sums[e] = s;
}

// one wave per row: row_sq[i] = sum_j (x_ij - m_{y_i, j})^2, lanes stride the columns, fixed butterfly order
__global__ __launch_bounds__(kThreads) void row_scatter_kernel(const float* __restrict__ x, int64_t n, int32_t d,
                                                               int64_t ldx, const int64_t* __restrict__ labels,
                                                               int32_t c, const double* __restrict__ means,
                                                               double* __restrict__ row_sq, int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t y = labels[i];
  if (y < 0 || y >= c) {
    if (lane == 0) {
      *bad = 1;
      row_sq[i] = 0.0;
    }
    return;
  }
  double a = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double t = (double)x[i * ldx + j] - means[y * d + j];
    a += t * t;
  }
  a = wave_sum_f64(a);
  if (lane == 0) row_sq[i] = a;
}

// one thread per class, rows in index order
__global__ void class_scatter_sum_kernel(const double* __restrict__ row_sq, const int64_t* __restrict__ labels,
                                         int64_t n, int32_t c, double* __restrict__ scatter) {
  const int cl = blockIdx.x * blockDim.x + threadIdx.x;
  if (cl >= c) return;
  double s = 0.0;
  for (int64_t i = 0; i < n; ++i)
    if (labels[i] == cl) s += row_sq[i];
  scatter[cl] = s;
}

inline int class_sum_splits(int64_t n, int32_t d, int32_t c) {
  int64_t cap = (int64_t)(((size_t)64 << 20) / ((size_t)c * d * sizeof(double)));
  cap = cap < 1 ? 1 : (cap > 64 ? 64 : cap);
  const int64_t by_rows = hcir_cdiv(n, 256);
  return (int)(by_rows < cap ? by_rows : cap);
}

inline bool probe_shape_ok(int64_t n, int32_t d, int32_t c) { return n > 0 && d > 0 && d % 8 == 0 && c >= 2; }
inline bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

template <typename K>
inline void allow_lds(K kernel, size_t bytes) {
  if (bytes > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

}  // namespace

extern "C" {

size_t hcir_softmax_xent_workspace_bytes(int64_t n, int32_t d, int32_t c) {
  if (!probe_shape_ok(n, d, c) || c > kMaxClasses) return 0;
  return xent_layout(xent_groups(n, d, c), d, c).bytes;
}

int hcir_softmax_xent_fwd_bwd(const float* x, int64_t n, int32_t d, int64_t ldx, const int64_t* labels,
                              const float* w, const float* b, int32_t c, double* loss, float* gw, float* gb,
                              int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!x || !labels || !w || !b || !loss || !gw || !gb || !bad || !workspace) return HCIR_ERR_INVALID;
  if (!probe_shape_ok(n, d, c) || ldx < d || !aligned16(x, ldx) || !aligned16(w, d)) return HCIR_ERR_INVALID;
  if (c > kMaxClasses) return HCIR_ERR_UNSUPPORTED;
  const int groups = xent_groups(n, d, c);
  const XentWorkspace lay = xent_layout(groups, d, c);
  if (workspace_bytes < lay.bytes) return HCIR_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  float* gw_part = reinterpret_cast<float*>(ws + lay.gw_off);
  double* gb_part = reinterpret_cast<double*>(ws + lay.gb_off);
  double* loss_part = reinterpret_cast<double*>(ws + lay.loss_off);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rt = row_tiles_per_pass(n, c);
  const size_t lds = (size_t)32 * rt * pad32(c) * sizeof(float);
  if (rt == 4) {
    allow_lds(xent_kernel<4>, lds);
    hipLaunchKernelGGL(xent_kernel<4>, dim3(groups), dim3(kThreads), lds, st, x, ldx, n, d, labels, w, b, c, gw_part,
                       gb_part, loss_part, bad);
  } else {
    allow_lds(xent_kernel<1>, lds);
    hipLaunchKernelGGL(xent_kernel<1>, dim3(groups), dim3(kThreads), lds, st, x, ldx, n, d, labels, w, b, c, gw_part,
                       gb_part, loss_part, bad);
  }
  HCIR_LAUNCH_CHECK();
  const int64_t cd = (int64_t)c * d;
  hipLaunchKernelGGL(xent_reduce_kernel, dim3((unsigned)hcir_cdiv(cd + c + 1, 256)), dim3(256), 0, st, gw_part,
                     gb_part, loss_part, groups, cd, c, gw, gb, loss);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_linear_argmax(const float* x, int64_t n, int32_t d, int64_t ldx, const float* w, const float* b, int32_t c,
                       int64_t* pred, float* logits, void* stream) {
  HCIR_ENTER();
  if (!x || !w || !b || !pred) return HCIR_ERR_INVALID;
  if (!probe_shape_ok(n, d, c) || ldx < d || !aligned16(x, ldx) || !aligned16(w, d)) return HCIR_ERR_INVALID;
  if (c > kMaxClasses) return HCIR_ERR_UNSUPPORTED;
  const int64_t tiles = hcir_cdiv(n, 32);
  const size_t lds = (size_t)32 * pad32(c) * sizeof(float);
  allow_lds(argmax_kernel, lds);
  hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)(tiles < 2048 ? tiles : 2048)), dim3(kThreads), lds,
                     static_cast<hipStream_t>(stream), x, ldx, n, d, w, b, c, pred, logits);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

size_t hcir_class_moments_workspace_bytes(int64_t n, int32_t d, int32_t c) {
  if (n <= 0 || d <= 0 || c <= 0) return 0;
  const size_t sums = (size_t)class_sum_splits(n, d, c) * c * d * sizeof(double);
  const size_t rows = (size_t)n * sizeof(double);
  return sums > rows ? sums : rows;
}

int hcir_class_sums_f64(const float* x, int64_t n, int32_t d, int64_t ldx, const int64_t* labels, int32_t c,
                        int64_t* counts, double* sums, int32_t* bad, void* workspace, size_t workspace_bytes,
                        void* stream) {
  HCIR_ENTER();
  if (!x || !labels || !counts || !sums || !bad || !workspace) return HCIR_ERR_INVALID;
  if (n <= 0 || d <= 0 || c <= 0 || ldx < d) return HCIR_ERR_INVALID;
  const int splits = class_sum_splits(n, d, c);
  const size_t need = (size_t)splits * c * d * sizeof(double);
  if (workspace_bytes < need) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(workspace, 0, need, st) != hipSuccess) return HCIR_ERR_LAUNCH;
  if (hipMemsetAsync(counts, 0, (size_t)c * sizeof(int64_t), st) != hipSuccess) return HCIR_ERR_LAUNCH;
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(class_sums_kernel, dim3((unsigned)hcir_cdiv(d, 64), (unsigned)splits), dim3(64), 0, st, x, n, d,
                     ldx, labels, c, hcir_cdiv(n, splits), part, reinterpret_cast<unsigned long long*>(counts), bad);
  HCIR_LAUNCH_CHECK();
  const int64_t cd = (int64_t)c * d;
  hipLaunchKernelGGL(class_sums_reduce_kernel, dim3((unsigned)hcir_cdiv(cd, 256)), dim3(256), 0, st, part, splits, cd,
                     sums);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_class_scatter_f64(const float* x, int64_t n, int32_t d, int64_t ldx, const int64_t* labels, int32_t c,
                           const double* means, double* scatter, int32_t* bad, void* workspace,
                           size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!x || !labels || !means || !scatter || !bad || !workspace) return HCIR_ERR_INVALID;
  if (n <= 0 || d <= 0 || c <= 0 || ldx < d) return HCIR_ERR_INVALID;
  if (workspace_bytes < (size_t)n * sizeof(double)) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* row_sq = static_cast<double*>(workspace);
  hipLaunchKernelGGL(row_scatter_kernel, dim3((unsigned)hcir_cdiv(n, kWaves)), dim3(kThreads), 0, st, x, n, d, ldx,
                     labels, c, means, row_sq, bad);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(class_scatter_sum_kernel, dim3((unsigned)hcir_cdiv(c, 64)), dim3(64), 0, st, row_sq, labels, n, c,
                     scatter);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
