// bn2d.hip — batch-statistics BatchNorm2d (+ residual, + ReLU) over fp16 NHWC maps, forward and backward: the
// normalisation layers of a ResNet-18 / ResNet-50 body in training (hcir/conv_train.py, the `hip_train_norm` switch).
// Geometry (lanes over the map, chunks, grids, workspace): bn2d_plan.h.
//
// Streaming kernels: every access to a map is 16 bytes per lane, all arithmetic fp32, each stored activation rounded
// to fp16 once.  Reductions go lane -> LDS -> workspace[chunk][C][2] -> one finalize launch, every step in a fixed
// order: no atomics, two calls give the same bits.
//
//   forward   stats     per chunk and channel (mean, M2).  A lane sums d = x - k and d * d with k its own first value
//                       (shifted sums: k is within a few sigma of the mean, so M2 = sum d^2 - (sum d)^2 / n loses a
//                       small constant factor, not mean^2 / var as sum x^2 - (sum x)^2 / n would), lanes and chunks
//                       then merge with Chan's formula
//             finalize  chunks merged per channel -> save_mean, save_rstd, running statistics
//             apply     y = fp16(relu?((x - mean) * (rstd * gamma) + beta (+ resid)))
//   backward  reduce    per chunk and channel (sum g, sum g (x - mean)), g = dy or dy [y > 0]
//             finalize  -> dbeta, dgamma = rstd * sum g (x - mean)
//             apply     dx = fp16(gamma rstd (g - dbeta / M - (x - mean) rstd dgamma / M)), dresid = fp16(g)
#include "bn2d_plan.h"
#include "common.h"

namespace {

struct Geo {   // a lane's place in its workgroup's pass
  int wv;      // vectors of a row per wavefront
  int rpp;     // rows per pass
  int cs;      // vector inside the slab
  int g;       // row inside the pass
};

__device__ __forceinline__ Geo geo(int wv_log2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rpw = 64 >> wv_log2;
  Geo o;
  o.wv = 1 << wv_log2;
  o.rpp = 4 * rpw;
  o.cs = lane & (o.wv - 1);
  o.g = wave * rpw + (lane >> wv_log2);
  return o;
}

// rows r, r + step, ... < r1: U rows' loads are issued before the first is used
template <int U, class Load, class Use>
__device__ __forceinline__ void rows_loop(int64_t r, int64_t r1, int64_t step, Load load, Use use) {
  for (; r + (U - 1) * step < r1; r += U * step) {
    decltype(load(r)) v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = load(r + u * step);
#pragma unroll
    for (int u = 0; u < U; ++u) use(r + u * step, v[u]);
  }
  for (; r < r1; r += step) {
    const auto v = load(r);
    use(r, v);
  }
}

__device__ __forceinline__ void load8(const float* p, float (&o)[8]) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = a[j], o[4 + j] = b[j];
}

// rows of [r0, r1) that row g of a pass visits
__device__ __forceinline__ int rows_of(int64_t len, int g, int rpp) { return g < len ? (int)((len - g + rpp - 1) / rpp) : 0; }

// Chan et al.: (na, ma, Ma) <- merged with (nb, mb, Mb)
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb, ma = mb, Ma = Mb;
    return;
  }
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma += d * f;
  Ma += Mb + d * d * na * f;
  na = n;
}

struct V1 {
  f16x8 a;
};
struct V2 {
  f16x8 a, b;
};
struct V3 {
  f16x8 a, b, c;
};

// ---------------------------------------------------------------- forward
__global__ __launch_bounds__(BN2D_THREADS) void bn2d_stats_kernel(const f16x8* __restrict__ x, int64_t m, int cv,
                                                                  int wv_log2, int slabs, int64_t rows_per_chunk,
                                                                  f32x2* __restrict__ ws) {
  __shared__ f32x2 part[BN2D_THREADS * 8];   // [row of the pass][channel of the slab]
  const Geo t = geo(wv_log2);
  const int slab = blockIdx.x % slabs, chunk = blockIdx.x / slabs;
  const int64_t r0 = chunk * rows_per_chunk, r1 = r0 + rows_per_chunk < m ? r0 + rows_per_chunk : m;
  const f16x8* px = x + slab * t.wv + t.cs;
  float k[8], s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = s[j] = q[j] = 0.f;
  const int64_t first = r0 + t.g;
  if (first < r1) {
    const f16x8 v = px[first * cv];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = (float)v[j];
    rows_loop<4>(
        first + t.rpp, r1, t.rpp, [&](int64_t r) { return V1{px[r * cv]}; },
        [&](int64_t, const V1& v) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = (float)v.a[j] - k[j];
            s[j] += d;
            q[j] = fmaf(d, d, q[j]);
          }
        });
  }
  const int nt = rows_of(r1 - r0, t.g, t.rpp);
  const float inv = nt > 0 ? 1.f / (float)nt : 0.f;
  f32x2* mine = part + (t.g * t.wv + t.cs) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float ds = s[j] * inv;
    mine[j] = f32x2{k[j] + ds, fmaxf(q[j] - s[j] * ds, 0.f)};
  }
  __syncthreads();
  const int nch = t.wv * 8;
  for (int ch = threadIdx.x; ch < nch; ch += BN2D_THREADS) {
    float na = 0.f, ma = 0.f, Ma = 0.f;
    for (int g = 0; g < t.rpp; ++g) {
      const f32x2 b = part[g * nch + ch];
      chan_merge(na, ma, Ma, (float)rows_of(r1 - r0, g, t.rpp), b[0], b[1]);
    }
    ws[(int64_t)chunk * (cv * 8) + slab * nch + ch] = f32x2{ma, Ma};
  }
}

// one wavefront per channel: a lane merges a contiguous run of chunks in order, the lanes then merge in lane order
__global__ __launch_bounds__(BN2D_THREADS) void bn2d_stats_finalize_kernel(
    const f32x2* __restrict__ ws, int chunks, int64_t rows_per_chunk, int64_t m, int c, float eps, float momentum,
    float* __restrict__ running_mean, float* __restrict__ running_var, float* __restrict__ save_mean,
    float* __restrict__ save_rstd) {
  const int lane = threadIdx.x & 63, ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int per = (chunks + 63) / 64, c0 = lane * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  float na = 0.f, ma = 0.f, Ma = 0.f;
  for (int k = c0; k < c1; ++k) {
    const int64_t r0 = k * rows_per_chunk, left = m - r0;
    const f32x2 b = ws[(int64_t)k * c + ch];
    chan_merge(na, ma, Ma, (float)(left < rows_per_chunk ? left : rows_per_chunk), b[0], b[1]);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float nb = __shfl_down(na, o), mb = __shfl_down(ma, o), Mb = __shfl_down(Ma, o);
    if ((lane & (2 * o - 1)) == 0) chan_merge(na, ma, Ma, nb, mb, Mb);
  }
  if (lane == 0) {
    save_mean[ch] = ma;
    save_rstd[ch] = 1.f / sqrtf(Ma / (float)m + eps);
    if (running_mean) running_mean[ch] = (1.f - momentum) * running_mean[ch] + momentum * ma;
    if (running_var) running_var[ch] = (1.f - momentum) * running_var[ch] + momentum * (Ma / (float)(m - 1));
  }
}

template <bool RELU, bool RESID>
__global__ __launch_bounds__(BN2D_THREADS) void bn2d_fwd_apply_kernel(
    const f16x8* __restrict__ x, const f16x8* __restrict__ resid, f16x8* __restrict__ y, int64_t m, int cv,
    int wv_log2, int slabs, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ rstd) {
  const Geo t = geo(wv_log2);
  const int slab = blockIdx.x % slabs, rb = blockIdx.x / slabs, nrb = gridDim.x / slabs;
  const int col = slab * t.wv + t.cs;
  float mu[8], sc[8], be[8], ga[8];
  load8(mean + col * 8, mu);
  load8(rstd + col * 8, sc);
  load8(gamma + col * 8, ga);
  load8(beta + col * 8, be);
#pragma unroll
  for (int j = 0; j < 8; ++j) sc[j] *= ga[j];
  const auto use = [&](int64_t r, f16x8 xv, f16x8 rv) {
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = fmaf((float)xv[j] - mu[j], sc[j], be[j]);
      if (RESID) v += (float)rv[j];
      if (RELU) v = fmaxf(v, 0.f);
      o[j] = (_Float16)v;
    }
    y[r * cv + col] = o;
  };
  const int64_t first = (int64_t)rb * t.rpp + t.g, step = (int64_t)nrb * t.rpp;
  if (RESID)
    rows_loop<4>(
        first, m, step, [&](int64_t r) { return V2{x[r * cv + col], resid[r * cv + col]}; },
        [&](int64_t r, const V2& v) { use(r, v.a, v.b); });
  else
    rows_loop<4>(
        first, m, step, [&](int64_t r) { return V1{x[r * cv + col]}; },
        [&](int64_t r, const V1& v) { use(r, v.a, v.a); });
}

// ---------------------------------------------------------------- backward
template <bool RELU>
__global__ __launch_bounds__(BN2D_THREADS) void bn2d_bwd_reduce_kernel(
    const f16x8* __restrict__ dy, const f16x8* __restrict__ x, const f16x8* __restrict__ yr, int64_t m, int cv,
    int wv_log2, int slabs, int64_t rows_per_chunk, const float* __restrict__ mean, f32x2* __restrict__ ws) {
  __shared__ f32x2 part[BN2D_THREADS * 8];
  const Geo t = geo(wv_log2);
  const int slab = blockIdx.x % slabs, chunk = blockIdx.x / slabs;
  const int64_t r0 = chunk * rows_per_chunk, r1 = r0 + rows_per_chunk < m ? r0 + rows_per_chunk : m;
  const int col = slab * t.wv + t.cs;
  float mu[8], s1[8], s2[8];
  load8(mean + col * 8, mu);
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  const auto use = [&](f16x8 gv, f16x8 xv, f16x8 yv) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = (float)gv[j];
      if (RELU) g = (float)yv[j] > 0.f ? g : 0.f;
      s1[j] += g;
      s2[j] = fmaf(g, (float)xv[j] - mu[j], s2[j]);
    }
  };
  if (RELU)
    rows_loop<2>(
        r0 + t.g, r1, t.rpp, [&](int64_t r) { return V3{dy[r * cv + col], x[r * cv + col], yr[r * cv + col]}; },
        [&](int64_t, const V3& v) { use(v.a, v.b, v.c); });
  else
    rows_loop<2>(
        r0 + t.g, r1, t.rpp, [&](int64_t r) { return V2{dy[r * cv + col], x[r * cv + col]}; },
        [&](int64_t, const V2& v) { use(v.a, v.b, v.a); });
  f32x2* mine = part + (t.g * t.wv + t.cs) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) mine[j] = f32x2{s1[j], s2[j]};
  __syncthreads();
  const int nch = t.wv * 8;
  for (int ch = threadIdx.x; ch < nch; ch += BN2D_THREADS) {
    f32x2 a = part[ch];
    for (int g = 1; g < t.rpp; ++g) a += part[g * nch + ch];   // rows without a lane's visit hold zeros
    ws[(int64_t)chunk * (cv * 8) + slab * nch + ch] = a;
  }
}

__global__ __launch_bounds__(BN2D_THREADS) void bn2d_bwd_finalize_kernel(const f32x2* __restrict__ ws, int chunks, int c,
                                                                         const float* __restrict__ rstd,
                                                                         float* __restrict__ dgamma,
                                                                         float* __restrict__ dbeta) {
  const int lane = threadIdx.x & 63, ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int per = (chunks + 63) / 64, c0 = lane * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  float s1 = 0.f, s2 = 0.f;
  for (int k = c0; k < c1; ++k) {
    const f32x2 b = ws[(int64_t)k * c + ch];
    s1 += b[0];
    s2 += b[1];
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {   // lanes past the last chunk add zeros
    s1 += __shfl_down(s1, o);
    s2 += __shfl_down(s2, o);
  }
  if (lane == 0) {
    dbeta[ch] = s1;
    dgamma[ch] = s2 * rstd[ch];
  }
}

template <bool RELU, bool DRESID>
__global__ __launch_bounds__(BN2D_THREADS) void bn2d_bwd_apply_kernel(
    const f16x8* __restrict__ dy, const f16x8* __restrict__ x, const f16x8* __restrict__ yr, f16x8* __restrict__ dx,
    f16x8* __restrict__ dresid, int64_t m, int cv, int wv_log2, int slabs, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ dgamma,
    const float* __restrict__ dbeta) {
  const Geo t = geo(wv_log2);
  const int slab = blockIdx.x % slabs, rb = blockIdx.x / slabs, nrb = gridDim.x / slabs;
  const int col = slab * t.wv + t.cs;
  float mu[8], a[8], b[8], cc[8], rs[8];
  load8(mean + col * 8, mu);
  load8(gamma + col * 8, a);
  load8(dbeta + col * 8, b);
  load8(dgamma + col * 8, cc);
  load8(rstd + col * 8, rs);
  const float inv_m = 1.f / (float)m;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] *= rs[j];             // gamma rstd
    b[j] *= inv_m;             // dbeta / M
    cc[j] *= rs[j] * inv_m;    // rstd dgamma / M
  }
  const auto use = [&](int64_t r, f16x8 gv, f16x8 xv, f16x8 yv) {
    f16x8 o, og;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      _Float16 gh = gv[j];
      if (RELU) gh = (float)yv[j] > 0.f ? gh : (_Float16)0.f;
      og[j] = gh;
      const float g = (float)gh;
      o[j] = (_Float16)(a[j] * (g - b[j] - ((float)xv[j] - mu[j]) * cc[j]));
    }
    dx[r * cv + col] = o;
    if (DRESID) dresid[r * cv + col] = og;
  };
  const int64_t first = (int64_t)rb * t.rpp + t.g, step = (int64_t)nrb * t.rpp;
  if (RELU)
    rows_loop<2>(
        first, m, step, [&](int64_t r) { return V3{dy[r * cv + col], x[r * cv + col], yr[r * cv + col]}; },
        [&](int64_t r, const V3& v) { use(r, v.a, v.b, v.c); });
  else
    rows_loop<2>(
        first, m, step, [&](int64_t r) { return V2{dy[r * cv + col], x[r * cv + col]}; },
        [&](int64_t r, const V2& v) { use(r, v.a, v.b, v.a); });
}

}  // namespace

extern "C" size_t hcir_bn2d_workspace_bytes(int64_t m, int32_t c) {
  Bn2dPlan p;
  return bn2d_plan(m, c, &p) == HCIR_OK ? bn2d_workspace_bytes(p, c) : 0;
}

// HOST: the number of row chunks the reductions run the shape with, or the status the entry points return for it.
extern "C" int32_t hcir_bn2d_chunks(int64_t m, int32_t c) {
  Bn2dPlan p;
  const int st = bn2d_plan(m, c, &p);
  return st == HCIR_OK ? p.chunks : st;
}

extern "C" int hcir_bn2d_fwd_nhwc_f16(const void* x, int64_t m, int32_t c, const float* gamma, const float* beta,
                                      float eps, float momentum, const void* resid, int relu, float* running_mean,
                                      float* running_var, float* save_mean, float* save_rstd, void* y, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  Bn2dPlan p;
  const int st = bn2d_plan(m, c, &p);   // host arithmetic only: no device needed
  if (st != HCIR_OK) return st;
  if (!x || !gamma || !beta || !save_mean || !save_rstd || !y) return HCIR_ERR_INVALID;
  if (!workspace || workspace_bytes < bn2d_workspace_bytes(p, c)) return HCIR_ERR_WORKSPACE;
  HCIR_ENTER();
  hipStream_t hs = (hipStream_t)stream;
  const f16x8 *px = (const f16x8*)x, *pr = (const f16x8*)resid;
  f16x8* py = (f16x8*)y;
  hipLaunchKernelGGL(bn2d_stats_kernel, dim3((unsigned)(p.chunks * p.slabs)), dim3(BN2D_THREADS), 0, hs, px, m, p.cv,
                     p.wv_log2, p.slabs, p.rows_per_chunk, (f32x2*)workspace);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn2d_stats_finalize_kernel, dim3((unsigned)(c / 4)), dim3(BN2D_THREADS), 0, hs,
                     (const f32x2*)workspace, p.chunks, p.rows_per_chunk, m, c, eps, momentum, running_mean,
                     running_var, save_mean, save_rstd);
  HCIR_LAUNCH_CHECK();
  const dim3 grid((unsigned)(p.apply_blocks * p.slabs)), block(BN2D_THREADS);
#define BN2D_FWD(RELU, RESID)                                                                                       \
  hipLaunchKernelGGL((bn2d_fwd_apply_kernel<RELU, RESID>), grid, block, 0, hs, px, pr, py, m, p.cv, p.wv_log2, p.slabs, \
                     gamma, beta, (const float*)save_mean, (const float*)save_rstd)
  if (relu) {
    if (resid) BN2D_FWD(true, true); else BN2D_FWD(true, false);
  } else {
    if (resid) BN2D_FWD(false, true); else BN2D_FWD(false, false);
  }
#undef BN2D_FWD
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

// The forward's first two launches alone: the stem normalises inside its pooling kernel (stem_train.hip).
extern "C" int hcir_bn2d_stats_nhwc_f16(const void* x, int64_t m, int32_t c, float eps, float momentum,
                                        float* running_mean, float* running_var, float* save_mean, float* save_rstd,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  Bn2dPlan p;
  const int st = bn2d_plan(m, c, &p);
  if (st != HCIR_OK) return st;
  if (!x || !save_mean || !save_rstd) return HCIR_ERR_INVALID;
  if (!workspace || workspace_bytes < bn2d_workspace_bytes(p, c)) return HCIR_ERR_WORKSPACE;
  HCIR_ENTER();
  hipStream_t hs = (hipStream_t)stream;
  hipLaunchKernelGGL(bn2d_stats_kernel, dim3((unsigned)(p.chunks * p.slabs)), dim3(BN2D_THREADS), 0, hs,
                     (const f16x8*)x, m, p.cv, p.wv_log2, p.slabs, p.rows_per_chunk, (f32x2*)workspace);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn2d_stats_finalize_kernel, dim3((unsigned)(c / 4)), dim3(BN2D_THREADS), 0, hs,
                     (const f32x2*)workspace, p.chunks, p.rows_per_chunk, m, c, eps, momentum, running_mean,
                     running_var, save_mean, save_rstd);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_bn2d_bwd_nhwc_f16(const void* dy, const void* x, const void* y_relu, int64_t m, int32_t c,
                                      const float* gamma, const float* save_mean, const float* save_rstd, void* dx,
                                      void* dresid, float* dgamma, float* dbeta, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  Bn2dPlan p;
  const int st = bn2d_plan(m, c, &p);
  if (st != HCIR_OK) return st;
  if (!dy || !x || !gamma || !save_mean || !save_rstd || !dx || !dgamma || !dbeta) return HCIR_ERR_INVALID;
  if (!workspace || workspace_bytes < bn2d_workspace_bytes(p, c)) return HCIR_ERR_WORKSPACE;
  HCIR_ENTER();
  hipStream_t hs = (hipStream_t)stream;
  const f16x8 *pg = (const f16x8*)dy, *px = (const f16x8*)x, *py = (const f16x8*)y_relu;
  const dim3 rgrid((unsigned)(p.chunks * p.slabs)), grid((unsigned)(p.apply_blocks * p.slabs)), block(BN2D_THREADS);
  if (y_relu)
    hipLaunchKernelGGL(bn2d_bwd_reduce_kernel<true>, rgrid, block, 0, hs, pg, px, py, m, p.cv, p.wv_log2, p.slabs,
                       p.rows_per_chunk, save_mean, (f32x2*)workspace);
  else
    hipLaunchKernelGGL(bn2d_bwd_reduce_kernel<false>, rgrid, block, 0, hs, pg, px, py, m, p.cv, p.wv_log2, p.slabs,
                       p.rows_per_chunk, save_mean, (f32x2*)workspace);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn2d_bwd_finalize_kernel, dim3((unsigned)(c / 4)), block, 0, hs, (const f32x2*)workspace,
                     p.chunks, c, save_rstd, dgamma, dbeta);
  HCIR_LAUNCH_CHECK();
#define BN2D_BWD(RELU, DRESID)                                                                                   \
  hipLaunchKernelGGL((bn2d_bwd_apply_kernel<RELU, DRESID>), grid, block, 0, hs, pg, px, py, (f16x8*)dx,          \
                     (f16x8*)dresid, m, p.cv, p.wv_log2, p.slabs, gamma, save_mean, save_rstd, (const float*)dgamma, \
                     (const float*)dbeta)
  if (y_relu) {
    if (dresid) BN2D_BWD(true, true); else BN2D_BWD(true, false);
  } else {
    if (dresid) BN2D_BWD(false, true); else BN2D_BWD(false, false);
  }
#undef BN2D_BWD
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}
