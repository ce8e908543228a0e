// optim.hip — the optimizer tail of the HSimCLR step as three launches over a chunk table, no host read.
//
// Replaces the last five lines of the reference's batch loop (HP/src/pretrain_engine.py:745-749) with the optimizer
// of HP/utils/utils.py:59-71 (torch.optim.Adam, coupled L2 weight decay, two parameter groups):
//     scaler.scale(total).backward(); scaler.unscale_(opt); clip_grad_norm_(params, 1.0); scaler.step(opt);
//     scaler.update()
// which torch runs as about a dozen multi_tensor_apply passes plus one host read of found_inf.
//
//   hcir_grad_sumsq      per chunk: sum of (g * inv_scale)^2 and a "some element is non-finite" flag, plain stores
//   hcir_optim_finalize  one workgroup: fp64 sum of the partials in a fixed order, total_norm, clip coefficient,
//                        found_inf, GradScaler.update, per-parameter step / step_size / bc2_sqrt
//   hcir_adam_step       per chunk: p, exp_avg, exp_avg_sq updated in place; nothing is written on found_inf
//
// The chunk table is the one of momentum.hip with more columns: chunk c covers counts[c] (<= 65 536) consecutive
// floats of ONE parameter at p/g/m/v_ptrs[c]; one workgroup of 256 lanes per chunk, 16 B per lane per access where
// all pointers of the chunk are 16-byte aligned, a 4-byte path otherwise, tail elements on the 4-byte path.
// HBM-bound: 4 B per parameter for the norm pass, 16 B read + 12 B written for the Adam pass.
// No atomics: every output has one writer and every sum a fixed order, so two calls on the same inputs give the
// same bits.
//
// FP CONTRACTION IS OFF in every kernel of this file (HIP contracts a*b + c into an FMA by default).  Each product
// and each sum below is one IEEE fp32 operation, rounded on its own, in exactly the order written; division and
// sqrtf are correctly rounded (hipcc's default) and fp32 denormals are kept (gfx9 default).  The per-element error
// bound and the numpy emulation of tests/_optim_ref.py restate this order operation by operation.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGroups = 16;

struct GroupArgs {
  int32_t n;
  int32_t end[kMaxGroups];  // participating parameters [end[g-1], end[g]) belong to group g
  double lr[kMaxGroups];
};

// ctl[0] = total_norm, ctl[1] = c = inv_scale * clip_coef, ctl[2] = found_inf (0 or 1), ctl[3] = clip_coef
enum { CTL_NORM = 0, CTL_C = 1, CTL_FOUND_INF = 2, CTL_CLIP = 3 };

__device__ __forceinline__ float inv_scale_of(const float* scale) {
  // torch.amp.GradScaler: self._scale.double().reciprocal().float()
  return scale ? (float)(1.0 / (double)scale[0]) : 1.0f;
}

__device__ __forceinline__ bool non_finite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const uint64_t* __restrict__ g_ptrs,
                                                              const int64_t* __restrict__ count,
                                                              const float* __restrict__ scale,
                                                              float* __restrict__ partial,
                                                              int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  __shared__ float red[kThreads / HCIR_WAVE];
  __shared__ int bad_any[kThreads / HCIR_WAVE];
  const int64_t c = blockIdx.x;
  const float* __restrict__ g = reinterpret_cast<const float*>(g_ptrs[c]);
  const int64_t n = count[c];
  const float inv = inv_scale_of(scale);
  const bool vec = (g_ptrs[c] & 15) == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  bool bad = false;
  // vector path: accumulator k of lane t takes elements 4 * (t + 256 j) + k, j ascending
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = threadIdx.x; i < n4; i += kThreads) {
    const f32x4 a = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float u = a[k] * inv;
      bad |= non_finite(u);
      acc[k] = acc[k] + u * u;
    }
  }
  float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  // 4-byte path (the whole chunk when unaligned, else its last n % 4 elements): lane t takes t + 256 j, j ascending
  for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += kThreads) {
    const float u = g[i] * inv;
    bad |= non_finite(u);
    s = s + u * u;
  }
  s = wave_sum(s);  // xor butterfly, offsets 32, 16, ..., 1
  const int w = threadIdx.x / HCIR_WAVE;
  const bool wave_bad = __any(bad);
  if (threadIdx.x % HCIR_WAVE == 0) {
    red[w] = s;
    bad_any[w] = wave_bad ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[c] = ((red[0] + red[1]) + red[2]) + red[3];
    flag[c] = bad_any[0] | bad_any[1] | bad_any[2] | bad_any[3];
  }
}

__global__ __launch_bounds__(kThreads) void optim_finalize_kernel(
    const float* __restrict__ partial, const int32_t* __restrict__ flag, int64_t n_chunks, float* __restrict__ scale,
    int32_t* __restrict__ tracker, float growth_factor, float backoff_factor, int32_t growth_interval, int use_clip,
    double max_norm, GroupArgs groups, double beta1, double beta2, const int32_t* __restrict__ part_idx,
    int32_t n_part, float* __restrict__ steps, float* __restrict__ step_size, float* __restrict__ bc2_sqrt,
    float* __restrict__ ctl) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads];
  __shared__ int bad_any[kThreads];
  __shared__ int found_sh;
  // lane t adds partials t, t + 256, ... in ascending order; then a halving tree over the 256 lanes
  double s = 0.0;
  int bad = 0;
  for (int64_t i = threadIdx.x; i < n_chunks; i += kThreads) {
    s = s + (double)partial[i];
    bad |= flag[i];
  }
  red[threadIdx.x] = s;
  bad_any[threadIdx.x] = bad;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
      bad_any[threadIdx.x] |= bad_any[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // a scaler decides whether the step is taken (GradScaler.step); without one the step is unconditional, as
    // clip_grad_norm_ + opt.step() are
    const int found = (scale != nullptr && bad_any[0]) ? 1 : 0;
    const double norm = sqrt(red[0]);
    double coef = 1.0;
    if (use_clip) {
      coef = max_norm / (norm + 1e-6);
      if (coef > 1.0) coef = 1.0;  // a NaN stays a NaN, as torch.clamp(max=1.0) keeps it
    }
    const double inv = scale ? 1.0 / (double)scale[0] : 1.0;
    ctl[CTL_NORM] = (float)norm;
    ctl[CTL_C] = (float)(inv * coef);
    ctl[CTL_FOUND_INF] = (float)found;
    ctl[CTL_CLIP] = (float)coef;
    if (scale) {  // torch.amp.GradScaler.update (_amp_update_scale_)
      if (found) {
        scale[0] = scale[0] * backoff_factor;
        tracker[0] = 0;
      } else {
        const int32_t ok = tracker[0] + 1;
        if (ok == growth_interval) {
          const float grown = scale[0] * growth_factor;
          if (!non_finite(grown)) scale[0] = grown;
          tracker[0] = 0;
        } else {
          tracker[0] = ok;
        }
      }
    }
    found_sh = found;
  }
  __syncthreads();
  if (found_sh) return;
  for (int32_t j = threadIdx.x; j < n_part; j += kThreads) {
    int gi = 0;
    while (gi + 1 < groups.n && j >= groups.end[gi]) ++gi;
    const int32_t i = part_idx[j];
    const float t = steps[i] + 1.0f;
    steps[i] = t;
    const double bc1 = 1.0 - pow(beta1, (double)t);
    const double bc2 = 1.0 - pow(beta2, (double)t);
    step_size[i] = (float)(groups.lr[gi] / bc1);
    bc2_sqrt[i] = (float)sqrt(bc2);
  }
}

struct AdamScalars {
  float c, beta2, om1, om2, eps;
};

__device__ __forceinline__ void adam_element(float& p, float grad, float& m, float& v, float wd, float ss, float bc2,
                                             const AdamScalars& k) {
#pragma clang fp contract(off)
  const float g = grad * k.c + wd * p;  // coupled L2: torch.optim.Adam's grad.add(param, alpha=weight_decay)
  m = m + (g - m) * k.om1;              // exp_avg.lerp_(grad, 1 - beta1)
  v = v * k.beta2 + k.om2 * (g * g);    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / bc2 + k.eps;
  p = p - ss * (m / denom);             // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(
    const uint64_t* __restrict__ p_ptrs, const uint64_t* __restrict__ g_ptrs, const uint64_t* __restrict__ m_ptrs,
    const uint64_t* __restrict__ v_ptrs, const int64_t* __restrict__ count, const int32_t* __restrict__ pidx,
    const float* __restrict__ wds, const float* __restrict__ step_size, const float* __restrict__ bc2_sqrt,
    const float* __restrict__ ctl, float beta2, float om1, float om2, float eps) {
#pragma clang fp contract(off)
  if (ctl[CTL_FOUND_INF] != 0.0f) return;  // GradScaler.step skips optimizer.step(): nothing is written
  const int64_t c = blockIdx.x;
  float* __restrict__ p = reinterpret_cast<float*>(p_ptrs[c]);
  const float* __restrict__ g = reinterpret_cast<const float*>(g_ptrs[c]);
  float* __restrict__ m = reinterpret_cast<float*>(m_ptrs[c]);
  float* __restrict__ v = reinterpret_cast<float*>(v_ptrs[c]);
  const int64_t n = count[c];
  const int32_t i_p = pidx[c];
  const float wd = wds[c], ss = step_size[i_p], bc2 = bc2_sqrt[i_p];
  const AdamScalars k = {ctl[CTL_C], beta2, om1, om2, eps};
  const bool vec = ((p_ptrs[c] | g_ptrs[c] | m_ptrs[c] | v_ptrs[c]) & 15) == 0;
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = threadIdx.x; i < n4; i += kThreads) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pp[e], me = mm[e], ve = vv[e];
      adam_element(pe, gg[e], me, ve, wd, ss, bc2, k);
      pp[e] = pe, mm[e] = me, vv[e] = ve;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += kThreads) adam_element(p[i], g[i], m[i], v[i], wd, ss, bc2, k);
}

}  // namespace

extern "C" int hcir_grad_sumsq(const uint64_t* g_ptrs, const int64_t* counts, int64_t n_chunks, const float* scale,
                               float* partial, int32_t* flags, void* stream) {
  HCIR_ENTER();
  if (!g_ptrs || !counts || !partial || !flags || n_chunks <= 0 || n_chunks > 0x7fffffff) return HCIR_ERR_INVALID;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     g_ptrs, counts, scale, partial, flags);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_optim_finalize(const float* partial, const int32_t* flags, int64_t n_chunks, float* scale,
                                   int32_t* growth_tracker, float growth_factor, float backoff_factor,
                                   int32_t growth_interval, int use_clip, double max_norm, const int32_t* group_end,
                                   const double* group_lr, int32_t n_groups, double beta1, double beta2,
                                   const int32_t* part_idx, int32_t n_part, float* steps, float* step_size,
                                   float* bc2_sqrt, float* ctl, void* stream) {
  HCIR_ENTER();
  if (n_chunks < 0 || n_chunks > 0x7fffffff || (n_chunks > 0 && (!partial || !flags))) return HCIR_ERR_INVALID;
  if ((scale == nullptr) != (growth_tracker == nullptr)) return HCIR_ERR_INVALID;
  if (scale && growth_interval <= 0) return HCIR_ERR_INVALID;
  if (!group_end || !group_lr || n_groups <= 0 || !part_idx || n_part <= 0 || !steps || !step_size || !bc2_sqrt ||
      !ctl)
    return HCIR_ERR_INVALID;
  if (n_groups > kMaxGroups) return HCIR_ERR_UNSUPPORTED;
  GroupArgs ga;
  ga.n = n_groups;
  int32_t prev = 0;
  for (int i = 0; i < kMaxGroups; ++i) {
    ga.end[i] = i < n_groups ? group_end[i] : n_part;
    ga.lr[i] = i < n_groups ? group_lr[i] : 0.0;
    if (i < n_groups && (group_end[i] < prev || group_end[i] > n_part)) return HCIR_ERR_INVALID;
    if (i < n_groups) prev = group_end[i];
  }
  if (prev != n_part) return HCIR_ERR_INVALID;
  hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), partial,
                     flags, n_chunks, scale, growth_tracker, growth_factor, backoff_factor, growth_interval, use_clip,
                     max_norm, ga, beta1, beta2, part_idx, n_part, steps, step_size, bc2_sqrt, ctl);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_adam_step(const uint64_t* p_ptrs, const uint64_t* g_ptrs, const uint64_t* m_ptrs,
                              const uint64_t* v_ptrs, const int64_t* counts, const int32_t* param_idx,
                              const float* weight_decay, int64_t n_chunks, const float* step_size,
                              const float* bc2_sqrt, const float* ctl, float beta2, float one_minus_beta1,
                              float one_minus_beta2, float eps, void* stream) {
  HCIR_ENTER();
  if (!p_ptrs || !g_ptrs || !m_ptrs || !v_ptrs || !counts || !param_idx || !weight_decay || !step_size ||
      !bc2_sqrt || !ctl || n_chunks <= 0 || n_chunks > 0x7fffffff)
    return HCIR_ERR_INVALID;
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     p_ptrs, g_ptrs, m_ptrs, v_ptrs, counts, param_idx, weight_decay, step_size, bc2_sqrt, ctl, beta2,
                     one_minus_beta1, one_minus_beta2, eps);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}
