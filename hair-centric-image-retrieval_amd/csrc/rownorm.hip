// rownorm.hip — row norms, L2 normalisation and fp32 -> fp16 / bf16 conversion of embedding matrices (the inputs of
// hcir_sim_topk).  See include/hcir.h for the contract.
#include "common.h"
#include <math.h>

namespace {

template <typename T>
__global__ __launch_bounds__(256) void row_invnorm_kernel(const T* __restrict__ x, int64_t n, int d,
                                                          int64_t ldx, float eps,
                                                          float* __restrict__ out) {
  // one wave per row; lane l sums elements 4*(l + 64 j) + e in order, then an
  // xor butterfly 32,16,...,1 (mirrored by oracle/knn_oracle.c: hcir_oracle_row_invnorm).
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const T* p = x + row * ldx;
  float s = 0.f;
  for (int k = 4 * lane; k < d; k += 256) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = (float)p[k + e];
      s = __builtin_fmaf(v, v, s);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) out[row] = 1.0f / fmaxf(sqrtf(s), eps);
}

__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, int64_t n,
                                                           int d, float eps, float* __restrict__ y32,
                                                           _Float16* __restrict__ y16) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* p = x + row * (int64_t)d;
  float s = 0.f;
  for (int k = 4 * lane; k < d; k += 256) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_fmaf(p[k + e], p[k + e], s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  const float nrm = fmaxf(sqrtf(s), eps);
  for (int k = 4 * lane; k < d; k += 256) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = p[k + e] / nrm;
      if (y32) y32[row * (int64_t)d + k + e] = v;
      if (y16) y16[row * (int64_t)d + k + e] = (_Float16)v;
    }
  }
}

template <typename T>
__global__ void convert_kernel(const float* __restrict__ x, int64_t n, T* __restrict__ y) {
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (; i + 3 < n; i += stride) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) y[i + e] = (T)v[e];
  }
  if (i < n && i + 3 >= n)
    for (int64_t j = i; j < n; ++j) y[j] = (T)x[j];
}

}  // namespace

extern "C" {

int hcir_row_invnorm(const void* x, int64_t n, int32_t d, int64_t ldx, int dtype, float eps,
                     float* out, void* stream) {
  HCIR_ENTER();
  if (!x || !out || n <= 0 || d <= 0 || (d & 3) || ldx < d) return HCIR_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)hcir_cdiv(n, 4)), block(256);
  if (dtype == HCIR_F32)
    hipLaunchKernelGGL(row_invnorm_kernel<float>, grid, block, 0, st, (const float*)x, n, d, ldx, eps, out);
  else if (dtype == HCIR_F16)
    hipLaunchKernelGGL(row_invnorm_kernel<_Float16>, grid, block, 0, st, (const _Float16*)x, n, d, ldx, eps, out);
  else if (dtype == HCIR_BF16)
    hipLaunchKernelGGL(row_invnorm_kernel<__bf16>, grid, block, 0, st, (const __bf16*)x, n, d, ldx, eps, out);
  else
    return HCIR_ERR_UNSUPPORTED;
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_l2_normalize(const float* x, int64_t n, int32_t d, float eps, float* y_f32, void* y_f16,
                      void* stream) {
  HCIR_ENTER();
  if (!x || n <= 0 || d <= 0 || (d & 3)) return HCIR_ERR_INVALID;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)hcir_cdiv(n, 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, n, d, eps, y_f32, (_Float16*)y_f16);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_convert_f32(const float* x, int64_t n, int dtype, void* y, void* stream) {
  HCIR_ENTER();
  if (!x || !y || n <= 0) return HCIR_ERR_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t blocks = hcir_cdiv(n, 1024);
  if (blocks > 4096) blocks = 4096;
  if (dtype == HCIR_F16)
    hipLaunchKernelGGL(convert_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, st, x, n, (_Float16*)y);
  else if (dtype == HCIR_BF16)
    hipLaunchKernelGGL(convert_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, st, x, n, (__bf16*)y);
  else
    return HCIR_ERR_UNSUPPORTED;
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
