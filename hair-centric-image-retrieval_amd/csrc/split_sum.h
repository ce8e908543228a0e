// split_sum.h — the second launch of the split weight-gradient kernels (gemm_tn.hip, conv_bwd.hip, stem_train.hip):
// out[i] = sum_s part[s][i], s = 0, 1, 2, ... in that order, so that two runs are bit-identical without float atomics
// (cdna_hip_programming.md Guideline 12).  4 elements per thread: n is a multiple of 4, part and out 16-B aligned.
#pragma once
#include "common.h"

namespace {

// PITCHED: element i = (row, col) of [n / k][k] goes to out[row * ldo + col], added to what is there when `accumulate`
// (k and ldo multiples of 4).  The dense form ignores k, ldo and accumulate and never pays for i / k.
template <bool PITCHED>
__global__ __launch_bounds__(256) void split_sum_kernel(const float* __restrict__ part, int splits, int64_t n, int k,
                                                        float* __restrict__ out, int64_t ldo, int accumulate) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(part + i);
  for (int sp = 1; sp < splits; ++sp) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + (int64_t)sp * n + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += v[e];
  }
  float* o = PITCHED ? out + (i / k) * ldo + (i % k) : out + i;
  if (PITCHED && accumulate) {
    const f32x4 old = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += old[e];
  }
  *reinterpret_cast<f32x4*>(o) = s;
}

// split_sum(...) is the dense form, split_sum<true>(..., k, ldo, accumulate) the pitched one; a file gets only the
// kernel it launches
template <bool PITCHED = false>
void split_sum(const float* part, int splits, int64_t n, float* out, hipStream_t st, int k = 0, int64_t ldo = 0,
               int accumulate = 0) {
  hipLaunchKernelGGL(split_sum_kernel<PITCHED>, dim3((unsigned)hcir_cdiv(n, 1024)), dim3(256), 0, st, part, splits, n,
                     k, out, ldo, accumulate);
}

}  // namespace
