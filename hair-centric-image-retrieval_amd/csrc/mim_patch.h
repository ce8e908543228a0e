// mim_patch.h — what the two masked-patch losses share (mim.hip: SimMIM's L1, mae.hip: MAE's MSE): the image
// descriptor, one target patch staged into LDS in lightly's element order, and the fixed-order workgroup sum.
#pragma once
#include "common.h"

namespace {

constexpr int MIM_THREADS = 256;
constexpr int MIM_L1_BLOCKS = 1024;    // most workgroups of a masked-patch loss
constexpr int MIM_MAX_P = 12288;       // one patch in LDS: 48 KB

inline int64_t mim_l1_blocks(int64_t rows) { return rows < MIM_L1_BLOCKS ? rows : MIM_L1_BLOCKS; }

struct MimImage {
  const float* img;
  int c, h, w, ps, gw, npatch;   // gw: patches per image row; npatch = (h / ps) * gw
};

// Patch `p` (0-based) of image `bi` into LDS in lightly's element order: lds[(py * ps + px) * c + ch].  Image reads are
// the ps contiguous floats of one patch row (64 B at ps = 16), 16 B per lane where ps % 4 == 0; the LDS writes have
// stride c between lanes (conflict-free for c = 3).  The caller has checked p and puts barriers around the call.
__device__ __forceinline__ void mim_stage_patch(const MimImage& im, int64_t bi, int p, float* lds) {
  const int ps = im.ps, gy = p / im.gw, gx = p - gy * im.gw;
  const float* base = im.img + (bi * im.c * im.h + (int64_t)gy * ps) * im.w + gx * ps;
  if ((ps & 3) == 0) {
    const int q4 = ps >> 2, per_c = ps * q4;
    for (int u = threadIdx.x; u < im.c * per_c; u += MIM_THREADS) {
      const int ch = u / per_c, rem = u - ch * per_c, py = rem / q4, px = (rem - py * q4) * 4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + ((int64_t)ch * im.h + py) * im.w + px);
#pragma unroll
      for (int e = 0; e < 4; ++e) lds[(py * ps + px + e) * im.c + ch] = v[e];
    }
  } else {
    const int per_c = ps * ps;
    for (int u = threadIdx.x; u < im.c * per_c; u += MIM_THREADS) {
      const int ch = u / per_c, rem = u - ch * per_c, py = rem / ps, px = rem - py * ps;
      lds[rem * im.c + ch] = base[((int64_t)ch * im.h + py) * im.w + px];
    }
  }
}

// The 64 lanes of a wave are added by the xor butterfly (offsets 32, 16, .., 1), the four waves in order.
__device__ __forceinline__ float mim_block_sum(float v, float* wave_part) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

// loss = (sum of the parts) * inv_n: thread i adds the parts i, i + 256, ... in order, then the same block sum.
__global__ __launch_bounds__(MIM_THREADS) void mim_l1_finish_kernel(const float* __restrict__ part, int nparts,
                                                                      float inv_n, float* __restrict__ loss) {
  __shared__ float wave_part[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += MIM_THREADS) acc += part[i];
  const float tot = mim_block_sum(acc, wave_part);
  if (threadIdx.x == 0) *loss = tot * inv_n;
}

// shape rules shared by the image readers: a status, and the image descriptor filled in
inline int mim_image(const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps, int32_t n, MimImage* im) {
  if (b <= 0 || c <= 0 || h <= 0 || w <= 0 || ps <= 0 || n <= 0 || h % ps || w % ps) return HCIR_ERR_INVALID;
  const int64_t P = (int64_t)c * ps * ps, np = (int64_t)(h / ps) * (w / ps);
  if (P % 8 || P > MIM_MAX_P || np >= (1 << 30) || b * n >= (int64_t)1 << 31) return HCIR_ERR_UNSUPPORTED;
  *im = MimImage{img, c, h, w, ps, w / ps, (int)np};
  return HCIR_OK;
}

}  // namespace
