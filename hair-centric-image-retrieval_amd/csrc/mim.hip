// mim.hip — the SimMIM-specific passes around the ViT walk (HairPretraining/src/backbone.py:549-601,
// src/pretrain_engine.py:514-532; lightly's MaskedVisionTransformerTorchvision.encode / mask_at_index / patchify).
//
//   hcir_mim_mask_tokens     masked rows of the token buffer <- mask_token + pos_mult * pos[token]
//   hcir_mim_mask_bwd        its backward: g_mask_token = column sums over the masked rows of the stream gradient, and
//                            the fp16 patch-row operand of the conv_proj weight gradient with the masked rows zeroed
//   hcir_mim_patch_targets   rows patchify(img)[idx - 1], element order (py, px, c)
//   hcir_mim_l1_fwd          mean |pred - target| and sign(pred - target), the target read straight from the image
// All four are memory-bound passes.  No float atomics: partial sums go to a caller-provided workspace and are added in
// a fixed order, so two runs give the same bits.  Every patch index read from device memory is range-checked before it
// addresses the image; a row whose index is outside [1, t) is written as zero and adds nothing.
#include "mim_patch.h"   // the image descriptor, the staged target patch, the workgroup sum (shared with mae.hip)
#include "split_sum.h"

namespace {

constexpr int MIM_BWD_ROWS = 64;       // fewest rows of one workgroup share of hcir_mim_mask_bwd
constexpr int MIM_BWD_CHUNKS = 256;    // most shares

__host__ __device__ inline int64_t mim_bwd_chunks(int64_t m) {
  const int64_t c = (m + MIM_BWD_ROWS - 1) / MIM_BWD_ROWS;
  return c < 1 ? 1 : (c > MIM_BWD_CHUNKS ? MIM_BWD_CHUNKS : c);
}

// ---------------------------------------------------------------- mask tokens
template <typename T>
__global__ __launch_bounds__(MIM_THREADS) void mim_mask_tokens_kernel(T* __restrict__ tok,
                                                                      const uint8_t* __restrict__ mask, int64_t m, int t,
                                                                      int d, const float* __restrict__ mask_token,
                                                                      const float* __restrict__ pos, float pos_mult) {
  const int groups = d >> 3;
  const int64_t i = (int64_t)blockIdx.x * MIM_THREADS + threadIdx.x;
  if (i >= m * groups) return;
  const int64_t row = i / groups;
  if (!mask[row]) return;
  const int col = (int)(i - row * groups) * 8;
  const int tk = (int)(row % t);
  float v[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x4 mt = *reinterpret_cast<const f32x4*>(mask_token + col + 4 * h);
    const f32x4 p = *reinterpret_cast<const f32x4*>(pos + (int64_t)tk * d + col + 4 * h);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * h + e] = fmaf(pos_mult, p[e], mt[e]);   // one fp32 rounding
  }
  T* o = tok + row * d + col;
  if constexpr (sizeof(T) == 2) {
    f16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (_Float16)v[e];
    *reinterpret_cast<f16x8*>(o) = r;
  } else {
    *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(o + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  }
}

// ---------------------------------------------------------------- mask backward
// Workgroup (x, y): the 256 columns from 256 x, the rows [y rows_per, (y + 1) rows_per).  Thread (cx = tid % 32,
// ry = tid / 32) owns 8 columns and walks the rows ry, ry + 8, ... of the share in order; the 8 row lanes are then added
// in order ry = 0..7 and the share's sums go to part[y][d].  split_sum adds the shares in order.
__global__ __launch_bounds__(MIM_THREADS) void mim_mask_bwd_kernel(const float* __restrict__ dtok,
                                                                   const uint8_t* __restrict__ mask, int64_t m, int t,
                                                                   int d, int64_t rows_per,
                                                                   _Float16* __restrict__ dpatch,
                                                                   float* __restrict__ part) {
  __shared__ float red[8][256 + 8];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int col = (blockIdx.x * 32 + cx) * 8;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = r0 + rows_per < m ? r0 + rows_per : m;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (col < d) {
    for (int64_t r = r0 + ry; r < r1; r += 8) {
      const int64_t bi = r / t;
      const int tk = (int)(r - bi * t);
      const bool mk = mask[r] != 0;
      if (!mk && tk == 0) continue;               // an unmasked class token: no patch row, no sum
      const f32x4 a = *reinterpret_cast<const f32x4*>(dtok + r * d + col);
      const f32x4 b = *reinterpret_cast<const f32x4*>(dtok + r * d + col + 4);
      if (mk) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[e] += a[e];
          acc[4 + e] += b[e];
        }
      }
      if (tk) {
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = mk ? (_Float16)0.f : (_Float16)a[e];
          o[4 + e] = mk ? (_Float16)0.f : (_Float16)b[e];
        }
        *reinterpret_cast<f16x8*>(dpatch + (bi * (t - 1) + tk - 1) * d + col) = o;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ry][cx * 8 + e] = acc[e];
  __syncthreads();
  if (ry == 0 && col < d) {
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] = red[0][cx * 8 + e];
#pragma unroll
      for (int y = 1; y < 8; ++y) s[e] += red[y][cx * 8 + e];
    }
    float* o = part + (int64_t)blockIdx.y * d + col;
    *reinterpret_cast<f32x4*>(o) = (f32x4){s[0], s[1], s[2], s[3]};
    *reinterpret_cast<f32x4*>(o + 4) = (f32x4){s[4], s[5], s[6], s[7]};
  }
}

// ---------------------------------------------------------------- patches of the image
__global__ __launch_bounds__(MIM_THREADS) void mim_patch_targets_kernel(MimImage im, const int64_t* __restrict__ idx,
                                                                        int n, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int64_t row = blockIdx.x;
  const int P = im.c * im.ps * im.ps;
  const int64_t tkn = idx[row];
  const bool ok = tkn >= 1 && tkn <= im.npatch;     // the same value in every thread: the branch is uniform
  if (ok) mim_stage_patch(im, row / n, (int)(tkn - 1), lds);
  __syncthreads();
  float* o = out + row * P;
  for (int e = threadIdx.x * 4; e < P; e += MIM_THREADS * 4)
    *reinterpret_cast<f32x4*>(o + e) = ok ? *reinterpret_cast<const f32x4*>(lds + e) : (f32x4){0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------- masked-patch L1
// Workgroup w takes the rows [w share, (w + 1) share).  A thread adds |pred - target| of its 8-element groups
// (groups tid, tid + 256, ... of each row, elements in order, rows in order) into one fp32 accumulator; the 64 lanes of
// a wave are added by the xor butterfly (offsets 32, 16, .., 1), the four waves in order; part[w] gets the sum.
__global__ __launch_bounds__(MIM_THREADS) void mim_l1_kernel(const _Float16* __restrict__ pred, MimImage im,
                                                             const int64_t* __restrict__ idx, int n, int64_t rows,
                                                             int64_t share, _Float16* __restrict__ sgn,
                                                             float* __restrict__ part) {
  extern __shared__ float lds[];
  __shared__ float wave_part[4];
  const int P = im.c * im.ps * im.ps;
  const int64_t r0 = (int64_t)blockIdx.x * share;
  const int64_t r1 = r0 + share < rows ? r0 + share : rows;
  float acc = 0.f;
  for (int64_t row = r0; row < r1; ++row) {
    const int64_t tkn = idx[row];
    const bool ok = tkn >= 1 && tkn <= im.npatch;   // uniform
    __syncthreads();                                // the previous row's reads of lds are done
    if (ok) mim_stage_patch(im, row / n, (int)(tkn - 1), lds);
    __syncthreads();
    for (int e = threadIdx.x * 8; e < P; e += MIM_THREADS * 8) {
      f16x8 s;
      if (ok) {
        const f16x8 pv = *reinterpret_cast<const f16x8*>(pred + row * P + e);
        const f32x4 ta = *reinterpret_cast<const f32x4*>(lds + e), tb = *reinterpret_cast<const f32x4*>(lds + e + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float df = (float)pv[j] - (j < 4 ? ta[j & 3] : tb[j & 3]);
          acc += fabsf(df);
          s[j] = (_Float16)((df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = (_Float16)0.f;
      }
      *reinterpret_cast<f16x8*>(sgn + row * P + e) = s;
    }
  }
  const float tot = mim_block_sum(acc, wave_part);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

}  // namespace

extern "C" {

int hcir_mim_mask_tokens(void* tok, int tok_dtype, int64_t b, int32_t t, int32_t d, const uint8_t* mask,
                         const float* mask_token, const float* pos, float pos_mult, void* stream) {
  HCIR_ENTER();
  if (b <= 0 || t <= 0 || d <= 0) return HCIR_ERR_INVALID;
  if (d % 8 || (tok_dtype != HCIR_F32 && tok_dtype != HCIR_F16)) return HCIR_ERR_UNSUPPORTED;
  if (!tok || !mask || !mask_token || !pos) return HCIR_ERR_INVALID;
  const int64_t m = b * t;
  const dim3 grid((unsigned)hcir_cdiv(m * (d / 8), MIM_THREADS));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (tok_dtype == HCIR_F16)
    hipLaunchKernelGGL(mim_mask_tokens_kernel<_Float16>, grid, dim3(MIM_THREADS), 0, st, static_cast<_Float16*>(tok),
                       mask, m, t, d, mask_token, pos, pos_mult);
  else
    hipLaunchKernelGGL(mim_mask_tokens_kernel<float>, grid, dim3(MIM_THREADS), 0, st, static_cast<float*>(tok), mask, m,
                       t, d, mask_token, pos, pos_mult);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

size_t hcir_mim_mask_bwd_workspace_bytes(int64_t b, int32_t t, int32_t d) {
  if (b <= 0 || t <= 0 || d <= 0 || d % 8) return 0;
  return (size_t)mim_bwd_chunks(b * t) * d * sizeof(float);
}

int hcir_mim_mask_bwd(const float* dtok, int64_t b, int32_t t, int32_t d, const uint8_t* mask, float* g_mask_token,
                      void* dpatch, void* workspace, size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (b <= 0 || t <= 0 || d <= 0) return HCIR_ERR_INVALID;
  if (d % 8) return HCIR_ERR_UNSUPPORTED;
  if (!dtok || !mask || !g_mask_token || (!dpatch && t > 1)) return HCIR_ERR_INVALID;
  const int64_t m = b * t, chunks = mim_bwd_chunks(m);
  if (!workspace || workspace_bytes < (size_t)chunks * d * sizeof(float)) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mim_mask_bwd_kernel, dim3((unsigned)hcir_cdiv(d, 256), (unsigned)chunks), dim3(MIM_THREADS), 0, st,
                     dtok, mask, m, t, d, hcir_cdiv(m, chunks), static_cast<_Float16*>(dpatch),
                     static_cast<float*>(workspace));
  HCIR_LAUNCH_CHECK();
  split_sum(static_cast<const float*>(workspace), (int)chunks, d, g_mask_token, st);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_mim_patch_targets(const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps,
                           const int64_t* idx, int32_t n, float* out, void* stream) {
  HCIR_ENTER();
  MimImage im;
  const int rc = mim_image(img, b, c, h, w, ps, n, &im);
  if (rc != HCIR_OK) return rc;
  if (!img || !idx || !out) return HCIR_ERR_INVALID;
  const size_t lds = (size_t)c * ps * ps * sizeof(float);
  hipLaunchKernelGGL(mim_patch_targets_kernel, dim3((unsigned)(b * n)), dim3(MIM_THREADS), lds,
                     static_cast<hipStream_t>(stream), im, idx, n, out);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

size_t hcir_mim_l1_workspace_bytes(int64_t rows) {
  return rows <= 0 ? 0 : (size_t)mim_l1_blocks(rows) * sizeof(float);
}

int hcir_mim_l1_fwd(const void* pred, const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps,
                    const int64_t* idx, int32_t n, float* loss, void* sgn, void* workspace, size_t workspace_bytes,
                    void* stream) {
  HCIR_ENTER();
  MimImage im;
  const int rc = mim_image(img, b, c, h, w, ps, n, &im);
  if (rc != HCIR_OK) return rc;
  if (!pred || !img || !idx || !loss || !sgn) return HCIR_ERR_INVALID;
  const int64_t rows = b * n, blocks = mim_l1_blocks(rows);
  if (!workspace || workspace_bytes < (size_t)blocks * sizeof(float)) return HCIR_ERR_WORKSPACE;
  const int64_t P = (int64_t)c * ps * ps;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mim_l1_kernel, dim3((unsigned)blocks), dim3(MIM_THREADS), (size_t)P * sizeof(float), st,
                     static_cast<const _Float16*>(pred), im, idx, n, rows, hcir_cdiv(rows, blocks),
                     static_cast<_Float16*>(sgn), static_cast<float*>(workspace));
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(mim_l1_finish_kernel, dim3(1), dim3(MIM_THREADS), 0, st, static_cast<const float*>(workspace),
                     (int)blocks, 1.0f / (float)(rows * P), loss);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
