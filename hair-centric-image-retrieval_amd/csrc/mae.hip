// mae.hip — the MAE-specific passes around the two block stacks of hcir.vit_train.MaeTrainer
// (HairPretraining/src/backbone.py:462-525, src/pretrain_engine.py:323-338; lightly's MaskedVisionTransformerTIMM.encode
// with idx_keep, MAE.forward_decoder's repeat_token / set_at_index / get_at_index, MAEDecoderTIMM.decode's position add).
//
//   hcir_mae_gather_rows        compact[i k + j] = tok[i][idx[i][j]]  (fp16 rows; the kept rows in front of the encoder
//                               blocks, the masked rows in front of decoder_norm), pad rows written as zero
//   hcir_mae_scatter_rows       its backward: every row of the fp32 stream gradient is written, the compact row where
//                               the token is in idx, zero elsewhere - no separate fill
//   hcir_mae_decoder_input      x[i][tok] = (tok kept ? embed[i][j(tok)] : mask_token) + decoder_pos[tok], one pass
//   hcir_mae_decoder_input_bwd  d_embed[i][j] = fp16(dres[i][idx_keep[i][j]]) and g_mask_token = the column sums of the
//                               masked rows (decoder_pos_embed takes no gradient: requires_grad=False in lightly)
//   hcir_mae_mse_fwd            mean (pred - target)^2 and fp16(pred - target), the target read straight from the image
// All are memory-bound passes with 16-byte accesses (d % 8 == 0, P % 8 == 0).  The token indices of an image are
// distinct, so a gather or scatter needs no atomics; the kernels that go from a token to its compact row build the
// inverse table of the image in LDS (inv[tok] = j or -1).  No float atomics anywhere: partial sums go to a
// caller-provided workspace and are added in a fixed order, so two runs give the same bits.  Every index read from
// device memory is range-checked before it addresses anything; a compact row whose index is outside [0, t) is written
// as zero and the token table ignores it.
#include "mim_patch.h"
#include "split_sum.h"

namespace {

constexpr int MAE_THREADS = 256;
constexpr int MAE_MAX_T = 1024;        // tokens per image: the inverse table in LDS
constexpr int MAE_ROWS = 32;           // token rows per workgroup of the scatter and the decoder input
constexpr int MAE_BWD_CHUNKS = 256;    // most workgroup shares (of whole images) of hcir_mae_decoder_input_bwd

inline int64_t mae_bwd_chunks(int64_t b) { return b < MAE_BWD_CHUNKS ? b : MAE_BWD_CHUNKS; }

// inv[tok] = j with idx[j] == tok, or -1; ends on a barrier.  The caller puts a barrier in front of a rebuild.
__device__ __forceinline__ void mae_inverse_table(const int64_t* __restrict__ idx, int k, int t, int* inv) {
  for (int i = threadIdx.x; i < t; i += MAE_THREADS) inv[i] = -1;
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += MAE_THREADS) {
    const int64_t tk = idx[j];
    if (tk >= 0 && tk < t) inv[tk] = j;
  }
  __syncthreads();
}

// ---------------------------------------------------------------- gather
__global__ __launch_bounds__(MAE_THREADS) void mae_gather_kernel(const _Float16* __restrict__ tok, int64_t rows,
                                                                 int64_t pad_rows, int t, int d,
                                                                 const int64_t* __restrict__ idx, int k,
                                                                 _Float16* __restrict__ out) {
  const int groups = d >> 3;
  const int64_t i = (int64_t)blockIdx.x * MAE_THREADS + threadIdx.x;
  if (i >= pad_rows * groups) return;
  const int64_t row = i / groups;
  const int col = (int)(i - row * groups) * 8;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (row < rows) {
    const int64_t tk = idx[row];
    if (tk >= 0 && tk < t) v = *reinterpret_cast<const u32x4*>(tok + ((row / k) * t + tk) * d + col);
  }
  *reinterpret_cast<u32x4*>(out + row * d + col) = v;
}

// ---------------------------------------------------------------- scatter
// Workgroup (x, y): image x, token rows [32 y, 32 (y + 1)).
__global__ __launch_bounds__(MAE_THREADS) void mae_scatter_kernel(const float* __restrict__ comp, int t, int d,
                                                                  const int64_t* __restrict__ idx, int k,
                                                                  float* __restrict__ dtok) {
  __shared__ int inv[MAE_MAX_T];
  const int64_t bi = blockIdx.x;
  mae_inverse_table(idx + bi * k, k, t, inv);
  const int r0 = blockIdx.y * MAE_ROWS, r1 = r0 + MAE_ROWS < t ? r0 + MAE_ROWS : t;
  const int groups = d >> 2;
  for (int u = threadIdx.x; u < (r1 - r0) * groups; u += MAE_THREADS) {
    const int row = r0 + u / groups, col = (u % groups) * 4;
    const int j = inv[row];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (j >= 0) v = *reinterpret_cast<const f32x4*>(comp + (bi * k + j) * d + col);
    *reinterpret_cast<f32x4*>(dtok + (bi * t + row) * d + col) = v;
  }
}

// ---------------------------------------------------------------- decoder input
__global__ __launch_bounds__(MAE_THREADS) void mae_decoder_input_kernel(const _Float16* __restrict__ embed, int t, int d,
                                                                        const int64_t* __restrict__ idx, int k,
                                                                        const float* __restrict__ mask_token,
                                                                        const float* __restrict__ pos,
                                                                        _Float16* __restrict__ x) {
  __shared__ int inv[MAE_MAX_T];
  const int64_t bi = blockIdx.x;
  mae_inverse_table(idx + bi * k, k, t, inv);
  const int r0 = blockIdx.y * MAE_ROWS, r1 = r0 + MAE_ROWS < t ? r0 + MAE_ROWS : t;
  const int groups = d >> 3;
  for (int u = threadIdx.x; u < (r1 - r0) * groups; u += MAE_THREADS) {
    const int row = r0 + u / groups, col = (u % groups) * 8;
    const int j = inv[row];
    float v[8];
    if (j >= 0) {
      const f16x8 e = *reinterpret_cast<const f16x8*>(embed + (bi * k + j) * d + col);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (float)e[i];
    } else {
      const f32x4 m0 = *reinterpret_cast<const f32x4*>(mask_token + col);
      const f32x4 m1 = *reinterpret_cast<const f32x4*>(mask_token + col + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = m0[i];
        v[4 + i] = m1[i];
      }
    }
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pos + (int64_t)row * d + col);
    const f32x4 p1 = *reinterpret_cast<const f32x4*>(pos + (int64_t)row * d + col + 4);
    f16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (_Float16)(v[i] + (i < 4 ? p0[i & 3] : p1[i & 3]));   // one fp32 add, one rounding to fp16
    *reinterpret_cast<f16x8*>(x + (bi * t + row) * d + col) = o;
  }
}

// ---------------------------------------------------------------- decoder input, backward
// Workgroup (x, y): the 256 columns from 256 x, the images [y per, (y + 1) per).  Thread (cx = tid % 32, ry = tid / 32)
// owns 8 columns and walks the token rows ry, ry + 8, ... of each image of the share, images in order: a kept row goes
// to d_embed as fp16, a masked row is added to the thread's fp32 accumulators.  The 8 row lanes are then added in order
// ry = 0..7 and the share's sums go to part[y][d]; split_sum adds the shares in order.
__global__ __launch_bounds__(MAE_THREADS) void mae_decoder_input_bwd_kernel(const float* __restrict__ dres, int64_t b,
                                                                            int t, int d,
                                                                            const int64_t* __restrict__ idx, int k,
                                                                            int64_t per, _Float16* __restrict__ d_embed,
                                                                            float* __restrict__ part) {
  __shared__ int inv[MAE_MAX_T];
  __shared__ float red[8][256 + 8];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int col = (blockIdx.x * 32 + cx) * 8;
  const int64_t i0 = (int64_t)blockIdx.y * per;
  const int64_t i1 = i0 + per < b ? i0 + per : b;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int64_t bi = i0; bi < i1; ++bi) {
    __syncthreads();                               // the previous image's reads of inv are done
    mae_inverse_table(idx + bi * k, k, t, inv);
    if (col < d) {
      for (int row = ry; row < t; row += 8) {
        const float* src = dres + (bi * t + row) * d + col;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src);
        const f32x4 c = *reinterpret_cast<const f32x4*>(src + 4);
        const int j = inv[row];
        if (j >= 0) {
          f16x8 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = (_Float16)a[e];
            o[4 + e] = (_Float16)c[e];
          }
          *reinterpret_cast<f16x8*>(d_embed + (bi * k + j) * d + col) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] += a[e];
            acc[4 + e] += c[e];
          }
        }
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

// ---------------------------------------------------------------- masked-patch MSE
// The plan of mim_l1_kernel: workgroup w takes the rows [w share, (w + 1) share); a thread adds (pred - target)^2 of its
// 8-element groups (groups tid, tid + 256, ... of each row, elements in order, rows in order) into one fp32 accumulator
// by fma (the square itself is not rounded); wave butterfly, the four waves in order; part[w] gets the sum.
__global__ __launch_bounds__(MIM_THREADS) void mae_mse_kernel(const _Float16* __restrict__ pred, MimImage im,
                                                              const int64_t* __restrict__ idx, int n, int64_t rows,
                                                              int64_t share, _Float16* __restrict__ diff,
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
          acc = __builtin_fmaf(df, df, acc);
          s[j] = (_Float16)df;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = (_Float16)0.f;
      }
      *reinterpret_cast<f16x8*>(diff + row * P + e) = s;
    }
  }
  const float tot = mim_block_sum(acc, wave_part);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

int mae_token_args(int64_t b, int32_t t, int32_t d, int32_t k) {
  if (b <= 0 || t <= 0 || d <= 0 || k <= 0 || k > t) return HCIR_ERR_INVALID;
  if (d % 8 || t > MAE_MAX_T || b * t >= (int64_t)1 << 31 || b > 0x7fffffff) return HCIR_ERR_UNSUPPORTED;
  return HCIR_OK;
}

}  // namespace

extern "C" {

int hcir_mae_gather_rows(const void* tok, int64_t b, int32_t t, int32_t d, const int64_t* idx, int32_t k, void* out,
                         void* stream) {
  HCIR_ENTER();
  const int rc = mae_token_args(b, t, d, k);
  if (rc != HCIR_OK) return rc;
  if (!tok || !idx || !out) return HCIR_ERR_INVALID;
  const int64_t rows = b * k, pad_rows = (rows + 63) / 64 * 64;
  hipLaunchKernelGGL(mae_gather_kernel, dim3((unsigned)hcir_cdiv(pad_rows * (d / 8), MAE_THREADS)), dim3(MAE_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const _Float16*>(tok), rows, pad_rows, t, d, idx, k,
                     static_cast<_Float16*>(out));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_mae_scatter_rows(const float* comp, int64_t b, int32_t t, int32_t d, const int64_t* idx, int32_t k,
                          float* dtok, void* stream) {
  HCIR_ENTER();
  const int rc = mae_token_args(b, t, d, k);
  if (rc != HCIR_OK) return rc;
  if (!comp || !idx || !dtok) return HCIR_ERR_INVALID;
  hipLaunchKernelGGL(mae_scatter_kernel, dim3((unsigned)b, (unsigned)hcir_cdiv(t, MAE_ROWS)), dim3(MAE_THREADS), 0,
                     static_cast<hipStream_t>(stream), comp, t, d, idx, k, dtok);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_mae_decoder_input(const void* embed, int64_t b, int32_t t, int32_t d, const int64_t* idx_keep, int32_t k,
                           const float* mask_token, const float* pos, void* x, void* stream) {
  HCIR_ENTER();
  const int rc = mae_token_args(b, t, d, k);
  if (rc != HCIR_OK) return rc;
  if (!embed || !idx_keep || !mask_token || !pos || !x) return HCIR_ERR_INVALID;
  hipLaunchKernelGGL(mae_decoder_input_kernel, dim3((unsigned)b, (unsigned)hcir_cdiv(t, MAE_ROWS)), dim3(MAE_THREADS), 0,
                     static_cast<hipStream_t>(stream), static_cast<const _Float16*>(embed), t, d, idx_keep, k, mask_token,
                     pos, static_cast<_Float16*>(x));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

size_t hcir_mae_decoder_input_bwd_workspace_bytes(int64_t b, int32_t d) {
  if (b <= 0 || d <= 0 || d % 8) return 0;
  return (size_t)mae_bwd_chunks(b) * d * sizeof(float);
}

int hcir_mae_decoder_input_bwd(const float* dres, int64_t b, int32_t t, int32_t d, const int64_t* idx_keep, int32_t k,
                               void* d_embed, float* g_mask_token, void* workspace, size_t workspace_bytes,
                               void* stream) {
  HCIR_ENTER();
  const int rc = mae_token_args(b, t, d, k);
  if (rc != HCIR_OK) return rc;
  if (!dres || !idx_keep || !d_embed || !g_mask_token) return HCIR_ERR_INVALID;
  const int64_t chunks = mae_bwd_chunks(b);
  if (!workspace || workspace_bytes < (size_t)chunks * d * sizeof(float)) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mae_decoder_input_bwd_kernel, dim3((unsigned)hcir_cdiv(d, 256), (unsigned)chunks),
                     dim3(MAE_THREADS), 0, st, dres, b, t, d, idx_keep, k, hcir_cdiv(b, chunks),
                     static_cast<_Float16*>(d_embed), static_cast<float*>(workspace));
  HCIR_LAUNCH_CHECK();
  split_sum(static_cast<const float*>(workspace), (int)chunks, d, g_mask_token, st);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

size_t hcir_mae_mse_workspace_bytes(int64_t rows) {
  return rows <= 0 ? 0 : (size_t)mim_l1_blocks(rows) * sizeof(float);
}

int hcir_mae_mse_fwd(const void* pred, const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps,
                     const int64_t* idx, int32_t n, float* loss, void* diff, void* workspace, size_t workspace_bytes,
                     void* stream) {
  HCIR_ENTER();
  MimImage im;
  const int rc = mim_image(img, b, c, h, w, ps, n, &im);
  if (rc != HCIR_OK) return rc;
  if (!pred || !img || !idx || !loss || !diff) return HCIR_ERR_INVALID;
  const int64_t rows = b * n, blocks = mim_l1_blocks(rows);
  if (!workspace || workspace_bytes < (size_t)blocks * sizeof(float)) return HCIR_ERR_WORKSPACE;
  const int64_t P = (int64_t)c * ps * ps;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mae_mse_kernel, dim3((unsigned)blocks), dim3(MIM_THREADS), (size_t)P * sizeof(float), st,
                     static_cast<const _Float16*>(pred), im, idx, n, rows, hcir_cdiv(rows, blocks),
                     static_cast<_Float16*>(diff), static_cast<float*>(workspace));
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(mim_l1_finish_kernel, dim3(1), dim3(MIM_THREADS), 0, st, static_cast<const float*>(workspace),
                     (int)blocks, 1.0f / (float)(rows * P), loss);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
