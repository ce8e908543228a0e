// dense_match.hip — DenseCL's dense correspondence: for every query position the most similar key position of the same
// image, and the gather of that position's value row.
//
// Semantics: lightly.models.utils.select_most_similar(x, y, y_values), as called by the DenseCL step at
// HairPretraining/src/pretrain_engine.py:304-306:
//   j*(b, n) = argmax_m (x_bn . y_bm) / max(||y_bm||, 1e-12),   out[b][n] = y_values[b][j*(b, n)]
// x's own norm is a positive row constant and is not computed; a zero x row scores 0 everywhere and takes index 0.  On
// exact ties of the fp32 scores the lowest m wins (torch.argmax).
//
// Kernels
//   dm_prep  : one wave per key row: fp32 sum of squares -> 1 / max(||y||, 1e-12).
//   dm_match : one workgroup per (image, block of 128 query rows) on the pair_tiles.h main loop: keys streamed as
//              column tiles of 128, a lane owns one query row and keeps a running (best score, best index); the four
//              partials of a row meet in LDS in a fixed order, the lower index winning ties; the same workgroup then
//              copies the chosen value rows in 16-byte pieces.
#include "pair_tiles.h"

namespace {

__global__ __launch_bounds__(256) void dm_prep(const _Float16* __restrict__ y, int64_t rows, int c,
                                               float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s = 0.f;
  for (int k = lane; k < c; k += 64) {
    const float v = (float)y[row * c + k];
    s = __builtin_fmaf(v, v, s);
  }
  s = wave_sum(s);
  if (lane == 0) inv[row] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
}

struct DmArgs {
  const _Float16* x;   // [B][N][C]
  const _Float16* y;   // [B][M][C]
  const float* inv;    // [B][M]
  const char* values;  // [B][M][row_bytes] or NULL
  int32_t* idx;        // [B][N]
  char* out;           // [B][N][row_bytes]
  int n, m, c;
  int row_bytes;       // Dv * element size, a multiple of 16
};

template <bool GLDS>
__global__ __launch_bounds__(256, 2) void dm_match(DmArgs a) {
  using T = _Float16;
  using Cfg = PairCfg<T>;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_c = wave >> 1, wave_r = wave & 1;
  const int h = lane >> 5;
  const int64_t img = blockIdx.y;
  const int r0 = blockIdx.x * 128;
  const T* xb = a.x + img * a.n * (int64_t)a.c;
  const T* yb = a.y + img * a.m * (int64_t)a.c;
  const float* invb = a.inv + img * a.m;

  const float ninf = -__builtin_huge_valf();
  float bs[2] = {ninf, ninf};
  int bi[2] = {0, 0};
  for (int c0 = 0; c0 < a.m; c0 += 128) {
    f32x16 acc[2][2];
    pair_tile_products<T, GLDS>(acc, lds, yb, (int64_t)c0, (int64_t)a.m, xb, (int64_t)r0, (int64_t)a.n, a.c, tid, lane,
                                wave_c, wave_r);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int col = c0 + wave_c * 64 + ct * 32 + acc_row(i, h);
        const float rinv = invb[col < a.m ? col : a.m - 1];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          const float s = acc[ct][rt][i] * rinv;
          if (col < a.m && better(s, col, bs[rt], bi[rt])) {
            bs[rt] = s;
            bi[rt] = col;
          }
        }
      }
    }
  }
  // the four (wave_c, lane-half) partials of a row meet in LDS: [128 rows][4 src][score, index]; the chosen indices
  // of the block follow
  float* red = reinterpret_cast<float*>(lds);
  int* chosen = reinterpret_cast<int*>(lds + 128 * 4 * 2 * 4);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int rl = wave_r * 64 + rt * 32 + (lane & 31), src = wave_c * 2 + h;
    red[(rl * 4 + src) * 2 + 0] = bs[rt];
    red[(rl * 4 + src) * 2 + 1] = __int_as_float(bi[rt]);
  }
  __syncthreads();
  if (tid < 128) {
    const float* p = red + tid * 8;
    float s = p[0];
    int j = __float_as_int(p[1]);
#pragma unroll
    for (int q = 1; q < 4; ++q) {  // fixed order; the lower index wins a tie
      const float sq = p[q * 2];
      const int jq = __float_as_int(p[q * 2 + 1]);
      if (better(sq, jq, s, j)) {
        s = sq;
        j = jq;
      }
    }
    j = j < 0 ? 0 : (j >= a.m ? a.m - 1 : j);
    chosen[tid] = j;
    if (r0 + tid < a.n) a.idx[img * a.n + r0 + tid] = j;
  }
  if (!a.values) return;
  __syncthreads();
  const int rows = a.n - r0 < 128 ? a.n - r0 : 128;
  const int ppr = a.row_bytes >> 4;  // 16-byte pieces per row
  const char* vb = a.values + img * a.m * (int64_t)a.row_bytes;
  char* ob = a.out + (img * a.n + r0) * (int64_t)a.row_bytes;
  for (int64_t t = tid; t < (int64_t)rows * ppr; t += 256) {
    const int rl = (int)(t / ppr), piece = (int)(t - (int64_t)rl * ppr);
    const u32x4 v = *reinterpret_cast<const u32x4*>(vb + chosen[rl] * (int64_t)a.row_bytes + piece * 16);
    *reinterpret_cast<u32x4*>(ob + rl * (int64_t)a.row_bytes + piece * 16) = v;
  }
}

}  // namespace

extern "C" {

size_t hcir_dense_match_workspace_bytes(int64_t b, int32_t m) {
  if (b <= 0 || m <= 0) return 0;
  return (size_t)b * m * 4;
}

int hcir_dense_match_f16(const void* x, const void* y, const void* y_values, int values_dtype, int64_t b, int32_t n,
                         int32_t m, int32_t c, int32_t dv, int32_t* idx, void* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  HCIR_ENTER();
  if (!x || !y || !idx || b <= 0 || n <= 0 || m <= 0 || c <= 0 || b > 65535) return HCIR_ERR_INVALID;
  if (y_values && (!out || dv <= 0)) return HCIR_ERR_INVALID;
  if (n > 256 || m > 256 || (c & 7) || (y_values && (dv & 7))) return HCIR_ERR_UNSUPPORTED;
  if (y_values && values_dtype != HCIR_F32 && values_dtype != HCIR_F16) return HCIR_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < hcir_dense_match_workspace_bytes(b, m)) return HCIR_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* inv = static_cast<float*>(workspace);
  hipLaunchKernelGGL(dm_prep, dim3((unsigned)hcir_cdiv(b * m, 4)), dim3(256), 0, st, static_cast<const _Float16*>(y),
                     b * m, c, inv);
  HCIR_LAUNCH_CHECK();
  DmArgs a{static_cast<const _Float16*>(x), static_cast<const _Float16*>(y), inv,
           static_cast<const char*>(y_values), idx, static_cast<char*>(out), n, m, c,
           y_values ? dv * (values_dtype == HCIR_F32 ? 4 : 2) : 0};
  const dim3 grid((unsigned)hcir_cdiv(n, 128), (unsigned)b);
  if (c % SimElem<_Float16>::kPerStage == 0)
    hipLaunchKernelGGL(dm_match<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(dm_match<false>, grid, dim3(256), 0, st, a);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
