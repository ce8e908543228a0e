// conv_bwd.hip — the backward half of the ResNet body convolutions: weight gradient, and the "spread by 2" copy that
// turns hcir_conv2d_f16 into the data gradient of a stride-2 convolution (hcir/conv_train.py holds the three dgrad
// plans).  Geometry and split choice: conv_plan.h.  Decisions and measurements: DESIGN.md §3.4.
#include "common.h"
#include "conv_plan.h"
#include "split_sum.h"
#include "tr_layout.h"

namespace {

// ------------------------------------------------------------------ hcir_conv2d_wgrad_f16
// dw[n][r][s][c] = sum_m dy[m][n] * x[pixel(m) + tap(r, s)][c], m = (b, ho, wo) linear, padding taps zero.
// The contraction index m is the SLOW index of both operands (gemm_tn.hip's situation), so the tiles are staged as
// they are stored - [64 m][TN n] of dy and [64 m][TC c] of the tap's input pixels, the gather with zeros in the padding
// being the A fill of conv2d_f16_kernel - and the fragments are read TRANSPOSED with ds_read_b64_tr_b16, two reads
// per 16x16x32 operand.  The swizzle of the 256-B and 128-B rows and the lanes' rows: tr_layout.h.
// Workgroup: 4 waves (2 along n x 2 along c) on a TN x TC tile of ONE tap, TN / TC = 128 where the channel count
// allows, else 64; fill through registers one step ahead (two LDS buffers, one barrier per step) as in conv.hip.
// M is split over workgroups; each (tile, split) writes its fp32 partial tile to the workspace and a second kernel
// (split_sum.h) adds the splits in split order: no float atomics, two runs are bit-identical.

struct WgradArgs {
  const _Float16* x;
  const _Float16* dy;
  float* part;             // [splits][Cout][K] partial tiles, or dw itself when splits == 1
  int64_t part_stride;     // Cout * K (0 when splits == 1)
  int64_t m, rows_per_split;
  int32_t h, w_px, cin, cout, s, stride, pad, ho, wo, k, tiles_c, taps, tiles;
};

template <int TN, int TC>
__global__ __launch_bounds__(256) void conv2d_wgrad_kernel(const WgradArgs a) {
  constexpr int FN = TN / 32, FC = TC / 32;            // 16 x 16 fragments per wave along n / c
  constexpr int CPR_N = TN / 8, CPR_C = TC / 8;        // 16-B chunks per tile row
  constexpr int RP_N = 256 / CPR_N, RP_C = 256 / CPR_C;  // rows one pass of the 256 threads fills
  constexpr int PN = WGRAD_BM / RP_N, PC = WGRAD_BM / RP_C;
  __shared__ __attribute__((aligned(16))) char Ys[2][WGRAD_BM * TN * 2];
  __shared__ __attribute__((aligned(16))) char Xs[2][WGRAD_BM * TC * 2];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wave_n = wv & 1, wave_c = wv >> 1;
  const int tile = (int)(blockIdx.x % (unsigned)a.tiles), split = (int)(blockIdx.x / (unsigned)a.tiles);
  const int tap = tile % a.taps, tnc = tile / a.taps;   // tap fastest: neighbours share the dy rows in L2
  const int n0 = (tnc / a.tiles_c) * TN, c0 = (tnc % a.tiles_c) * TC;
  const int r = tap / a.s, s = tap - r * a.s;
  const int64_t m_begin = (int64_t)split * a.rows_per_split;
  const int64_t m_end = m_begin + a.rows_per_split < a.m ? m_begin + a.rows_per_split : a.m;
  const int nsteps = (int)((m_end - m_begin + WGRAD_BM - 1) / WGRAD_BM);   // >= 1: split < cdiv(m, rows_per_split)

  // fill roles: dy chunk column yc of rows yr + RP_N i; x chunk column xc of rows xr + RP_C i.  The x rows' output
  // pixel (b, oh, ow) is decoded once and then advanced by 64 pixels per step with two carries.
  const int yc = t % CPR_N, yr = t / CPR_N, xc = t % CPR_C, xr = t / CPR_C;
  const int32_t adv_w = WGRAD_BM % a.wo, q64 = WGRAD_BM / a.wo, adv_h = q64 % a.ho, adv_b = q64 / a.ho;
  int32_t ob[PC], oh[PC], ow[PC];
#pragma unroll
  for (int i = 0; i < PC; ++i) {
    const int64_t m = m_begin + xr + RP_C * i;
    const int32_t hw = a.ho * a.wo;
    ob[i] = (int32_t)(m / hw);
    const int32_t rem = (int32_t)(m - (int64_t)ob[i] * hw);
    oh[i] = rem / a.wo;
    ow[i] = rem - oh[i] * a.wo;
  }

  u32x4 yreg[PN], xreg[PC];
  auto load = [&](int step) {   // called for step = 0, 1, 2, ... in order: it advances the pixel state
    const int64_t mb = m_begin + (int64_t)step * WGRAD_BM;
#pragma unroll
    for (int i = 0; i < PN; ++i) {
      const int64_t m = mb + yr + RP_N * i;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m < m_end) v = *(const u32x4*)(a.dy + m * a.cout + n0 + yc * 8);
      yreg[i] = v;
    }
#pragma unroll
    for (int i = 0; i < PC; ++i) {
      const int64_t m = mb + xr + RP_C * i;
      const int hi = oh[i] * a.stride + r - a.pad, wi = ow[i] * a.stride + s - a.pad;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m < m_end && (unsigned)hi < (unsigned)a.h && (unsigned)wi < (unsigned)a.w_px)
        v = *(const u32x4*)(a.x + (((int64_t)ob[i] * a.h + hi) * a.w_px + wi) * a.cin + c0 + xc * 8);
      xreg[i] = v;
      ow[i] += adv_w;
      const int cw = ow[i] >= a.wo;
      ow[i] -= cw ? a.wo : 0;
      oh[i] += adv_h + cw;
      const int chh = oh[i] >= a.ho;
      oh[i] -= chh ? a.ho : 0;
      ob[i] += adv_b + chh;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < PN; ++i) *(u32x4*)(&Ys[buf][tr_fill_off<2 * TN>(yr + RP_N * i, yc)]) = yreg[i];
#pragma unroll
    for (int i = 0; i < PC; ++i) *(u32x4*)(&Xs[buf][tr_fill_off<2 * TC>(xr + RP_C * i, xc)]) = xreg[i];
  };

  f32x4 acc[FN][FC];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FC; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const TrLane ln = tr_lane(lane);
  load(0);
  stash(0);
  __syncthreads();
  for (int step = 0; step < nsteps; ++step) {
    const int buf = step & 1;
    const bool more = step + 1 < nsteps;   // uniform over the workgroup: the transposed reads below run with EXEC full
    if (more) load(step + 1);
    const char* yt = Ys[buf];
    const char* xt = Xs[buf];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f16x8 af[FN], bf[FC];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int row = tr_lane_row(ln, ks, hf);
#pragma unroll
        for (int i = 0; i < FN; ++i) {
          const int c32 = wave_n * FN + i;   // 16 columns = 32 B = one chunk
          tr_read_half(af[i], hf, yt + tr_read_off<2 * TN>(row, c32, ln.p4));
        }
#pragma unroll
        for (int j = 0; j < FC; ++j) {
          const int c32 = wave_c * FC + j;
          tr_read_half(bf[j], hf, xt + tr_read_off<2 * TC>(row, c32, ln.p4));
        }
      }
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
  }

  // acc[i][j][e] is dw[n0 + (TN/2) wave_n + 16 i + 4 (lane >> 4) + e][tap][c0 + (TC/2) wave_c + 16 j + (lane & 15)]
  float* out = a.part + (int64_t)split * a.part_stride;
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + wave_n * (TN / 2) + i * 16 + ln.g16 * 4 + e;
#pragma unroll
      for (int j = 0; j < FC; ++j)
        out[(int64_t)n * a.k + tap * a.cin + c0 + wave_c * (TC / 2) + j * 16 + (lane & 15)] = acc[i][j][e];
    }
}

// ------------------------------------------------------------------ hcir_spread2_nhwc_f16
// One thread per 16-B chunk of dst: the source pixel's chunk at even (y, x) inside the source map, zeros elsewhere.
__global__ __launch_bounds__(256) void spread2_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int hs,
                                                      int ws, int c8, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c8);
  const int64_t pix = i / c8;
  const int x = (int)(pix % w);
  const int64_t rest = pix / w;
  const int y = (int)(rest % h);
  const int64_t b = rest / h;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (!((x | y) & 1) && (y >> 1) < hs && (x >> 1) < ws) v = src[((b * hs + (y >> 1)) * ws + (x >> 1)) * c8 + ch];
  dst[i] = v;
}

template <int TN, int TC>
void wgrad_launch(const WgradArgs& a, unsigned blocks, hipStream_t st) {
  hipLaunchKernelGGL((conv2d_wgrad_kernel<TN, TC>), dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace

extern "C" size_t hcir_conv2d_wgrad_workspace_bytes(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                                    int32_t r, int32_t s, int32_t stride, int32_t pad) {
  WgradPlan p;
  if (wgrad_plan(b, h, w, cin, cout, r, s, stride, pad, &p) != HCIR_OK) return 0;
  return wgrad_workspace_bytes(p, cout);
}

// HOST: the number of M splits the launch uses, or the status hcir_conv2d_wgrad_f16 would return for the shape.
extern "C" int32_t hcir_conv2d_wgrad_splits(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r,
                                            int32_t s, int32_t stride, int32_t pad) {
  WgradPlan p;
  const int st = wgrad_plan(b, h, w, cin, cout, r, s, stride, pad, &p);
  return st != HCIR_OK ? st : p.splits;
}

extern "C" int hcir_conv2d_wgrad_f16(const void* x, const void* dy, int64_t b, int32_t h, int32_t w, int32_t cin,
                                     int32_t cout, int32_t r, int32_t s, int32_t stride, int32_t pad, float* dw,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  WgradPlan p;
  const int st = wgrad_plan(b, h, w, cin, cout, r, s, stride, pad, &p);   // host arithmetic only: no device needed
  if (st != HCIR_OK) return st;
  if (!x || !dy || !dw) return HCIR_ERR_INVALID;
  const size_t need = wgrad_workspace_bytes(p, cout);
  if (need && (!workspace || workspace_bytes < need)) return HCIR_ERR_WORKSPACE;
  const int64_t blocks = (int64_t)p.tiles * p.splits;
  if (blocks > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  HCIR_ENTER();
  const int64_t nk = (int64_t)cout * p.k;
  WgradArgs a;
  a.x = (const _Float16*)x;
  a.dy = (const _Float16*)dy;
  a.part = p.splits > 1 ? (float*)workspace : dw;
  a.part_stride = p.splits > 1 ? nk : 0;
  a.m = p.m;
  a.rows_per_split = p.rows_per_split;
  a.h = h; a.w_px = w; a.cin = cin; a.cout = cout; a.s = s; a.stride = stride; a.pad = pad;
  a.ho = p.ho; a.wo = p.wo; a.k = p.k; a.tiles_c = cin / p.tc; a.taps = p.taps; a.tiles = p.tiles;
  hipStream_t hs = (hipStream_t)stream;
  if (p.tn == 128 && p.tc == 128) wgrad_launch<128, 128>(a, (unsigned)blocks, hs);
  else if (p.tn == 128) wgrad_launch<128, 64>(a, (unsigned)blocks, hs);
  else if (p.tc == 128) wgrad_launch<64, 128>(a, (unsigned)blocks, hs);
  else wgrad_launch<64, 64>(a, (unsigned)blocks, hs);
  HCIR_LAUNCH_CHECK();
  if (p.splits > 1) {
    split_sum((const float*)workspace, p.splits, nk, dw, hs);   // Cout * K is a multiple of 4096
    HCIR_LAUNCH_CHECK();
  }
  return HCIR_OK;
}

extern "C" int hcir_spread2_nhwc_f16(const void* src, int64_t b, int32_t hs, int32_t ws, int32_t c, int32_t h,
                                     int32_t w, void* dst, void* stream) {
  if (b < 1 || hs < 1 || ws < 1 || c < 1 || h < 1 || w < 1) return HCIR_ERR_INVALID;
  if (2 * ((int64_t)hs - 1) > (int64_t)h - 1 || 2 * ((int64_t)ws - 1) > (int64_t)w - 1) return HCIR_ERR_INVALID;
  if (c % 8 != 0) return HCIR_ERR_UNSUPPORTED;   // 16-B chunks
  const int64_t total = b * (int64_t)h * w * (c / 8);
  if (b > INT32_MAX || total > ((int64_t)1 << 38)) return HCIR_ERR_UNSUPPORTED;
  if (!src || !dst) return HCIR_ERR_INVALID;
  HCIR_ENTER();
  hipLaunchKernelGGL(spread2_kernel, dim3((unsigned)hcir_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const u32x4*)src, (u32x4*)dst, hs, ws, c / 8, h, w, total);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}
