// gemm.hip — out[M,N] = epilogue(A[M,K] . W[N,K]^T), fp16 MFMA, fp32 accumulate.
//
// Replaces nn.Linear / nn.MultiheadAttention in_proj,out_proj / MLPBlock / timm Mlp
// on the ViT path (HP/src/models_vit.py:63,66,70,79; torchvision EncoderBlock via
// HP/src/main_backbone.py:554) and Conv2d(3,768,16,16) patch embedding
// (HP/src/main_backbone.py:543; HP/src/models_vit.py:42,48).
//
// Three kernels (launch_gemm / launch_gemm_big pick):
//   * gemm_f16_big_kernel — M >= 1024, N % 256 == 0, K % 64 == 0 (every encoder GEMM of the benchmark):
//     persistent 256(n) x 256(m) x 64(k) tiles, 8 waves of 128 x 64 (MFMA 16x16x32), two 64 KB LDS slots filled
//     by LDS-DMA, LDS-transposed full-line epilogues incl. the LayerNorm fold (hcir_gemm_f16_fused);
//   * gemm_f16_mid_kernel — the same shapes when the 256 x 256 tiles fill the 256 CUs badly (small M, the rows
//     behind the last whole round of tiles): persistent 128(n) x 192(m) x 64(k) tiles, 4 waves of 64 x 96, two
//     workgroups per CU; bit-identical results;
//   * gemm_f16_kernel — everything else (small M, ragged N / K): the sim_core.h tile engine with W rows on the
//     MFMA row index and activation rows on the column index (a lane owns ONE activation row and receives the
//     output features in groups of 4 registers), workgroup tile 128 x 128 x 64, 4 waves of 2x2 MFMA 32x32x16.
// The two persistent kernels differ in geometry (G256 / GMid) and in their MFMA loops only: they share ONE stage
// issuer (GemmStages<G>) and ONE LDS-transposing epilogue (gemm_epilogue_lds).
#include "sim_core.h"
#include "act.h"
#include "gemm_plan.h"
#include "patch_plan.h"
#include "gemm_stage_addr.h"
#include <stdlib.h>

namespace {

using GemmCfg = SimCfg<_Float16, 2, 2, 2>;  // GM = 128 W rows, QB = 128 A rows

// Internal epilogue codes of hcir_gemm_f16_fused (persistent kernel only), beyond hcir_epilogue:
//   EPI_RESID_F16_STATS: BIAS_RESID_F16 that also writes per-row partial (mean, M2 = sum of squared deviations
//                        from it) of the stored fp16 rows, one slice per 64 output features, for the LayerNorm that reads them next;
//   EPI_LN_BIAS_F16 / EPI_LN_BIAS_GELU_F16: the A rows are the RAW residual rows x and W carries the
//                        LayerNorm gamma (W' = gamma o W): out = act(rstd[m] (acc - mean[m] c1[n]) + bias[n])
//                        with c1[n] = sum_k W'[n][k], bias[n] = sum_k beta[k] W[n][k] + b[n]  (LayerNorm folded
//                        into the GEMM; no normalised copy of the tokens is ever written).
constexpr int EPI_RESID_F16_STATS = 7;
constexpr int EPI_LN_BIAS_F16 = 8;
constexpr int EPI_LN_BIAS_GELU_F16 = 9;
constexpr int EPI_BIAS_F16_DUAL_GELU = 10;  // out = fp16(acc + bias) AND out2 = fp16(gelu(acc + bias)) (hcir_gemm_f16_gelu_dual)
// patch embedding (hcir_patch_embed_fused, PatchGemmArgs): out row m + m / np + 1 = fp16(acc + bias + pos_mult pos[1 + m % np])
// and, with stats_part, the slice statistics of EPI_RESID_F16_STATS for the stored rows
constexpr int EPI_PATCH_F16_STATS = 11;

struct GemmArgs {
  const _Float16* a;
  const _Float16* w;
  const float* bias;
  const float* scale;
  void* out;
  int64_t m, lda, ldw, ldo;
  int n, k;
  const float* ln_stats;  // [m][2] (mean, rstd) of the A rows           (EPI_LN_*)
  const float* ln_c1;     // [n]                                           (EPI_LN_*)
  float* stats_part;      // [n/64][m][2] partial (mean, M2) of out rows  (EPI_RESID_F16_STATS)
  const void* resid;      // residual rows of the *_RESID_* epilogues (same type and row pitch as out); == out: in place
  void* out2;             // second fp16 output of EPI_BIAS_F16_DUAL_GELU (row pitch ldo)
  int64_t stats_ld = 0;   // rows per slice of stats_part (0: m) - a launch over a row range of a larger matrix
};

// XCD-aware tile order (gemm_stage_addr.h)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) { return gemm_xcd_remap(bid, nwg); }

template <int EPI, int NTILES>
__device__ __forceinline__ void gemm_epilogue_t(const GemmArgs& g, const f32x16 (&acc)[NTILES][2],
                                                int64_t m0, int nbase, int wave_m, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int64_t m = m0 + wave_m * 64 + mt * 32 + r;
    if (m >= g.m) continue;
#pragma unroll
    for (int nt = 0; nt < NTILES; ++nt) {
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        const int n = nbase + nt * 32 + 8 * grp + 4 * h;
        if (n >= g.n) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[nt][mt][4 * grp + e];
        f32x4 b = {0.f, 0.f, 0.f, 0.f};
        if (g.bias) b = *reinterpret_cast<const f32x4*>(g.bias + n);
        if constexpr (EPI == HCIR_EPI_AFFINE_RELU_F16 || EPI == HCIR_EPI_AFFINE_F32) {
          const f32x4 s = *reinterpret_cast<const f32x4*>(g.scale + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(v[e], s[e], b[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += b[e];
        }
        if constexpr (EPI == HCIR_EPI_BIAS_F16 || EPI == HCIR_EPI_BIAS_GELU_F16 ||
                      EPI == HCIR_EPI_AFFINE_RELU_F16) {
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = v[e];
            if constexpr (EPI == HCIR_EPI_BIAS_GELU_F16) x = gelu_erf(x);
            if constexpr (EPI == HCIR_EPI_AFFINE_RELU_F16) x = fmaxf(x, 0.f);
            o[e] = (_Float16)x;
          }
          *reinterpret_cast<f16x4*>(static_cast<_Float16*>(g.out) + m * g.ldo + n) = o;
        } else if constexpr (EPI == HCIR_EPI_BIAS_RESID_F16) {
          _Float16* p = static_cast<_Float16*>(g.out) + m * g.ldo + n;
          const f16x4 oh = *reinterpret_cast<const f16x4*>(static_cast<const _Float16*>(g.resid) + m * g.ldo + n);
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float sc1 = g.scale ? g.scale[n + e] : 1.0f;
            o[e] = (_Float16)__builtin_fmaf(sc1, v[e], (float)oh[e]);
          }
          *reinterpret_cast<f16x4*>(p) = o;
        } else if constexpr (EPI == HCIR_EPI_BIAS_RESID_F32) {
          float* p = static_cast<float*>(g.out) + m * g.ldo + n;
          f32x4 o = *reinterpret_cast<const f32x4*>(static_cast<const float*>(g.resid) + m * g.ldo + n);
          if (g.scale) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(g.scale + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(s[e], v[e], o[e]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += v[e];
          }
          *reinterpret_cast<f32x4*>(p) = o;
        } else {
          *reinterpret_cast<f32x4*>(static_cast<float*>(g.out) + m * g.ldo + n) = v;
        }
      }
    }
  }
}

template <int EPI>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, const f32x16 (&acc)[2][2],
                                              int64_t m0, int n0, int wave_n, int wave_m, int lane) {
  gemm_epilogue_t<EPI, 2>(g, acc, m0, n0 + wave_n * 64, wave_m, lane);
}
// Hide a value's origin from hipcc's waitcnt pass: after the explicit wait below, bias / scale
// registers are "produced by asm", not by a pending global load.  Without this the per-iteration
// control flow of the store loop makes the pass re-insert `s_waitcnt vmcnt(0)` before EVERY store
// (it can no longer prove the bias load retired), which also drains the previous store: the 16-32
// stores of a tile were fully serialised (seen in the .s; 40 % of GEMM time).
__device__ __forceinline__ void launder(f32x4& v) { asm volatile("" : "+v"(v)); }

// Accumulators of one wave tile (128 n x 64 m), MFMA 16x16x32:
//   a[nt 0..7][mt 0..3], f32x4: n = 16nt + 4(lane>>4) + i, m = 16mt + (lane&15)
struct WaveAcc {
  f32x4 a[8][4];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[x][y][i] = 0.f;
  }
};

// 8-lane (one 128-B output line) sum by DPP: quad xor 1, quad xor 2, then the mirror of the 8-lane half row
__device__ __forceinline__ float sum8_dpp(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  return v;
}

// (mean, sum of squared deviations from that mean) of the 64 STORED fp16 values of one row slice, 8 per lane over the
// 8 lanes of a 128-B line, for the next LayerNorm.  Two-pass per slice (the values are in registers) and Chan's
// combination in the finalize kernel: a plain (sum, sum of squares) pair loses the variance to cancellation when
// |mean| >> std (0.2 % error in rstd at mean/std = 50).
__device__ __forceinline__ f32x2 slice_stats8(const f16x8& o) {
  float xv[8], s1 = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    xv[e] = (float)o[e];
    s1 += xv[e];
  }
  const float mean_s = sum8_dpp(s1) * (1.0f / 64.0f);
  float m2 = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float dv = xv[e] - mean_s;
    m2 = __builtin_fmaf(dv, dv, m2);
  }
  return (f32x2){mean_s, sum8_dpp(m2)};
}

// Patch rows -> token rows for a block of rows that starts at m0w (which may lie past M on a ragged tile): ONE exact
// division per block, at the block's first row clamped into M, then a small non-negative offset from it per row (a
// reciprocal estimate with an exact fix-up).  Offsets are never taken from an unclamped first row.
struct PatchRowMap {
  int mb, bi0, rem0, np;
  float inv;
  __device__ __forceinline__ PatchRowMap() : mb(0), bi0(0), rem0(0), np(1), inv(1.f) {}
  __device__ __forceinline__ PatchRowMap(int64_t m0w, int64_t mtot, int np_) : np(np_) {
    mb = (int)(m0w < mtot ? m0w : mtot - 1);
    bi0 = mb / np;
    rem0 = mb - bi0 * np;
    inv = 1.0f / (float)np;
  }
  // image bi and patch pi of row min(m, M - 1), m >= m0w
  __device__ __forceinline__ void map(int64_t m, int64_t mtot, int& bi, int& pi) const {
    const int r = rem0 + ((int)(m < mtot ? m : mtot - 1) - mb);
    int q = (int)((float)r * inv);
    q += ((q + 1) * np <= r) ? 1 : 0;
    q -= (q * np > r) ? 1 : 0;
    bi = bi0 + q;
    pi = r - q * np;
  }
};

// LDS-transposing epilogue of both persistent kernels, for a 16x16x32 accumulator block acc[NTW n-tiles][MTH m-tiles
// from mt0, of MTT]: (16 NTW) features x (16 MTH) rows, transposed through `region` (16 MTH rows x 128 B, private to
// the wave) one 128-B output line per row and pass.  The 256 x 256 kernel instantiates it at <8, 4, 4> (its whole
// 128 x 64 wave tile), the 128 x 192 kernel at <4, 6, 3> (one 48-row half of its 64 x 96 wave tile): ONE body, so
// the two kernels round the same fp32 value once and store the same bits (test_gemm_big_and_mid_kernels_same_bits;
// the tail split of launch_gemm_big sends rows of one matrix through both).
template <int EPI, bool FULL, int NTW, int MTT, int MTH, class GA>
__device__ __forceinline__ void gemm_epilogue_lds_impl(const GA& g, const f32x4 (&acc)[NTW][MTT], int mt0,
                                                       char* region, int64_t m0w, int nbase, int lane) {
  constexpr bool kLn = (EPI == EPI_LN_BIAS_F16 || EPI == EPI_LN_BIAS_GELU_F16);
  constexpr bool kGelu = (EPI == HCIR_EPI_BIAS_GELU_F16 || EPI == EPI_LN_BIAS_GELU_F16);
  constexpr bool kResidH = (EPI == HCIR_EPI_BIAS_RESID_F16 || EPI == EPI_RESID_F16_STATS);
  constexpr bool kDual = (EPI == EPI_BIAS_F16_DUAL_GELU);
  constexpr bool kPatch = (EPI == EPI_PATCH_F16_STATS);
  constexpr bool kF16 = (EPI == HCIR_EPI_BIAS_F16 || kGelu || kLn ||
                         EPI == HCIR_EPI_AFFINE_RELU_F16 || kResidH || kDual || kPatch);
  constexpr bool kAffine = (EPI == HCIR_EPI_AFFINE_RELU_F16 || EPI == HCIR_EPI_AFFINE_F32);
  constexpr int FPP = kF16 ? 64 : 32;      // output features (128 B) per pass
  constexpr int NPASS = NTW * 16 / FPP;
  constexpr int NIT = MTH * 2;             // groups of 8 rows
  constexpr int UB = (NIT % 4 == 0) ? 4 : 3;  // rows requested / stored back to back
  static_assert(NIT % UB == 0 && (NTW * 16) % FPP == 0, "geometry");
  const int rrow = lane >> 3, rchunk = lane & 7;

  // fp16 outputs: bias / scale / activation / LayerNorm fold run on the ACCUMULATOR side, in fp32, before the one
  // rounding to fp16 - the row side only moves 16-B pieces (and adds the fp16 residual).  The earlier form rounded
  // the raw accumulator to fp16, widened it again behind the transposition, did the math there and rounded a second
  // time: five VALU instructions per output pair instead of two, and the epilogue phase of a tile is VALU / LDS-issue
  // time (in-kernel stamps: 4.6 us per qkv tile, 8.6 us per fc1 tile).
  constexpr bool kScaleA = kF16 && (EPI == HCIR_EPI_AFFINE_RELU_F16 || kResidH);
  f32x4 biasA[kF16 ? NTW : 1], scaleA[kScaleA ? NTW : 1];
  bool has_scale = false;
  if constexpr (kF16) {
    has_scale = kScaleA && (EPI == HCIR_EPI_AFFINE_RELU_F16 || g.scale != nullptr);
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int n = nbase + 16 * t + 4 * (lane >> 4);
      biasA[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (g.bias) biasA[t] = *reinterpret_cast<const f32x4*>(g.bias + n);
      if constexpr (kScaleA) {
        scaleA[t] = (f32x4){1.f, 1.f, 1.f, 1.f};
        if (has_scale) scaleA[t] = *reinterpret_cast<const f32x4*>(g.scale + n);
      }
    }
  }
  // fp32 outputs: per-lane bias / scale of every pass on the row side, loaded once, retired once, then laundered.
  // (Flattening these [pass][j] arrays to [pass] reschedules the address arithmetic of the fp32 epilogues.)
  constexpr int NB = kF16 ? 2 : 1;
  f32x4 bias[NPASS][NB], scale[NPASS][NB];
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    if constexpr (kF16) break;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int n = nbase + pass * FPP + rchunk * (kF16 ? 8 : 4) + 4 * j;
      bias[pass][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      scale[pass][j] = (f32x4){1.f, 1.f, 1.f, 1.f};
      if (g.bias) bias[pass][j] = *reinterpret_cast<const f32x4*>(g.bias + n);
      if (kAffine || (EPI == HCIR_EPI_BIAS_RESID_F32 && g.scale))
        scale[pass][j] = *reinterpret_cast<const f32x4*>(g.scale + n);
    }
  }
  // LayerNorm fold, out = rstd[m] (acc - mean[m] c1[n]) + bias[n], all on the accumulator side in fp32: rounding the
  // raw accumulator first loses the result under the cancellation acc - mean c1 when |mean| >> std (measured: 20x
  // the error at mean/std = 50, 2.4x at 5; equal at 0).  mean / rstd of the MTH rows this lane owns, c1 of its features.
  float ln_rs[MTH], ln_mean[MTH];
  f32x4 c1a[NTW];
  if constexpr (kLn) {
#pragma unroll
    for (int mt = 0; mt < MTH; ++mt) {
      int64_t mm = m0w + 16 * mt + (lane & 15);
      mm = mm < g.m ? mm : g.m - 1;
      ln_mean[mt] = g.ln_stats[2 * mm];
      ln_rs[mt] = g.ln_stats[2 * mm + 1];
    }
#pragma unroll
    for (int t = 0; t < NTW; ++t) c1a[t] = *reinterpret_cast<const f32x4*>(g.ln_c1 + nbase + 16 * t + 4 * (lane >> 4));
  }
  // patch embedding: image / patch index of a row of this block, mapped where it is used (a few VALU instructions
  // per row; kept in registers through the epilogue the twelve values spilled the stage offsets of the main loop)
  PatchRowMap rm;
  if constexpr (kPatch) rm = PatchRowMap(m0w, g.m, g.np);
  // (Issuing the next tile's first stage from here, behind these constant loads and with vmcnt(8), instead of from
  // inside the tile's last k-step - so that this wait does not sit out the rest of the stage's round trip - was
  // measured: 3-5 % SLOWER on every shape, tools/ab_gemm.py; like the early-issue main loop, DESIGN.md "GEMM round 2".)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (kLn) {
#pragma unroll
    for (int mt = 0; mt < MTH; ++mt) asm volatile("" : "+v"(ln_rs[mt]));
#pragma unroll
    for (int mt = 0; mt < MTH; ++mt) asm volatile("" : "+v"(ln_mean[mt]));
#pragma unroll
    for (int t = 0; t < NTW; ++t) launder(c1a[t]);
  }
  if constexpr (kF16) {
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      launder(biasA[t]);
      if constexpr (kScaleA) launder(scaleA[t]);
    }
  } else {
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        launder(bias[pass][j]);
        launder(scale[pass][j]);
      }
  }

  // (dual output: every 64-feature pass runs twice through the same wave-private image - first the pre-activation,
  // then its GELU; a wave's LDS operations execute in order, so the second write follows the first pass's reads)
  constexpr int NITER = kDual ? 2 * NPASS : NPASS;
#pragma unroll
  for (int iter = 0; iter < NITER; ++iter) {
    const int pass = kDual ? iter >> 1 : iter;
    const bool second = kDual && (iter & 1);
    // ---- accumulators -> LDS (lane = output row m, registers = features n)
    const int r16 = lane & 15, q16 = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < MTH; ++mt) {
      const int row = mt * 16 + r16;
      if constexpr (kF16) {
        f32x4 posA[kPatch ? 4 : 1];
        if constexpr (kPatch) {
          int bi, pi;
          rm.map(m0w + row, g.m, bi, pi);
          const float* prow = g.pos + (int64_t)(1 + pi) * g.n + nbase + 64 * pass + 4 * q16;
#pragma unroll
          for (int q = 0; q < 4; ++q) posA[q] = *reinterpret_cast<const f32x4*>(prow + 16 * q);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // 64 features per pass = 4 n-tiles of 16
          const int nt = 4 * pass + q;
          f16x4 o;
          float xs[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = acc[nt][mt0 + mt][e];
            const float bb = biasA[nt][e];
            if constexpr (kLn) {
              // out = rstd[m] (acc - mean[m] c1[n]) + bias[n]: centered first (cancellation when |mean| >> std)
              x = __builtin_fmaf(ln_rs[mt], __builtin_fmaf(-ln_mean[mt], c1a[nt][e], x), bb);
            } else if constexpr (EPI == HCIR_EPI_AFFINE_RELU_F16) {
              x = fmaxf(__builtin_fmaf(x, scaleA[nt][e], bb), 0.f);
            } else if constexpr (kResidH) {
              x = scaleA[nt][e] * (x + bb);
            } else if constexpr (kPatch) {
              x = __builtin_fmaf(g.pos_mult, posA[q][e], x + bb);
            } else {
              x += bb;
            }
            xs[e] = x;
          }
          if (kGelu || second) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
              const gelu_f32x2 y = gelu_erf2((gelu_f32x2){xs[e], xs[e + 1]});
              xs[e] = y[0];
              xs[e + 1] = y[1];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (_Float16)xs[e];
          const int chunk = 2 * q + (q16 >> 1);
          *reinterpret_cast<f16x4*>(region + row * 128 + ((chunk ^ (row & 7)) << 4) + 8 * (q16 & 1)) = o;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {   // 32 features per pass = 2 n-tiles of 16
          const int nt = 2 * pass + q;
          const int chunk = 4 * q + q16;
          *reinterpret_cast<f32x4*>(region + row * 128 + ((chunk ^ (row & 7)) << 4)) = acc[nt][mt0 + mt];
        }
      }
    }
    // ---- LDS -> rows: lane = (row rrow + 8 it, 16-B chunk rchunk)
    if constexpr (kF16) {
      const int n = nbase + pass * 64 + rchunk * 8;
#pragma unroll
      for (int it0 = 0; it0 < NIT; it0 += UB) {
        // fp16 residual: the old rows of a group are requested back to back (counted waits).  (Not reading them
        // at all - a timing ablation, wrong results - took proj 237 -> 201 us, fc2 709 -> 686 us at batch 880.
        // Requesting all sixteen pieces of the tile during its last k-step instead (registers freed by keeping the
        // bias in LDS; bit-identical) made proj 3.5 % and fc2 1.3 % SLOWER: the 128 KB a tile reads here go through
        // the same L2 -> CU path as its stages, and that path is what bounds the main loop -
        // profiles/r4_gemm_resid_prefetch.txt)
        f16x8 oldh[UB];
        if constexpr (kResidH) {
#pragma unroll
          for (int u = 0; u < UB; ++u) {
            const int64_t mm = m0w + (it0 + u) * 8 + rrow;
#pragma unroll
            for (int e = 0; e < 8; ++e) oldh[u][e] = (_Float16)0.f;
            if (FULL || mm < g.m)
              oldh[u] = *reinterpret_cast<const f16x8*>(static_cast<const _Float16*>(g.resid) + mm * g.ldo + n);
          }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int row = (it0 + u) * 8 + rrow;
          const f16x8 v = *reinterpret_cast<const f16x8*>(region + row * 128 + ((rchunk ^ (row & 7)) << 4));
          // the image already holds the finished fp16 values; the fp16 residual is one packed add per pair (the
          // exact sum of two fp16 numbers, rounded once)
          f16x8 o;
          if constexpr (kResidH)
            o = v + oldh[u];
          else
            o = v;
          int64_t m = m0w + row;
          const int64_t mrow = m;
          if constexpr (kPatch) {  // the token row: class-token rows lie between the images
            int bi, pi;
            rm.map(m, g.m, bi, pi);
            m = (int64_t)bi * (g.np + 1) + 1 + pi;
          }
          // non-temporal: the 128 KB a workgroup writes per tile would otherwise push the W panels out of the
          // XCD's L2 (W is re-fetched ~50x from the Infinity Cache per qkv launch); +1.4 % end to end
          if (FULL || mrow < g.m)
            __builtin_nontemporal_store(
                o, reinterpret_cast<f16x8*>(static_cast<_Float16*>(second ? g.out2 : g.out) + m * g.ldo + n));
          if constexpr (EPI == EPI_RESID_F16_STATS || kPatch) {
            const f32x2 ss = slice_stats8(o);
            if (rchunk == 0 && (FULL || mrow < g.m) && (!kPatch || g.stats_part)) {
              const int64_t slice = (nbase >> 6) + pass;
              *reinterpret_cast<f32x2*>(g.stats_part + (slice * (g.stats_ld ? g.stats_ld : g.m) + m) * 2) = ss;
            }
          }
        }
      }
    } else {
      const int n = nbase + pass * 32 + rchunk * 4;
      const f32x4 b = bias[pass][0], sc = scale[pass][0];
#pragma unroll
      for (int it0 = 0; it0 < NIT; it0 += UB) {
        // the old-value loads of a group are issued back to back, so their waits are COUNTED
        // (vmcnt(3), ...) and the stores of the previous group stay in flight
        f32x4 oldv[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int64_t mm = m0w + (it0 + u) * 8 + rrow;
          oldv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if constexpr (EPI == HCIR_EPI_BIAS_RESID_F32) {
            if (FULL || mm < g.m)
              oldv[u] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(g.resid) + mm * g.ldo + n);
          }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int row = (it0 + u) * 8 + rrow;
          const int64_t mm = m0w + row;
          f32x4 v = *reinterpret_cast<const f32x4*>(region + row * 128 + ((rchunk ^ (row & 7)) << 4));
          if constexpr (EPI == HCIR_EPI_AFFINE_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(v[e], sc[e], b[e]);
          } else if constexpr (EPI == HCIR_EPI_BIAS_RESID_F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(sc[e], v[e] + b[e], oldv[u][e]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += b[e];
          }
          if (FULL || mm < g.m) *reinterpret_cast<f32x4*>(static_cast<float*>(g.out) + mm * g.ldo + n) = v;
        }
      }
    }
  }
}

// Every wave transposes its accumulator block through a private piece of the LDS slot that the tile's last k-step
// has just released, 128 B of one output row at a time, so that a lane ends up with 16 contiguous bytes of ONE
// output row and 8 lanes cover a whole 128-B line (the direct layout gives every lane 8 B of a different row:
// 1.6-1.9 TB/s effective on the fp16 outputs).  The fp32 outputs take bias / residual on the row-contiguous side.
// [16 MTH rows][128 B] image, 16-B chunks XOR-swizzled with row & 7.
// Full blocks (all 16 MTH rows inside M) take a branch-free path.
template <int EPI, int NTW, int MTT, int MTH, class GA>
__device__ __forceinline__ void gemm_epilogue_lds(const GA& g, const f32x4 (&acc)[NTW][MTT], int mt0,
                                                  char* region, int64_t m0w, int nbase, int lane) {
  // opaque lane id: the epilogue's ~60 loop-invariant LDS / global addresses all derive from it, so hipcc
  // cannot hoist them out of the persistent tile loop into long-lived registers
  asm volatile("" : "+v"(lane));
  if (m0w + 16 * MTH <= g.m)
    gemm_epilogue_lds_impl<EPI, true, NTW, MTT, MTH>(g, acc, mt0, region, m0w, nbase, lane);
  else
    gemm_epilogue_lds_impl<EPI, false, NTW, MTT, MTH>(g, acc, mt0, region, m0w, nbase, lane);
}

template <int EPI, bool GLDS>
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(GemmArgs g, int tiles_n, int tiles_m) {
  using Cfg = GemmCfg;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_n = wave >> 1, wave_m = wave & 1;
  // tile order: n fastest inside a run of one XCD -> the A panel (128 rows x K) stays
  // in that XCD's L2 while the W panels stream through it.
  const int t = xcd_remap(blockIdx.x, tiles_n * tiles_m);
  const int tn = t % tiles_n, tm = t / tiles_n;
  const int n0 = tn * 128;
  const int64_t m0 = (int64_t)tm * 128;
  const int nkc = (g.k + 63) / 64;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  // The tile engine addresses rows as base + row * d: lda == ldw == k is required
  // (checked on the host); "d" is the row length in elements.
  if constexpr (GLDS) {
    // K % 64 == 0: LDS-DMA straight into the double buffer, next stage issued before the MFMAs
    // of the current one; __syncthreads() waits for the DMA (vmcnt) and the barrier.
    sim_stage_glds<_Float16, Cfg>(lds, g.w, n0, g.n - 1, g.a, m0, g.m - 1, g.k, 0, tid);
    for (int kc = 0; kc < nkc; ++kc) {
      const int cur = kc & 1;
      sim_glds_retire_and_sync();  // stage kc landed for every wave; slot cur^1 is free
      if (kc + 1 < nkc)
        sim_stage_glds<_Float16, Cfg>(lds + (cur ^ 1) * Cfg::STAGE_BYTES, g.w, n0, g.n - 1, g.a, m0,
                                      g.m - 1, g.k, kc + 1, tid);
      sim_stage_mfma<_Float16, Cfg, 2>(acc, lds + cur * Cfg::STAGE_BYTES, wave_n, wave_m, lane);
    }
  } else {
    // ragged K: register-staged, zero-filled past K
    u32x4 regs[Cfg::NLOAD];
    sim_stage_load<_Float16, Cfg>(regs, g.w, n0, g.n - 1, g.a, m0, g.m - 1, g.k, 0, tid);
    sim_stage_store<Cfg>(regs, lds, tid);
    __syncthreads();
    for (int kc = 0; kc < nkc; ++kc) {
      const int cur = kc & 1;
      if (kc + 1 < nkc)
        sim_stage_load<_Float16, Cfg>(regs, g.w, n0, g.n - 1, g.a, m0, g.m - 1, g.k, kc + 1, tid);
      sim_stage_mfma<_Float16, Cfg, 2>(acc, lds + cur * Cfg::STAGE_BYTES, wave_n, wave_m, lane);
      if (kc + 1 < nkc) sim_stage_store<Cfg>(regs, lds + (cur ^ 1) * Cfg::STAGE_BYTES, tid);
      __syncthreads();
    }
  }
  gemm_epilogue<EPI>(g, acc, m0, n0, wave_n, wave_m, lane);
}

#ifdef HCIR_DIAG_GSTAMPS
// diagnostic build only (tools/diag_gemm_stamps.py): 100 MHz wall-clock stamps around the SECOND tile of every
// workgroup of the 256 x 256 kernel
__device__ unsigned long long g_gemm_stamps[256 * 8];
#define HCIR_GSTAMP(cond, i)                                                                   \
  do {                                                                                         \
    if ((cond) && threadIdx.x == 0 && blockIdx.x < 256)                                        \
      g_gemm_stamps[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime();                  \
  } while (0)
#else
#define HCIR_GSTAMP(cond, i) \
  do {                       \
  } while (0)
#endif

// (the n-group sizes of the 256 x 256 tile order, kGemmNGroup / kGemmNGroupWide: gemm_stage_addr.h)

// Geometry of a persistent kernel: NT threads as WAVES_N x WAVES_M waves on a TN(n) x TM(m) tile; a stage is TN W
// rows then TM activation rows of 128 B (BK = 64), filled by NLOAD 16-B LDS-DMA pieces per thread, the first NW of
// them W rows (NT * NW == TN * 8: no piece straddles the two operands).
struct G256 {
  static constexpr int NT = 512;
  static constexpr int TN = 256, TM = 256;
  static constexpr int WAVES_N = 2, WAVES_M = 4;   // wave tile 128(n) x 64(m)
  static constexpr int ROWS = TN + TM;             // 256 W rows (n) then 256 activation rows (m)
  static constexpr int STAGE_BYTES = ROWS * 128;   // 64 KB
  static constexpr int NLOAD = ROWS * 8 / NT;      // 16-B pieces per thread per stage = 8 (4 W + 4 activation)
  static constexpr int NW = TN * 8 / NT;           // 4
  static constexpr bool N_GROUPED = true;          // tile order: kGemmNGroup / kGemmNGroupWide
  static_assert(WAVES_N * WAVES_M * 64 == NT && NT * NW == TN * 8, "geometry");
};

struct GMid {
  static constexpr int NT = 256;
  static constexpr int TN = 128, TM = 192;
  static constexpr int WAVES_N = 2, WAVES_M = 2;   // wave tile 64(n) x 96(m), two 48-row halves
  static constexpr int ROWS = TN + TM;             // 128 W rows (n) then 192 activation rows (m)
  static constexpr int STAGE_BYTES = ROWS * 128;   // 40 KB
  static constexpr int NLOAD = ROWS * 8 / NT;      // 10 pieces of 16 B per thread per stage (4 W + 6 activation)
  static constexpr int NW = TN * 8 / NT;           // 4
  static constexpr bool N_GROUPED = false;         // tile order: n fastest
  static_assert(WAVES_N * WAVES_M * 64 == NT && NT * NW == TN * 8, "geometry");
};

// Stage issuer of both persistent kernels: which tiles this workgroup owns, where a tile lies, and the LDS-DMA
// pieces of the next stage to issue (stages run on across tile boundaries).  The kernels keep their own MFMA loops
// and decide where in them the pieces go out.
//
// Source addresses (gemm_stage_addr.h): a thread keeps TWO per-lane byte offsets for the whole kernel, `woff` for
// its W pieces and `aoff` for its activation pieces; everything that changes from piece to piece, k-step to k-step
// and tile to tile is wave-uniform and goes into the transfer's scalar base.  Only a ragged tile (the last row of
// tiles, a_last < TM - 1) computes clamped per-lane offsets, when its activation pieces are issued.  A tile's origin
// is computed ONCE, when the issuer reaches the tile (next_tile), and handed on to the epilogue (origin()).
template <class G>
struct GemmStages {
  // State first, configuration after it: hipcc numbers the loop-carried values in member order (reordering them
  // reschedules the 256 x 256 kernel: compare with tools/cmp_device_asm.py).  All of the state is wave-uniform; the
  // two lane offsets are written once and sit behind the configuration they are made from.
  int issue_kc = 0, issue_ti = 0;  // next stage to issue
  const char* wbase = nullptr;     // W / activation origin of tile issue_ti
  const char* abase = nullptr;
  int a_last = 0;                  // last valid activation row of tile issue_ti, from its first row; at most TM - 1
  // origins of tiles issue_ti, issue_ti - 1, issue_ti - 2: the issuer runs one tile (at one k-step per tile, two)
  // ahead of the tile whose epilogue comes next
  GemmTileOrigins org;
  const GemmArgs& g;
  char* const lds;
  const int tiles_n, tiles_m, tid;
  const int ntiles = tiles_n * tiles_m;
  const int nkc = g.k / 64;
  const int my_tiles =
      (int)blockIdx.x < ntiles ? (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  const int nsteps = my_tiles * nkc;
  const int wave_dst = __builtin_amdgcn_readfirstlane((tid & ~63) * 16);  // the wave's 1 KB of a piece's 8 (NT / 64) KB
  // per-thread DMA source offsets (row tid >> 3 + swizzled chunk), in bytes: 32-bit VGPR offsets on wave-uniform
  // 64-bit bases (global saddr mode); the same for every piece, k-step and tile
  uint32_t woff, aoff;

  __device__ __forceinline__ GemmStages(const GemmArgs& g_, char* lds_, int tiles_n_, int tiles_m_, int tid_)
      : g(g_), lds(lds_), tiles_n(tiles_n_), tiles_m(tiles_m_), tid(tid_) {
    set_lane_offsets();
  }

  // The two lane offsets, from an opaque thread id.  Once per kernel; the one kernel whose epilogue has no register
  // to spare for them (the dual-output epilogue) calls this again behind the epilogue, so that they do not live
  // through it: six instructions.
  __device__ __forceinline__ void set_lane_offsets() {
    int otid = tid;
    asm volatile("" : "+v"(otid));
    woff = gemm_lane_off(otid, g.ldw);
    aoff = gemm_lane_off(otid, g.lda);
  }

  // origin of this workgroup's ti-th tile, from scratch (the issuer itself: next_tile)
  __device__ __forceinline__ void tile_origin(int ti, int& n0, int64_t& m0) const {
    gemm_tile_origin<G::N_GROUPED, G::TN, G::TM>((int)blockIdx.x, (int)gridDim.x, ti, tiles_n, tiles_m, n0, m0);
  }

  // origin of the tile whose epilogue is due: ti == issue_ti - 1, or issue_ti - 2 when every step ends a tile
  __device__ __forceinline__ void origin(int ti, int& n0, int64_t& m0) const {
    int mt;
    org.get(issue_ti - ti, n0, mt);
    m0 = (int64_t)mt * G::TM;
  }

  // the issuer has reached tile issue_ti: its origin and bases; the origins of the two tiles before it move on
  __device__ __forceinline__ void next_tile() {
    org.shift();
    if (issue_ti < my_tiles) {
      int n0;
      int64_t m0;
      tile_origin(issue_ti, n0, m0);
      org.set(n0, (int)(m0 / G::TM));
      wbase = reinterpret_cast<const char*>(g.w + (int64_t)n0 * g.ldw);
      abase = reinterpret_cast<const char*>(g.a + m0 * g.lda);
      a_last = gemm_tile_last_row<G::TM>(g.m, m0);
    }
  }

  __device__ __forceinline__ bool ragged() const { return a_last < G::TM - 1; }

  template <bool RAGGED>
  __device__ __forceinline__ void issue_piece_as(int slot, int i) const {
    // pieces 0..NW-1 are W rows, the rest activation rows (i is a constant after unrolling).  Default cache policy
    // on both operands: `nt` (aux 2) on the activation rows measured +-1 %, on the W rows -9..-13 %
    // (every CU of an XCD re-reads them from L2).  The transfer is issued outside the compiler's view (common.h
    // lds_dma16): +1.3 % over the layer against __builtin_amdgcn_global_load_lds (qkv +2.6 %)
    const uint32_t dst = lds_addr(lds) + slot * G::STAGE_BYTES + wave_dst + G::NT * i * 16;
    // ragged: rows clamped to the matrix, counted from the TILE's first row, from an opaque thread id: nothing of
    // it outlives the piece
    int otid = tid;
    if constexpr (RAGGED) asm volatile("" : "+v"(otid));
    int64_t base;
    uint32_t off;
    gemm_piece_source<G::NT, G::NW, RAGGED>(i, otid, a_last, g.lda, g.ldw, woff, aoff, base, off);
    lds_dma16((i < G::NW ? wbase : abase) + issue_kc * 128 + base, off, dst);
  }

  // pieces i0 .. i0 + cnt - 1 (constants after unrolling); ONE wave-uniform branch where activation rows are among them
  __device__ __forceinline__ void issue_pieces(int slot, int i0, int cnt) const {
    if (i0 + cnt > G::NW && ragged()) {
#pragma unroll
      for (int i = i0; i < i0 + cnt; ++i) issue_piece_as<true>(slot, i);
    } else {
#pragma unroll
      for (int i = i0; i < i0 + cnt; ++i) issue_piece_as<false>(slot, i);
    }
  }

  __device__ __forceinline__ void issue_piece(int slot, int i) const { issue_pieces(slot, i, 1); }

  __device__ __forceinline__ void issue_advance() {
    if (++issue_kc == nkc) {
      issue_kc = 0;
      ++issue_ti;
      next_tile();
    }
  }

  // the whole first stage, into slot 0
  __device__ __forceinline__ void issue_first() {
    if (nsteps > 0) {
      next_tile();
      issue_pieces(0, 0, G::NLOAD);
      issue_advance();
    }
  }
};

// ---------------------------------------------------------------------------
// Big-tile GEMM: 256(n) x 256(m) per workgroup, 8 waves as 2(n) x 4(m), each wave
// 128(n) x 64(m) = 8 x 4 MFMA 16x16x32 tiles (128 accumulator registers), persistent
// over tiles.  Why this geometry (measured, DESIGN.md "GEMM ablation"): with 64 x 64
// wave tiles the LDS pipe (fragment reads + DMA writes, ~170 B/clk of 256) is the limit
// and compute alone tops out at 1.24 PF; 128 x 64 wave tiles cut LDS reads per MFMA by
// 25 % and L2->LDS traffic per flop by 2x.  Rows stay 128 B (BK = 64): with 64-B row
// pieces (BK = 32) the LDS-DMA path moved 2.2-2.8x fewer bytes per second.
//
// A stage is 512 rows x 128 B = 64 KB; two slots.  Step s: wait for stage s (vmcnt(0)),
// barrier, then the eight DMA pieces of stage s+1 are issued between the fragment reads
// and the MFMAs of the FIRST 32-k substep, so that they have the rest of the step (32+
// MFMAs per wave) to land.  Stages run on across tile boundaries: the next tile's first
// stage flies under the epilogue.  Requires K % 64 == 0.
// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_f16_big_kernel(GemmArgs g, int tiles_n, int tiles_m) {
  __shared__ __attribute__((aligned(16))) char lds[2 * G256::STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_n = wave / G256::WAVES_M, wave_m = wave % G256::WAVES_M;
  GemmStages<G256> stg(g, lds, tiles_n, tiles_m, tid);
  const int nkc = stg.nkc, nsteps = stg.nsteps;

  WaveAcc acc;
  acc.zero();

  stg.issue_first();

  int kc = 0, ti = 0;
  for (int step = 0; step < nsteps; ++step) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    HCIR_GSTAMP(ti == 1 && kc == 0, 0);
    HCIR_GSTAMP(ti == 2 && kc == 0, 4);
#ifdef HCIR_DIAG_GSTAMPS
    // shader-clock counter at the same two points: (s_memtime delta) / (s_memrealtime delta) x 100 MHz = the clock
    // the chip holds inside the kernel (MI355X_MICROARCH.md, DVFS give-back item 6)
    if (kc == 0 && (ti == 1 || ti == 2) && threadIdx.x == 0 && blockIdx.x < 256)
      g_gemm_stamps[blockIdx.x * 8 + (ti == 1 ? 6 : 7)] = __builtin_amdgcn_s_memtime();
#endif

    const char* st = lds + (step & 1) * G256::STAGE_BYTES;
    const bool do_issue = step + 1 < nsteps;
    const int islot = (step + 1) & 1;
    // 16x16x32: lane (r16 = lane&15, kq = lane>>4) holds row r16, k = 32*ks2 + 8*kq .. +7
    const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int chunk = 4 * ks2 + kq;
      u32x4 bf[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        bf[mt] = *reinterpret_cast<const u32x4*>(st + sim_slot_off(G256::TN + wave_m * 64 + mt * 16 + r16, chunk));
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        u32x4 af[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          af[q] = *reinterpret_cast<const u32x4*>(
              st + sim_slot_off(wave_n * 128 + (4 * half + q) * 16 + r16, chunk));
        if (do_issue && ks2 == 0) {  // the eight DMA pieces of stage step+1 in the first 32-k substep
          stg.issue_pieces(islot, 4 * half, 4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            acc.a[4 * half + q][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                __builtin_bit_cast(f16x8, af[q]), __builtin_bit_cast(f16x8, bf[mt]), acc.a[4 * half + q][mt],
                0, 0, 0);
      }
    }
    if (do_issue) stg.issue_advance();
    HCIR_GSTAMP(ti == 2 && kc == 0, 5);

    if (++kc == nkc) {
      int n0;
      int64_t m0;
      stg.origin(ti, n0, m0);
      HCIR_GSTAMP(ti == 1, 1);
      // all waves are done reading slot step&1 (their MFMAs have consumed it) after this barrier;
      // the slot stays free until the DMA of stage step+2 is issued behind the next step's barrier.
      // Per wave a private 8 KB piece of it: 64 rows x 128 B.
      __builtin_amdgcn_s_barrier();
      HCIR_GSTAMP(ti == 1, 2);
      gemm_epilogue_lds<EPI, 8, 4, 4>(g, acc.a, 0, lds + (step & 1) * G256::STAGE_BYTES + wave * 8192,
                                      m0 + wave_m * 64, n0 + wave_n * 128, lane);
      HCIR_GSTAMP(ti == 1, 3);
      acc.zero();
      kc = 0;
      ++ti;
      // nothing of the issuer is re-derived here: its two lane offsets are the same for every tile, and the bases and
      // the origin of the tile being issued are scalars (eight per-piece VGPR offsets living through the epilogue
      // were SPILLED in the dual-output variant, and the reload put vmcnt(0) in front of every DMA group)
      if constexpr (EPI == EPI_BIAS_F16_DUAL_GELU) stg.set_lane_offsets();
    }
  }
}

// ---------------------------------------------------------------------------
// Mid-tile GEMM: 128(n) x 192(m) per workgroup of FOUR waves (2 x 2, wave tile 64 x 96 = 4 x 6 MFMA 16x16x32
// tiles, 96 accumulator registers), 2 x 40 KB LDS slots -> TWO workgroups per CU (2 x 80 KB = the CU's 160 KB).
//
// Why: the 256 x 256 kernel runs ONE workgroup per CU, so a CU's matrix pipes idle for the whole epilogue of
// every tile (22 % of the launch at K = 768: LDS transposition, bias / GELU / LayerNorm-fold math, 128 KB of
// stores per tile, all CUs at the same moment).  Two independent workgroups per CU fall into anti-phase by
// themselves: while one transposes and stores, the other owns the matrix pipes, and the output bursts of a CU
// (and of the chip) spread over the tile time.  Price: 1.67 x the L2->LDS bytes per flop of the 256^2 tile and
// 10 instead of 12 fragment reads per 24 instead of 32 MFMAs (+11 % LDS reads per MFMA).
// Same staging (GemmStages: LDS-DMA, 128-B rows, XOR swizzle), same MFMA operand maps and k order as the 256^2
// kernel, the same epilogue (gemm_epilogue_lds): results are bit-identical to it.  Requires K % 64 == 0, N % 128 == 0.
// ---------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f16_mid_kernel(GemmArgs g, int tiles_n, int tiles_m) {
  __shared__ __attribute__((aligned(16))) char lds[2 * GMid::STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_n = wave / GMid::WAVES_M, wave_m = wave % GMid::WAVES_M;
  GemmStages<GMid> stg(g, lds, tiles_n, tiles_m, tid);
  const int nkc = stg.nkc, nsteps = stg.nsteps;

  f32x4 acc[4][6];
  auto zero_acc = [&]() {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 6; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  zero_acc();

  stg.issue_first();

  const int r16 = lane & 15, kq = lane >> 4;
  int kc = 0, ti = 0;
  for (int step = 0; step < nsteps; ++step) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const char* st = lds + (step & 1) * GMid::STAGE_BYTES;
    const bool do_issue = step + 1 < nsteps;
    const int islot = (step + 1) & 1;
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int chunk = 4 * ks2 + kq;
      u32x4 bf[6], af[4];
#pragma unroll
      for (int mt = 0; mt < 6; ++mt)
        bf[mt] = *reinterpret_cast<const u32x4*>(st + sim_slot_off(GMid::TN + wave_m * 96 + mt * 16 + r16, chunk));
#pragma unroll
      for (int q = 0; q < 4; ++q)
        af[q] = *reinterpret_cast<const u32x4*>(st + sim_slot_off(wave_n * 64 + q * 16 + r16, chunk));
#pragma unroll
      for (int hq = 0; hq < 2; ++hq) {
        if (do_issue && ks2 == 0) {  // the ten DMA pieces of stage step+1 in the first 32-k substep
          stg.issue_pieces(islot, 5 * hq, 5);
        }
#pragma unroll
        for (int q = 2 * hq; q < 2 * hq + 2; ++q)
#pragma unroll
          for (int mt = 0; mt < 6; ++mt)
            acc[q][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, af[q]),
                                                               __builtin_bit_cast(f16x8, bf[mt]), acc[q][mt], 0, 0, 0);
      }
    }
    if (do_issue) stg.issue_advance();

    if (++kc == nkc) {
      int n0;
      int64_t m0;
      stg.origin(ti, n0, m0);
      // every wave is done reading slot step&1; it stays free until the DMA of stage step+2 goes out behind the
      // next step's barrier.  Per wave a private 6 KB piece of it: 48 rows x 128 B, two row halves per tile.
      __builtin_amdgcn_s_barrier();
      char* region = lds + (step & 1) * GMid::STAGE_BYTES + wave * 6144;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        gemm_epilogue_lds<EPI, 4, 6, 3>(g, acc, 3 * hh, region, m0 + wave_m * 96 + hh * 48, n0 + wave_n * 64, lane);
      zero_acc();
      kc = 0;
      ++ti;
    }
  }
}

// ---------------------------------------------------------------------------
// Patch embedding: Conv2d(C, D, P, P) as a GEMM whose A operand is gathered from
// the fp32 NCHW image on the fly (no im2col buffer), P == 16.
//   k = c*256 + ky*16 + kx ; a 64-wide k chunk = 4 image rows of one channel;
//   a 16-B LDS slot = 8 consecutive pixels of one row (32 B of fp32 source).
// ---------------------------------------------------------------------------
struct PatchArgs {
  int p, kreal, kpad;  // patch size, C*P*P, row length of the (zero-padded) weight matrix
  const float* img;
  const _Float16* w;
  const float* bias;
  const float* pos;
  void* tok;
  int64_t b;
  int c, h, w_px, gh, gw, d;
  float pos_mult;
};

template <typename TokT, bool P16>
__global__ __launch_bounds__(256) void patch_embed_kernel(PatchArgs p, int tiles_n, int tiles_m) {
  using Cfg = GemmCfg;
  __shared__ __attribute__((aligned(16))) char lds[Cfg::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_n = wave >> 1, wave_m = wave & 1;
  const int t = xcd_remap(blockIdx.x, tiles_n * tiles_m);
  const int tn = t % tiles_n, tm = t / tiles_n;
  const int n0 = tn * 128;
  const int64_t m0 = (int64_t)tm * 128;
  const int np = p.gh * p.gw;
  const int64_t mtot = p.b * np;
  const int kdim = p.kpad;
  const int nkc = kdim / 64;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  u32x4 regs[Cfg::NLOAD];
  auto load = [&](int kc) {
#pragma unroll
    for (int i = 0; i < Cfg::NLOAD; ++i) {
      const int slot = tid + 256 * i;
      const int row = slot >> 3, chunk = slot & 7;
      const int k0 = kc * 64 + chunk * 8;
      if (row < Cfg::GM) {
        int nr = n0 + row;
        nr = nr > p.d - 1 ? p.d - 1 : nr;
        regs[i] = *reinterpret_cast<const u32x4*>(p.w + (int64_t)nr * kdim + k0);
      } else {
        int64_t m = m0 + (row - Cfg::GM);
        m = m > mtot - 1 ? mtot - 1 : m;
        const int64_t bi = m / np;
        const int pi = (int)(m % np);
        const int py = pi / p.gw, px = pi % p.gw;
        f16x8 v;
        if constexpr (P16) {
          const int c = k0 >> 8, ky = (k0 >> 4) & 15, kx = k0 & 15;
          const float* src = p.img + ((bi * p.c + c) * p.h + (py * 16 + ky)) * (int64_t)p.w_px + px * 16 + kx;
          const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = (_Float16)lo[e];
            v[4 + e] = (_Float16)hi[e];
          }
        } else {
          // any patch size: k = (c * P + ky) * P + kx, element by element, zero past C*P*P
          const int pp = p.p * p.p;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            float x = 0.f;
            if (k < p.kreal) {
              const int c = k / pp, rem = k - c * pp;
              const int ky = rem / p.p, kx = rem - ky * p.p;
              x = p.img[((bi * p.c + c) * p.h + (py * p.p + ky)) * (int64_t)p.w_px + px * p.p + kx];
            }
            v[e] = (_Float16)x;
          }
        }
        regs[i] = __builtin_bit_cast(u32x4, v);
      }
    }
  };
  load(0);
  sim_stage_store<Cfg>(regs, lds, tid);
  __syncthreads();
  for (int kc = 0; kc < nkc; ++kc) {
    const int cur = kc & 1;
    if (kc + 1 < nkc) load(kc + 1);
    sim_stage_mfma<_Float16, Cfg, 2>(acc, lds + cur * Cfg::STAGE_BYTES, wave_n, wave_m, lane);
    if (kc + 1 < nkc) sim_stage_store<Cfg>(regs, lds + (cur ^ 1) * Cfg::STAGE_BYTES, tid);
    __syncthreads();
  }
  // epilogue: tok[b][1 + p][n] = acc + bias[n] + pos_mult * pos[1 + p][n]
  const int r = lane & 31, h = lane >> 5;
  if constexpr (sizeof(TokT) == 2) {
    // fp16 token rows: the wave transposes its 64 x 64 tile through 8 KB of the (now idle) stage buffers and
    // stores whole 128-B lines; the direct layout below writes 8 B of 32 different rows per instruction
    // (the same fix took 13 % off the attention kernel)
    char* ot = lds + wave * 8192;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int row = mt * 32 + r;
      int64_t m = m0 + wave_m * 64 + row;
      m = m < mtot ? m : mtot - 1;
      const float* prow = p.pos + (int64_t)(1 + (int)(m % np)) * p.d;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
          int n = n0 + wave_n * 64 + nt * 32 + 8 * grp + 4 * h;
          n = n < p.d ? n : p.d - 4;  // (d is a multiple of 8: a clamped read, the column is not stored)
          const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n);
          const f32x4 ps = *reinterpret_cast<const f32x4*>(prow + n);
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (_Float16)(acc[nt][mt][4 * grp + e] + b[e] + p.pos_mult * ps[e]);
          *reinterpret_cast<f16x4*>(ot + row * 128 + (((4 * nt + grp) ^ (row & 7)) << 4) + 8 * h) = o;
        }
      }
    }
    const int rr = lane >> 3, cc = lane & 7;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = it * 8 + rr;
      const int64_t m = m0 + wave_m * 64 + row;
      const int n = n0 + wave_n * 64 + cc * 8;
      const u32x4 v = *reinterpret_cast<const u32x4*>(ot + row * 128 + ((cc ^ (row & 7)) << 4));
      if (m < mtot && n < p.d) {
        const int64_t bi = m / np;
        const int pi = (int)(m % np);
        *reinterpret_cast<u32x4*>(static_cast<_Float16*>(p.tok) + (bi * (np + 1) + 1 + pi) * (int64_t)p.d + n) = v;
      }
    }
    return;
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int64_t m = m0 + wave_m * 64 + mt * 32 + r;
    if (m >= mtot) continue;
    const int64_t bi = m / np;
    const int pi = (int)(m % np);
    TokT* orow = static_cast<TokT*>(p.tok) + (bi * (np + 1) + 1 + pi) * (int64_t)p.d;
    const float* prow = p.pos + (int64_t)(1 + pi) * p.d;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        const int n = n0 + wave_n * 64 + nt * 32 + 8 * grp + 4 * h;
        if (n >= p.d) continue;
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n);
        const f32x4 ps = *reinterpret_cast<const f32x4*>(prow + n);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[nt][mt][4 * grp + e] + b[e] + p.pos_mult * ps[e];
        if constexpr (sizeof(TokT) == 4) {
          *reinterpret_cast<f32x4*>(orow + n) = v;
        } else {
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (_Float16)v[e];
          *reinterpret_cast<f16x4*>(orow + n) = o;
        }
      }
    }
  }
}

template <typename TokT>
__global__ void cls_row_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                               float pos_mult, int64_t b, int t, int d, TokT* __restrict__ tok) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b * d) return;
  const int64_t bi = i / d;
  const int n = (int)(i % d);
  tok[bi * t * (int64_t)d + n] = (TokT)(cls[n] + pos_mult * pos[n]);
}

// ---------------------------------------------------------------------------
// Patch embedding on the persistent 256 x 256 tile engine (hcir_patch_embed_fused; route: patch_plan.h): the geometry,
// LDS image, MFMA loop, tile order and epilogue body of gemm_f16_big_kernel.  The W rows of a stage go by LDS-DMA
// exactly as GemmStages issues them; the activation rows have no fp16 source to transfer, so every thread GATHERS its
// four 16-B slots (8 pixels of one image row = two f32x4 loads each) from the fp32 NCHW image into registers one stage
// ahead - where the DMA pieces go out - and converts and writes them into the next slot behind the step's MFMAs.
// With d / 256 n-tiles the image is read from L2 and converted d / 256 times (ViT-B: 3) instead of d / 128 times.
// GEMM view: m = b * np patch rows, n = d, k = c * 256; out row = token row (EPI_PATCH_F16_STATS).
// ---------------------------------------------------------------------------
struct PatchGemmArgs : GemmArgs {
  const float* img;
  const float* pos;
  float pos_mult;
  int np, gw, c, h, w_px;
};

__global__ __launch_bounds__(512, 2) void patch_embed_big_kernel(PatchGemmArgs g, int tiles_n, int tiles_m) {
  __shared__ __attribute__((aligned(16))) char lds[2 * G256::STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_n = wave / G256::WAVES_M, wave_m = wave % G256::WAVES_M;
  GemmStages<G256> stg(g, lds, tiles_n, tiles_m, tid);
  const int nkc = stg.nkc, nsteps = stg.nsteps;
  constexpr int NA = G256::NLOAD - G256::NW;  // activation slots per thread and stage: rows (tid >> 3) + 64 i, chunk tid & 7

  // image origin of the NA patch rows this thread gathers for the tile being issued: channel 0, the patch's image
  // row ky = chunk >> 1 (a 64-wide k chunk is image rows 4 (kc & 3) .. + 3 of channel kc >> 2), column 8 (chunk & 1);
  // 32-bit byte offsets from the image of the tile's first row (wave-uniform; patch_plan.h bounds a tile's span)
  const char* ibase = nullptr;
  uint32_t aoff[NA];
  auto set_rows = [&](int t_i) {
    int n0;
    int64_t m0;
    stg.tile_origin(t_i, n0, m0);
    int otid = tid;
    asm volatile("" : "+v"(otid));  // (opaque: nothing of this hoisted out of the tile loop)
    const int chunk = otid & 7;
    const int bfirst = (int)m0 / g.np;  // (patch_plan.h: b * T < 2^31; m0 < M)
    ibase = reinterpret_cast<const char*>(g.img + (int64_t)bfirst * g.c * g.h * g.w_px);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      int64_t m = m0 + (otid >> 3) + 64 * i;
      m = m < g.m ? m : g.m - 1;
      const int mi = (int)m;
      const int bi = mi / g.np, pi = mi - bi * g.np;
      const int py = pi / g.gw, px = pi - py * g.gw;
      aoff[i] = (uint32_t)((((bi - bfirst) * g.c * g.h + py * 16 + (chunk >> 1)) * g.w_px + px * 16 + 8 * (chunk & 1)) * 4);
    }
  };
  f32x4 stage_a[2 * NA];
  auto gather_load = [&](int kc) {
    const char* kbase = ibase + ((int64_t)(kc >> 2) * g.h + 4 * (kc & 3)) * g.w_px * 4;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      stage_a[2 * i] = *reinterpret_cast<const f32x4*>(kbase + aoff[i]);
      stage_a[2 * i + 1] = *reinterpret_cast<const f32x4*>(kbase + aoff[i] + 16);
    }
  };
  auto gather_store = [&](int slot) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      f16x8 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (_Float16)stage_a[2 * i][e];
        v[4 + e] = (_Float16)stage_a[2 * i + 1][e];
      }
      *reinterpret_cast<f16x8*>(lds + slot * G256::STAGE_BYTES + sim_slot_off(G256::TN + (tid >> 3) + 64 * i, tid & 7)) = v;
    }
  };

  WaveAcc acc;
  acc.zero();

  if (nsteps > 0) {  // the whole first stage, into slot 0
    stg.next_tile();
    set_rows(0);
    gather_load(0);
#pragma unroll
    for (int i = 0; i < G256::NW; ++i) stg.issue_piece(0, i);
    gather_store(0);
    stg.issue_advance();
    if (stg.issue_kc == 0 && stg.issue_ti < stg.my_tiles) set_rows(stg.issue_ti);
  }

  int kc = 0, ti = 0;
  for (int step = 0; step < nsteps; ++step) {
    // stage `step` has landed: the W pieces (DMA) and every wave's converted activation slots (LDS writes)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const char* st = lds + (step & 1) * G256::STAGE_BYTES;
    const bool do_issue = step + 1 < nsteps;
    const int islot = (step + 1) & 1;
    const int r16 = lane & 15, kq = lane >> 4;
    if (do_issue) gather_load(stg.issue_kc);  // in flight under the whole step
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int chunk = 4 * ks2 + kq;
      u32x4 bf[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        bf[mt] = *reinterpret_cast<const u32x4*>(st + sim_slot_off(G256::TN + wave_m * 64 + mt * 16 + r16, chunk));
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        u32x4 af[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          af[q] = *reinterpret_cast<const u32x4*>(
              st + sim_slot_off(wave_n * 128 + (4 * half + q) * 16 + r16, chunk));
        if (do_issue && ks2 == 0 && half == 0) {  // the four W pieces of stage step+1
#pragma unroll
          for (int i = 0; i < G256::NW; ++i) stg.issue_piece(islot, i);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            acc.a[4 * half + q][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                __builtin_bit_cast(f16x8, af[q]), __builtin_bit_cast(f16x8, bf[mt]), acc.a[4 * half + q][mt],
                0, 0, 0);
      }
    }
    if (do_issue) {
      // slot islot was last read in step - 1: every wave has passed this step's barrier since
      gather_store(islot);
      stg.issue_advance();
      if (stg.issue_kc == 0 && stg.issue_ti < stg.my_tiles) set_rows(stg.issue_ti);
    }

    if (++kc == nkc) {
      int n0;
      int64_t m0;
      stg.tile_origin(ti, n0, m0);
      // as gemm_f16_big_kernel: slot step&1 is free after this barrier, 8 KB of it per wave.  Rows are counted from
      // the TILE's first row (m0 + 64 wave_m may lie past M on the ragged tile: the epilogue clamps before it maps)
      __builtin_amdgcn_s_barrier();
      gemm_epilogue_lds<EPI_PATCH_F16_STATS, 8, 4, 4>(g, acc.a, 0, lds + (step & 1) * G256::STAGE_BYTES + wave * 8192,
                                                      m0 + wave_m * 64, n0 + wave_n * 128, lane);
      acc.zero();
      kc = 0;
      ++ti;
      if (stg.issue_ti < stg.my_tiles) set_rows(stg.issue_ti);
    }
  }
}

// Class-token rows of hcir_patch_embed_fused: tok[bi][0] = fp16(cls + pos_mult pos[0]) and the slice statistics of the
// stored values; one thread per 8 features, the 8 lanes of a 64-feature slice side by side (slice_stats8).  d % 64 == 0.
__global__ __launch_bounds__(256) void cls_row_stats_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                            float pos_mult, int64_t b, int t, int d,
                                                            _Float16* __restrict__ tok, float* __restrict__ stats_part) {
  const int per = d >> 3;
  const int64_t total = b * per;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool inside = i < total;
  i = inside ? i : total - 1;  // (every lane of a wave takes part in the 8-lane sums)
  const int64_t bi = i / per;
  const int n = (int)(i - bi * per) * 8;
  f16x8 o;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x4 cv = *reinterpret_cast<const f32x4*>(cls + n + 4 * j);
    const f32x4 pv = *reinterpret_cast<const f32x4*>(pos + n + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[4 * j + e] = (_Float16)__builtin_fmaf(pos_mult, pv[e], cv[e]);
  }
  const f32x2 ss = slice_stats8(o);
  if (!inside) return;
  const int64_t row = bi * t;
  *reinterpret_cast<f16x8*>(tok + row * d + n) = o;
  if (stats_part && (threadIdx.x & 7) == 0)
    *reinterpret_cast<f32x2*>(stats_part + ((int64_t)(n >> 6) * (b * t) + row) * 2) = ss;
}

// (mean, M2) of the 64-feature slices of hcir_gemm_f16_fused -> (mean, rstd) per row by Chan's parallel-variance
// combination (equal slice sizes), slices visited in index order: deterministic, no cancellation
__global__ void ln_stats_finalize_kernel(const float* __restrict__ part, int parts, int64_t m, float slice_n,
                                         float eps, float* __restrict__ stats) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= m) return;
  float ms = 0.f;
  for (int p = 0; p < parts; ++p) ms += part[((int64_t)p * m + row) * 2];
  const float mean = ms / (float)parts;
  float m2 = 0.f;
  for (int p = 0; p < parts; ++p) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(part + ((int64_t)p * m + row) * 2);
    const float dm = v[0] - mean;
    m2 += v[1] + slice_n * dm * dm;
  }
  const float var = m2 / (slice_n * (float)parts);
  *reinterpret_cast<f32x2*>(stats + 2 * row) = (f32x2){mean, 1.0f / sqrtf(var + eps)};
}

// Which kernel a launch takes: gemm_plan.h.
template <int EPI>
void launch_gemm_mid(const GemmArgs& g, hipStream_t st) {
  const int tn = g.n / GMid::TN, tm = (int)hcir_cdiv(g.m, GMid::TM);
  const int grid = tn * tm < 512 ? tn * tm : 512;  // persistent: two workgroups per CU
  hipLaunchKernelGGL((gemm_f16_mid_kernel<EPI>), dim3(grid), dim3(GMid::NT), 0, st, g, tn, tm);
}

// The 256 x 256 persistent kernel over tn x tm tiles
template <int EPI>
void launch_big_tiles(const GemmArgs& g, int tn, int tm, hipStream_t st) {
  const int grid = tn * tm < 256 ? tn * tm : 256;  // persistent: one workgroup per CU
  hipLaunchKernelGGL((gemm_f16_big_kernel<EPI>), dim3(grid), dim3(G256::NT), 0, st, g, tn, tm);
}

template <int EPI>
void launch_gemm_big(const GemmArgs& g, const GemmPlan& p, hipStream_t st) {
  // (the dual-output epilogue exists on the 256 x 256 kernel only: gemm_plan never sends it elsewhere)
  if constexpr (EPI != EPI_BIAS_F16_DUAL_GELU) {
    if (p.route == HCIR_GEMM_ROUTE_SPLIT) {
      // pointers advanced to the row range; the per-row statistics keep the full matrix's slice pitch
      const int64_t m1 = p.m1;
      GemmArgs g1 = g, g2 = g;
      g1.m = m1;
      g1.stats_ld = g.stats_ld ? g.stats_ld : g.m;
      g2.m = g.m - m1;
      g2.stats_ld = g1.stats_ld;
      g2.a = g.a + m1 * g.lda;
      const bool f32out = EPI == HCIR_EPI_BIAS_RESID_F32 || EPI == HCIR_EPI_BIAS_F32 || EPI == HCIR_EPI_AFFINE_F32;
      const int64_t obytes = m1 * g.ldo * (f32out ? 4 : 2);
      g2.out = static_cast<char*>(g.out) + obytes;
      if (g.resid) g2.resid = static_cast<const char*>(g.resid) + obytes;
      if (g.ln_stats) g2.ln_stats = g.ln_stats + 2 * m1;
      if (g.stats_part) g2.stats_part = g.stats_part + 2 * m1;
      launch_big_tiles<EPI>(g1, p.tn, p.tm1, st);
      launch_gemm_mid<EPI>(g2, st);
      return;
    }
    if (p.route == HCIR_GEMM_ROUTE_MID) {
      launch_gemm_mid<EPI>(g, st);
      return;
    }
  }
  launch_big_tiles<EPI>(g, p.tn, p.tm, st);
}

template <int EPI>
void launch_gemm(const GemmArgs& g, hipStream_t st) {
  const GemmPlan p = gemm_plan(g.m, g.n, g.k, EPI == EPI_BIAS_F16_DUAL_GELU);
  if (p.route != HCIR_GEMM_ROUTE_SMALL) {
    launch_gemm_big<EPI>(g, p, st);
    return;
  }
  if (g.k % 64 == 0)
    hipLaunchKernelGGL((gemm_f16_kernel<EPI, true>), dim3(p.tn * p.tm), dim3(256), 0, st, g, p.tn, p.tm);
  else
    hipLaunchKernelGGL((gemm_f16_kernel<EPI, false>), dim3(p.tn * p.tm), dim3(256), 0, st, g, p.tn, p.tm);
}

}  // namespace

extern "C" {

int hcir_gemm_f16(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                  const float* scale, int64_t m, int32_t n, int32_t k, int epilogue, void* out,
                  int64_t ldo, void* stream) {
  return hcir_gemm_f16_resid(a, lda, w, ldw, bias, scale, m, n, k, epilogue, nullptr, out, ldo, stream);
}

int hcir_gemm_f16_resid(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                        const float* scale, int64_t m, int32_t n, int32_t k, int epilogue, const void* resid,
                        void* out, int64_t ldo, void* stream) {
  HCIR_ENTER();
  if (resid && epilogue != HCIR_EPI_BIAS_RESID_F16 && epilogue != HCIR_EPI_BIAS_RESID_F32) return HCIR_ERR_INVALID;
  if (!a || !w || !out || m <= 0 || n <= 0 || k <= 0) return HCIR_ERR_INVALID;
  if ((k & 7) || (n & 7) || lda < k || ldw < k || (lda & 7) || (ldw & 7) || ldo < n || (ldo & 3))
    return HCIR_ERR_INVALID;
  // fp16 outputs of the persistent kernels are stored as 16-byte pieces of a row
  const bool f16out = epilogue == HCIR_EPI_BIAS_F16 || epilogue == HCIR_EPI_BIAS_GELU_F16 ||
                      epilogue == HCIR_EPI_AFFINE_RELU_F16 || epilogue == HCIR_EPI_BIAS_RESID_F16;
  if (f16out && gemm_takes_big(m, n, k) && (ldo & 7)) return HCIR_ERR_INVALID;
  // row pitches other than k: only the 256x256 persistent kernel carries separate pitches
  if ((lda != k || ldw != k) && !gemm_takes_big(m, n, k)) return HCIR_ERR_UNSUPPORTED;
  if ((epilogue == HCIR_EPI_AFFINE_RELU_F16 || epilogue == HCIR_EPI_AFFINE_F32) && !scale)
    return HCIR_ERR_INVALID;
  if (hcir_cdiv(m, 128) * hcir_cdiv(n, 128) > 0x7fffffff) return HCIR_ERR_INVALID;
  GemmArgs g{static_cast<const _Float16*>(a), static_cast<const _Float16*>(w), bias, scale, out, m,
             lda, ldw, ldo, n, k, nullptr, nullptr, nullptr, resid ? resid : out, nullptr};
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (epilogue) {
    case HCIR_EPI_BIAS_F16: launch_gemm<HCIR_EPI_BIAS_F16>(g, st); break;
    case HCIR_EPI_BIAS_GELU_F16: launch_gemm<HCIR_EPI_BIAS_GELU_F16>(g, st); break;
    case HCIR_EPI_BIAS_RESID_F32: launch_gemm<HCIR_EPI_BIAS_RESID_F32>(g, st); break;
    case HCIR_EPI_BIAS_F32: launch_gemm<HCIR_EPI_BIAS_F32>(g, st); break;
    case HCIR_EPI_AFFINE_RELU_F16: launch_gemm<HCIR_EPI_AFFINE_RELU_F16>(g, st); break;
    case HCIR_EPI_AFFINE_F32: launch_gemm<HCIR_EPI_AFFINE_F32>(g, st); break;
    case HCIR_EPI_BIAS_RESID_F16: launch_gemm<HCIR_EPI_BIAS_RESID_F16>(g, st); break;
    default: return HCIR_ERR_UNSUPPORTED;
  }
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_gemm_f16_gelu_dual(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m,
                            int32_t n, int32_t k, void* out_pre, void* out_act, int64_t ldo, void* stream) {
  HCIR_ENTER();
  if (!a || !w || !out_pre || !out_act || m <= 0 || n <= 0 || k <= 0) return HCIR_ERR_INVALID;
  if (lda < k || ldw < k || (lda & 7) || (ldw & 7) || ldo < n || (ldo & 7)) return HCIR_ERR_INVALID;
  if (!gemm_takes_big(m, n, k)) return HCIR_ERR_UNSUPPORTED;
  GemmArgs g{static_cast<const _Float16*>(a), static_cast<const _Float16*>(w), bias, nullptr, out_pre, m,
             lda, ldw, ldo, n, k, nullptr, nullptr, nullptr, out_pre, out_act};
  launch_gemm_big<EPI_BIAS_F16_DUAL_GELU>(g, gemm_plan(m, n, k, true), static_cast<hipStream_t>(stream));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

#ifdef HCIR_DIAG_GSTAMPS
int hcir_debug_gemm_stamps(unsigned long long* host_dst) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_gemm_stamps), sizeof(unsigned long long) * 256 * 8);
}
#endif

int hcir_gemm_fused_supported(int64_t m, int32_t n, int32_t k) { return gemm_takes_big(m, n, k) ? 1 : 0; }

int32_t hcir_gemm_stats_slices(int32_t n) { return n / 64; }

int hcir_gemm_route(int64_t m, int32_t n, int32_t k, int epilogue, int64_t* rows_on_big) {
  if (m <= 0 || n <= 0 || k <= 0 || (k & 7) || (n & 7)) return HCIR_ERR_INVALID;
  if (epilogue < HCIR_EPI_BIAS_F16 || (epilogue > HCIR_EPI_BIAS_RESID_F16 && epilogue != HCIR_GEMM_ROUTE_EPI_DUAL))
    return HCIR_ERR_INVALID;
  const GemmPlan p = gemm_plan(m, n, k, epilogue == HCIR_GEMM_ROUTE_EPI_DUAL);
  if (rows_on_big) *rows_on_big = p.m1;
  return p.route;
}

int hcir_gemm_f16_fused(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                        const float* scale, int64_t m, int32_t n, int32_t k, int epilogue, void* out,
                        int64_t ldo, const float* ln_stats, const float* ln_c1, float* stats_part,
                        void* stream) {
  HCIR_ENTER();
  if (!a || !w || !out || m <= 0 || n <= 0 || k <= 0) return HCIR_ERR_INVALID;
  if ((k & 7) || (n & 7) || lda < k || ldw < k || (lda & 7) || (ldw & 7) || ldo < n || (ldo & 7))
    return HCIR_ERR_INVALID;
  const bool ln = ln_stats || ln_c1;
  if (ln && (!ln_stats || !ln_c1 || !bias)) return HCIR_ERR_INVALID;
  if (ln && stats_part) return HCIR_ERR_INVALID;
  if (!ln && !stats_part) return HCIR_ERR_INVALID;  // nothing fused: use hcir_gemm_f16
  if (ln && epilogue != HCIR_EPI_BIAS_F16 && epilogue != HCIR_EPI_BIAS_GELU_F16) return HCIR_ERR_UNSUPPORTED;
  if (stats_part && epilogue != HCIR_EPI_BIAS_RESID_F16) return HCIR_ERR_UNSUPPORTED;
  if (!gemm_takes_big(m, n, k)) return HCIR_ERR_UNSUPPORTED;
  GemmArgs g{static_cast<const _Float16*>(a), static_cast<const _Float16*>(w), bias, scale, out, m,
             lda, ldw, ldo, n, k, ln_stats, ln_c1, stats_part, out, nullptr};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const GemmPlan p = gemm_plan(m, n, k, false);
  if (stats_part) launch_gemm_big<EPI_RESID_F16_STATS>(g, p, st);
  else if (epilogue == HCIR_EPI_BIAS_F16) launch_gemm_big<EPI_LN_BIAS_F16>(g, p, st);
  else launch_gemm_big<EPI_LN_BIAS_GELU_F16>(g, p, st);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_gemm_f16_ln_rows(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m,
                          int32_t n, int32_t k, void* out, int64_t ldo, const float* ln_stats, const float* ln_c1,
                          void* stream) {
  HCIR_ENTER();
  if (!a || !w || !out || !bias || !ln_stats || !ln_c1 || m <= 0 || n <= 0 || k <= 0) return HCIR_ERR_INVALID;
  if (lda < k || ldw < k || (lda & 7) || (ldw & 7) || ldo < n || (ldo & 7)) return HCIR_ERR_INVALID;
  if (k % 64 || n % GMid::TN) return HCIR_ERR_UNSUPPORTED;
  if ((n / GMid::TN) * hcir_cdiv(m, GMid::TM) > 0x7fffffff) return HCIR_ERR_INVALID;
  GemmArgs g{static_cast<const _Float16*>(a), static_cast<const _Float16*>(w), bias, nullptr, out, m,
             lda, ldw, ldo, n, k, ln_stats, ln_c1, nullptr, out, nullptr};
  launch_gemm_mid<EPI_LN_BIAS_F16>(g, static_cast<hipStream_t>(stream));
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_ln_stats_finalize(const float* stats_part, int32_t slices, int64_t m, int32_t n_features, float eps,
                           float* ln_stats, void* stream) {
  HCIR_ENTER();
  if (!stats_part || !ln_stats || slices <= 0 || m <= 0 || n_features <= 0) return HCIR_ERR_INVALID;
  if ((int64_t)slices * 64 != n_features) return HCIR_ERR_INVALID;  // slices are 64 features wide
  hipLaunchKernelGGL(ln_stats_finalize_kernel, dim3((unsigned)hcir_cdiv(m, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), stats_part, slices, m, 64.0f, eps, ln_stats);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_patch_embed(const float* img, int64_t b, int32_t c, int32_t h, int32_t w_px, int32_t p,
                     const void* w_f16, int64_t ldw, const float* bias, const float* cls,
                     const float* pos, float pos_mult, int32_t d, void* tok, int tok_dtype,
                     void* stream) {
  HCIR_ENTER();
  if (!img || !w_f16 || !bias || !cls || !pos || !tok || b <= 0) return HCIR_ERR_INVALID;
  if (p <= 0 || p > 32 || c <= 0 || h % p || w_px % p || (d & 7)) return HCIR_ERR_INVALID;
  const int kreal = c * p * p;
  if (ldw < kreal || (ldw & 63)) return HCIR_ERR_INVALID;  // weight rows zero-padded to a multiple of 64
  PatchArgs a{p, kreal, (int)ldw, img, static_cast<const _Float16*>(w_f16), bias, pos, tok, b, c, h, w_px,
              h / p, w_px / p, d, pos_mult};
  const int np = a.gh * a.gw;
  const int tiles_n = (int)hcir_cdiv(d, 128), tiles_m = (int)hcir_cdiv(b * np, 128);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (tok_dtype != HCIR_F32 && tok_dtype != HCIR_F16) return HCIR_ERR_UNSUPPORTED;
  const dim3 cgrid((unsigned)hcir_cdiv(b * d, 256));
  if (tok_dtype == HCIR_F32) {
    if (p == 16)
      hipLaunchKernelGGL((patch_embed_kernel<float, true>), dim3(tiles_n * tiles_m), dim3(256), 0, st, a, tiles_n, tiles_m);
    else
      hipLaunchKernelGGL((patch_embed_kernel<float, false>), dim3(tiles_n * tiles_m), dim3(256), 0, st, a, tiles_n, tiles_m);
    HCIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_row_kernel<float>, cgrid, dim3(256), 0, st, cls, pos, pos_mult, b, np + 1, d,
                       static_cast<float*>(tok));
  } else {
    if (p == 16)
      hipLaunchKernelGGL((patch_embed_kernel<_Float16, true>), dim3(tiles_n * tiles_m), dim3(256), 0, st, a, tiles_n, tiles_m);
    else
      hipLaunchKernelGGL((patch_embed_kernel<_Float16, false>), dim3(tiles_n * tiles_m), dim3(256), 0, st, a, tiles_n, tiles_m);
    HCIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_row_kernel<_Float16>, cgrid, dim3(256), 0, st, cls, pos, pos_mult, b, np + 1, d,
                       static_cast<_Float16*>(tok));
  }
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

int hcir_patch_embed_route(int64_t b, int32_t c, int32_t h, int32_t w_px, int32_t p, int32_t d, int64_t ldw,
                           int tok_dtype) {
  if (b <= 0 || c <= 0 || h <= 0 || w_px <= 0 || p <= 0 || d <= 0 || h % p || w_px % p) return HCIR_ERR_INVALID;
  return patch_embed_plan(b, c, h, w_px, p, d, ldw, tok_dtype).route;
}

int hcir_patch_embed_fused(const float* img, int64_t b, int32_t c, int32_t h, int32_t w_px, int32_t p,
                           const void* w_f16, int64_t ldw, const float* bias, const float* cls, const float* pos,
                           float pos_mult, int32_t d, void* tok, int tok_dtype, float* stats_part, void* stream) {
  HCIR_ENTER();
  if (!img || !w_f16 || !bias || !cls || !pos || !tok || b <= 0) return HCIR_ERR_INVALID;
  if (p <= 0 || p > 32 || c <= 0 || h <= 0 || w_px <= 0 || h % p || w_px % p || d <= 0 || (d & 7))
    return HCIR_ERR_INVALID;
  if (tok_dtype != HCIR_F32 && tok_dtype != HCIR_F16) return HCIR_ERR_UNSUPPORTED;
  const PatchPlan q = patch_embed_plan(b, c, h, w_px, p, d, ldw, tok_dtype);
  if (q.route != HCIR_PATCH_ROUTE_BIG) return HCIR_ERR_UNSUPPORTED;
  PatchGemmArgs g{};
  g.a = nullptr;
  g.w = static_cast<const _Float16*>(w_f16);
  g.bias = bias;
  g.scale = nullptr;
  g.out = tok;
  g.m = q.rows;
  g.lda = 0;
  g.ldw = ldw;
  g.ldo = d;
  g.n = d;
  g.k = c * 256;
  g.stats_part = stats_part;
  g.resid = tok;
  g.stats_ld = b * q.t;
  g.img = img;
  g.pos = pos;
  g.pos_mult = pos_mult;
  g.np = q.np;
  g.gw = w_px / 16;
  g.c = c;
  g.h = h;
  g.w_px = w_px;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(patch_embed_big_kernel, dim3(q.grid), dim3(G256::NT), 0, st, g, q.tn, q.tm);
  HCIR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cls_row_stats_kernel, dim3((unsigned)hcir_cdiv(b * (d >> 3), 256)), dim3(256), 0, st, cls, pos,
                     pos_mult, b, q.t, d, static_cast<_Float16*>(tok), stats_part);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
