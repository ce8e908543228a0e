// attn_bwd32.hip — hcir_attn_bwd at head_dim 32, T <= 256: the decoder of MAE pre-training (MAEDecoderTIMM,
// decoder_embed_dim 512 / 16 heads; HairPretraining/src/backbone.py:472-482, autograd through its timm blocks in
// src/pretrain_engine.py:334).
//
// A SEPARATE, correctness-first kernel, as attn_fwd_generic_kernel is beside the tuned forward kernels - not a
// template of attn_bwd_kernel / attn_bwd2_kernel.  Why: those two are measured kernels whose register allocation and
// issue order were tuned by hand (attn_bwd.hip says where), instantiations of one template share the compiler's
// allocation context, and the head_dim-64 path has to give the bits and the time it gave.  This file is its own
// translation unit; attn_bwd.hip changes by one dispatch line.
//
// The structure is attn_bwd_kernel's (cdna_hip_programming.md Appendix B, "Attention backward": the KEY sits on the
// MFMA lane), restated for 64-byte image rows and a contraction of two 16-dim steps:
//   one workgroup of 8 waves per (batch, head); wave w owns keys [32 w, 32 (w + 1)) and keeps dK^T and dV^T of its
//   keys in registers (one 32-dim x 32-key accumulator each) over the sweep of the query tiles;
//   S = Q K^T and dP = dO V^T    MFMA 32x32x16, two k-steps; query on the row, key on the lane;
//   P = exp2(S scale log2e - lse), dS = P (dP - D), D_q = <dO_q, O_q> in fp32;
//   dV^T += dO^T P, dK^T += Q^T dS   the accumulators are the B operands, dO^T / Q^T by transposed LDS reads;
//   dQ^T = K^T dS^T              dS crosses LDS once (the wave's own [q][key] image); the eight partial dQ tiles meet
//                                in four padded fp32 slabs (wave 2j stores slab j, wave 2j+1 adds to it) that are
//                                summed in slab order: no atomics, fixed order, two runs are bit-equal.
// The arithmetic per element is that of attn_bwd_kernel with 32 in place of 64 terms in the dim contractions, which is
// what oracle.attention.bwd_bounds takes as a parameter.
// LDS: Q, dO, K images 3 x 16 KB (16-B chunks XOR-swizzled with (row >> 1) & 3), dS 16 KB, dQ slabs 4 x 4.1 KB,
// row constants 2 KB.
#include "common.h"

namespace {

struct AttnBwd32Args {
  const _Float16* qkv;   // [B][T][3][H][32]
  const _Float16* out;   // [B][T][H*32]
  const _Float16* dout;  // [B][T][H*32]
  const float* lse;      // [B][H][T]   log2 domain
  _Float16* dqkv;        // [B][T][3][H][32]
  int t, h;
  float scale, scale_log2e;
};

constexpr int kTP32 = 256;   // keys per (b, head): 8 waves x 32
constexpr int kHD = 32;
constexpr int kSlab = 33;    // floats per slab row: the 32 queries of a register spread over the banks

__device__ __forceinline__ int img32_off(int row, int c16) { return row * 64 + ((c16 ^ ((row >> 1) & 3)) << 4); }
// byte address of element column e0 (a multiple of 4) of `row`: a transposed read's 8-byte piece
__device__ __forceinline__ int img32_off_e(int row, int e0) { return img32_off(row, e0 >> 3) + (e0 & 7) * 2; }

__global__ __launch_bounds__(512, 1) void attn_bwd32_kernel(AttnBwd32Args a) {
  __shared__ __attribute__((aligned(16))) char lds[3 * kTP32 * 64 + 8 * 32 * 64 + 4 * 32 * kSlab * 4 + 2 * kTP32 * 4];
  char* qs = lds;
  char* dos = lds + kTP32 * 64;
  char* ks = lds + 2 * kTP32 * 64;
  char* dss = lds + 3 * kTP32 * 64;                                           // [8 waves][32 q][64 B]
  float* dqt = reinterpret_cast<float*>(lds + 3 * kTP32 * 64 + 8 * 32 * 64);  // [4 slabs][32 q][33]
  float* dsum = dqt + 4 * 32 * kSlab;                                         // D[q]
  float* lrow = dsum + kTP32;                                                 // lse[q]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int grp = lane >> 4, li = lane & 15;
  const int head = blockIdx.x % a.h;
  const int64_t b = blockIdx.x / a.h;
  const int64_t qkv_stride = (int64_t)3 * a.h * kHD, o_stride = (int64_t)a.h * kHD;
  const _Float16* qg = a.qkv + b * a.t * qkv_stride + head * kHD;
  const _Float16* kg = qg + (int64_t)a.h * kHD;
  const _Float16* vg = qg + (int64_t)2 * a.h * kHD;
  const _Float16* og = a.out + b * a.t * o_stride + head * kHD;
  const _Float16* dog = a.dout + b * a.t * o_stride + head * kHD;
  _Float16* dqg = a.dqkv + b * a.t * qkv_stride + head * kHD;
  _Float16* dkg = dqg + (int64_t)a.h * kHD;
  _Float16* dvg = dqg + (int64_t)2 * a.h * kHD;

  // ---- stage Q, dO, K images (rows past T: Q, K clamped to the last real row - finite, masked below; dO zero)
  for (int slot = tid; slot < kTP32 * 4; slot += 512) {
    const int row = slot >> 2, c = slot & 3;
    const int src = row < a.t ? row : a.t - 1;
    const u32x4 qv = *reinterpret_cast<const u32x4*>(qg + src * qkv_stride + c * 8);
    const u32x4 kv = *reinterpret_cast<const u32x4*>(kg + src * qkv_stride + c * 8);
    u32x4 dv = {0u, 0u, 0u, 0u};
    if (row < a.t) dv = *reinterpret_cast<const u32x4*>(dog + src * o_stride + c * 8);
    *reinterpret_cast<u32x4*>(qs + img32_off(row, c)) = qv;
    *reinterpret_cast<u32x4*>(ks + img32_off(row, c)) = kv;
    *reinterpret_cast<u32x4*>(dos + img32_off(row, c)) = dv;
  }
  // ---- row constants: D[q] = <dO[q], O[q]> (one fp32 fma chain over the 32 dims), lse[q] (+inf past T: P = 0 there)
  if (tid < kTP32) {
    const int q = tid;
    float dsv = 0.f, lv = __builtin_huge_valf();
    if (q < a.t) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f16x8 ov = *reinterpret_cast<const f16x8*>(og + q * o_stride + c * 8);
        const f16x8 dv = *reinterpret_cast<const f16x8*>(dog + q * o_stride + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) dsv = __builtin_fmaf((float)ov[e], (float)dv[e], dsv);
      }
      lv = a.lse[(b * a.h + head) * (int64_t)a.t + q];
    }
    dsum[q] = dsv;
    lrow[q] = lv;
  }
  // ---- this wave's K and V fragments (B operands: lane (key = 32 w + r, half h) holds [key][16 s + 8 h ..])
  f16x8 kf[2], vf[2];
  {
    int key = 32 * wave + r;
    key = key < a.t ? key : a.t - 1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      kf[s] = *reinterpret_cast<const f16x8*>(kg + key * qkv_stride + 16 * s + 8 * h);
      vf[s] = *reinterpret_cast<const f16x8*>(vg + key * qkv_stride + 16 * s + 8 * h);
    }
  }
  f32x16 dkt, dvt;   // lane = key column, registers = the 32 dims
#pragma unroll
  for (int i = 0; i < 16; ++i) dkt[i] = dvt[i] = 0.f;
  __syncthreads();

  char* myds = dss + wave * (32 * 64);
  auto ds_off = [](int row, int c16) { return row * 64 + ((c16 ^ ((row >> 1) & 3)) << 4); };
  const bool live = 32 * wave + r < a.t;
  const int nqt = (a.t + 31) >> 5;
  for (int qt = 0; qt < nqt; ++qt) {
    const int q0 = qt * 32;
    // ---- S = Q K^T, dP = dO V^T (A operands: row reads of the Q / dO images)
    f16x8 qf[2], dof[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      qf[s] = *reinterpret_cast<const f16x8*>(qs + img32_off(q0 + r, 2 * s + h));
      dof[s] = *reinterpret_cast<const f16x8*>(dos + img32_off(q0 + r, 2 * s + h));
    }
    f32x16 sc, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[i] = dp[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qf[s], kf[s], sc, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(dof[s], vf[s], dp, 0, 0, 0);
    }
    // ---- P and dS in the accumulator layout (row = query acc_row(i, h), column = key r)
    f16x8 pf[2], dsf[2];  // [16-query k-step]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qrow = acc_row(i, h);
      float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[i], a.scale_log2e, -lrow[q0 + qrow]));
      p = live ? p : 0.f;
      const float dsv = p * (dp[i] - dsum[q0 + qrow]);
      pf[i >> 3][i & 7] = (_Float16)p;
      dsf[i >> 3][i & 7] = (_Float16)dsv;
      // dS to the wave's [q][key] image for the dQ product (2-byte stores: 32 lanes = 64 contiguous bytes)
      *reinterpret_cast<_Float16*>(myds + ds_off(qrow, r >> 3) + (r & 7) * 2) = (_Float16)dsv;
    }
    asm volatile("" ::: "memory");  // the 2-byte dS stores above are read back below through another pointer type
    // ---- dV^T += dO^T P,  dK^T += Q^T dS: A operands by transposed reads, k order of an accumulator operand:
    //      element j of half h is query 16 s + 8 (j >> 2) + 4 h + (j & 3)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c0 = 16 * (grp & 1) + 4 * (li & 3);
      const int qb = q0 + 16 * s + 4 * (grp >> 1) + (li >> 2);
      f16x8 dot, qtf;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        tr_read_half(dot, half, dos + img32_off_e(qb + 8 * half, c0));
        tr_read_half(qtf, half, qs + img32_off_e(qb + 8 * half, c0));
      }
      dvt = __builtin_amdgcn_mfma_f32_32x32x16_f16(dot, pf[s], dvt, 0, 0, 0);
      dkt = __builtin_amdgcn_mfma_f32_32x32x16_f16(qtf, dsf[s], dkt, 0, 0, 0);
    }
    // ---- dQ^T[dim][q] = sum over this wave's keys of K^T[dim][key] dS^T[key][q]
    f32x16 dqa;
#pragma unroll
    for (int i = 0; i < 16; ++i) dqa[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // B operand: lane (q = r, half h) holds dS[q][16 s + 8 h .. + 7] of the wave's image (natural k order)
      const f16x8 dsb = *reinterpret_cast<const f16x8*>(myds + ds_off(r, 2 * s + h));
      const int c0 = 16 * (grp & 1) + 4 * (li & 3);
      const int kb = 32 * wave + 16 * s + 8 * (grp >> 1) + (li >> 2);
      f16x8 ktf;
#pragma unroll
      for (int half = 0; half < 2; ++half) tr_read_half(ktf, half, ks + img32_off_e(kb + 4 * half, c0));
      dqa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ktf, dsb, dqa, 0, 0, 0);
    }
    // the waves' partial tiles to four slabs, summed in slab order (see the header)
    {
      float* slab = dqt + (wave >> 1) * (32 * kSlab);
      if ((wave & 1) == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) slab[r * kSlab + acc_row(i, h)] = dqa[i];
      }
      __syncthreads();
      if ((wave & 1) == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) slab[r * kSlab + acc_row(i, h)] += dqa[i];
      }
      __syncthreads();
    }
    if (tid < 128) {
      const int q = tid >> 2, c = tid & 3;
      f16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float sacc = dqt[q * kSlab + c * 8 + e];
#pragma unroll
        for (int w = 1; w < 4; ++w) sacc += dqt[w * (32 * kSlab) + q * kSlab + c * 8 + e];
        o[e] = (_Float16)(sacc * a.scale);
      }
      if (q0 + q < a.t) *reinterpret_cast<f16x8*>(dqg + (q0 + q) * qkv_stride + c * 8) = o;
    }
    __syncthreads();
  }

  // ---- dK = scale dK^T, dV = dV^T: lane = key, registers = dims in groups of 4
  if (live) {
    const int key = 32 * wave + r;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f16x4 ok, ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ok[e] = (_Float16)(dkt[4 * g4 + e] * a.scale);
        ov[e] = (_Float16)dvt[4 * g4 + e];
      }
      const int dim = 8 * g4 + 4 * h;
      *reinterpret_cast<f16x4*>(dkg + key * qkv_stride + dim) = ok;
      *reinterpret_cast<f16x4*>(dvg + key * qkv_stride + dim) = ov;
    }
  }
}

}  // namespace

// the head_dim-32 arm of hcir_attn_bwd (attn_bwd.hip), which has checked the arguments
int hcir_attn_bwd32_launch(const void* qkv, const void* out, const void* d_out, const float* lse, int64_t b, int32_t t,
                           int32_t h, float scale, void* d_qkv, void* stream) {
  if (t > kTP32) return HCIR_ERR_UNSUPPORTED;
  AttnBwd32Args a{static_cast<const _Float16*>(qkv), static_cast<const _Float16*>(out),
                  static_cast<const _Float16*>(d_out), lse, static_cast<_Float16*>(d_qkv), t, h, scale,
                  scale * 1.44269504088896340736f};
  hipLaunchKernelGGL(attn_bwd32_kernel, dim3((unsigned)(b * h)), dim3(512), 0, static_cast<hipStream_t>(stream), a);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}
