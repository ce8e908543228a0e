// conv.hip — the ResNet-18/50 trunk in eval mode: implicit-GEMM convolution, fused stem, global average pool.
// Activations NHWC fp16, fp32 accumulate and epilogue, one rounding to fp16 per stored value.
// Geometry and tile choice: conv_plan.h.  Decisions and measurements: DESIGN.md §3.4.
#include "common.h"
#include "conv_plan.h"

namespace {

// ------------------------------------------------------------------ hcir_conv2d_f16
// M = B*Ho*Wo output pixels, N = Cout, K = R*S*Cin in (r, s, c) order: a K step of 64 is 64 contiguous channels of one
// tap of one input pixel (128 B), or zeros when the tap falls into the padding.  No im2col buffer: every thread owns
// the same 16-B chunk column of four A rows (output pixels) for the whole K loop, decodes their (b, ho, wo) once, and
// per K step only adds the tap offset.  An output pixel is decoded from its linear index m, so a tile that runs over
// the end of an output row or of an image needs no special case; rows m >= M read nothing and store nothing.
// Fill: global_load_dwordx4 into registers one K step ahead, ds_write_b128 after the MFMAs of the current step
// (two LDS buffers, one barrier per step).  LDS rows are 128 B; the 16-B chunk index is XORed with (row >> 1) & 7 so
// that the ds_read_b128 of an MFMA operand (32 rows x one chunk per half-wave) and the fill's writes are conflict-free.
struct ConvArgs {
  const _Float16* x;
  const _Float16* w;
  const float* scale;
  const float* bias;
  const _Float16* resid;
  _Float16* out;
  int32_t h, w_px, cin, cout, s, stride, pad, ho, wo, k, relu, grid_n;
  int64_t m;
};

__device__ __forceinline__ int conv_lds_off(int row, int chunk) { return row * CONV_BK + ((chunk ^ ((row >> 1) & 7)) << 3); }

template <int BN>
__global__ __launch_bounds__(256) void conv2d_f16_kernel(const ConvArgs a) {
  constexpr int NT = BN / 64;          // 32-wide n tiles per wave
  constexpr int BROWS = BN / 32;       // B rows per fill thread
  __shared__ __attribute__((aligned(16))) _Float16 As[2][CONV_BM * CONV_BK];
  __shared__ __attribute__((aligned(16))) _Float16 Bs[2][BN * CONV_BK];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t tile = blockIdx.x;
  const int n0 = (int)(tile % a.grid_n) * BN;       // n fastest: neighbouring workgroups share the A rows in L2
  const int64_t m0 = (tile / a.grid_n) * CONV_BM;

  // fill roles: chunk column fc of rows fr + 32 i
  const int fc = t & 7, fr = t >> 3;
  int32_t hi0[4], wi0[4], pix0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + fr + 32 * i;
    if (m < a.m) {
      const int32_t hw = a.ho * a.wo;
      const int32_t b = (int32_t)(m / hw), rem = (int32_t)(m - (int64_t)b * hw);
      const int32_t ho = rem / a.wo, wo = rem - ho * a.wo;
      hi0[i] = ho * a.stride - a.pad;
      wi0[i] = wo * a.stride - a.pad;
      pix0[i] = b * a.h * a.w_px;
    } else {
      hi0[i] = INT32_MIN / 2;   // every tap out of range: the row is zeros
      wi0[i] = 0;
      pix0[i] = 0;
    }
  }

  u32x4 areg[4], breg[BROWS];
  auto load = [&](int kt) {
    const int kofs = kt * CONV_BK;
    const int tap = kofs / a.cin, c0 = kofs - tap * a.cin;
    const int r = tap / a.s, s = tap - r * a.s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hi = hi0[i] + r, wi = wi0[i] + s;
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)hi < (unsigned)a.h && (unsigned)wi < (unsigned)a.w_px)
        v = *(const u32x4*)(a.x + (int64_t)(pix0[i] + hi * a.w_px + wi) * a.cin + c0 + fc * 8);
      areg[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i)
      breg[i] = *(const u32x4*)(a.w + (int64_t)(n0 + fr + 32 * i) * a.k + kofs + fc * 8);
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *(u32x4*)(&As[buf][conv_lds_off(fr + 32 * i, fc)]) = areg[i];
#pragma unroll
    for (int i = 0; i < BROWS; ++i) *(u32x4*)(&Bs[buf][conv_lds_off(fr + 32 * i, fc)]) = breg[i];
  };

  // MFMA roles: wave (wm, wn) owns rows wm*64 .. +63 and columns wn*BN/2 .. +BN/2-1
  const int wm = wv & 1, wn = wv >> 1, r32 = lane & 31, hf = lane >> 5;
  f32x16 acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nk = a.k / CONV_BK;
  load(0);
  stash(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ch = 2 * kk + hf;
      f16x8 af[2], bf[NT];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *(const f16x8*)(&As[buf][conv_lds_off(wm * 64 + i * 32 + r32, ch)]);
#pragma unroll
      for (int j = 0; j < NT; ++j) bf[j] = *(const f16x8*)(&Bs[buf][conv_lds_off(wn * (BN / 2) + j * 32 + r32, ch)]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) stash(buf ^ 1);
    __syncthreads();
  }

  // epilogue: v = acc * scale[n] + bias[n] (+ resid) (relu) -> fp16.  Accumulator register e of lane-half hf is row
  // acc_row(e, hf), column lane & 31: 32 lanes store 64 contiguous bytes of one output pixel.
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wn * (BN / 2) + j * 32 + r32;
    const float sc = a.scale[n], bi = a.bias[n];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t m = m0 + wm * 64 + i * 32 + acc_row(e, hf);
        if (m < a.m) {
          float v = acc[i][j][e] * sc + bi;
          if (a.resid) v += (float)a.resid[m * a.cout + n];
          if (a.relu) v = fmaxf(v, 0.f);
          a.out[m * a.cout + n] = (_Float16)v;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ hcir_resnet_stem
// One workgroup = one 7 x 7 tile of the POOLED map of one image: the 15 x 15 conv outputs under it (225 rows, padded
// to 8 MFMA tiles of 32) x 64 channels x K = 147 (padded to 160), from a 35 x 35 x 3 input patch held in LDS as fp16
// (the image is rounded to fp16 for the MFMA; zero outside the image = the conv's padding).  The A operand is gathered
// from the patch through a table k -> patch offset (tap k of a conv pixel is patch[base(pixel) + tbl[k]]); the padded
// taps re-read tap 0 against a zero weight.  conv * scale + bias, ReLU in fp32 go to LDS; conv pixels outside the conv map are the
// pool's padding and are stored as -inf, the identity of max, so they never win; the 3 x 3 / 2 max is taken in fp32
// and rounded once.  At 224 x 224 the pooled map is 56 x 56 = 8 x 8 whole tiles.
constexpr int STEM_PATCH = 3 * STEM_TI * STEM_TI;   // 3675 halves; base <= 1008, tbl <= 2666: every read is inside
constexpr int STEM_NPIX = STEM_TC * STEM_TC;        // 225

__global__ __launch_bounds__(256) void resnet_stem_kernel(const float* __restrict__ img, const _Float16* __restrict__ wp,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ bias, _Float16* __restrict__ out,
                                                          int h, int w, int hc, int wc, int hp, int wpool, int tiles_x,
                                                          int tiles_y) {
  __shared__ __attribute__((aligned(16))) _Float16 patch[STEM_PATCH];
  __shared__ __attribute__((aligned(16))) uint16_t tbl[STEM_KP];
  __shared__ float cbuf[STEM_NPIX * 64];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, r32 = lane & 31, hf = lane >> 5;
  const int64_t blk = blockIdx.x;
  const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
  const int64_t b = blk / ((int64_t)tiles_x * tiles_y);
  const int ph0 = ty * STEM_TP, pw0 = tx * STEM_TP;
  const int cy0 = 2 * ph0 - 1, cx0 = 2 * pw0 - 1;   // first conv row / column of the tile (-1: the pool's padding)
  const int iy0 = 2 * cy0 - 3, ix0 = 2 * cx0 - 3;   // first input row / column of the patch

  for (int idx = t; idx < STEM_PATCH; idx += 256) {
    const int c = idx / (STEM_TI * STEM_TI), rem = idx - c * (STEM_TI * STEM_TI);
    const int py = rem / STEM_TI, px = rem - py * STEM_TI;
    const int iy = iy0 + py, ix = ix0 + px;
    float v = 0.f;
    if ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) v = img[((b * 3 + c) * h + iy) * (int64_t)w + ix];
    patch[idx] = (_Float16)v;
  }
  if (t < STEM_KP) {
    const int c = t / 49, rem = t - c * 49, ky = rem / 7, kx = rem - ky * 7;
    tbl[t] = (uint16_t)(t < STEM_K ? c * (STEM_TI * STEM_TI) + ky * STEM_TI + kx : 0);
  }
  __syncthreads();

  f32x16 acc[2][2];
  int base[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int p = min((wv * 2 + i) * 32 + r32, STEM_NPIX - 1);   // rows past 225 recompute the last pixel, unused
    const int ly = p / STEM_TC, lx = p - ly * STEM_TC;
    base[i] = 2 * ly * STEM_TI + 2 * lx;
  }
  for (int kk = 0; kk < STEM_KP / 16; ++kk) {
    const u32x4 o4 = *(const u32x4*)(&tbl[16 * kk + 8 * hf]);
    f16x8 bf[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[j] = *(const f16x8*)(wp + ((int64_t)(kk * 2 + j) * 64 + lane) * 8);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f16x8 af;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        af[2 * q] = patch[base[i] + (int)(o4[q] & 0xffffu)];
        af[2 * q + 1] = patch[base[i] + (int)(o4[q] >> 16)];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf[j], acc[i][j], 0, 0, 0);
    }
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = j * 32 + r32;
    const float sc = scale[n], bi = bias[n];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = (wv * 2 + i) * 32 + acc_row(e, hf);
        if (p < STEM_NPIX) {
          const int ly = p / STEM_TC, lx = p - ly * STEM_TC;
          const bool inside = (unsigned)(cy0 + ly) < (unsigned)hc && (unsigned)(cx0 + lx) < (unsigned)wc;
          cbuf[p * 64 + n] = inside ? fmaxf(acc[i][j][e] * sc + bi, 0.f) : -INFINITY;
        }
      }
    }
  }
  __syncthreads();

  for (int o = t; o < STEM_TP * STEM_TP * 64; o += 256) {
    const int n = o & 63, q = o >> 6, py = q / STEM_TP, px = q - py * STEM_TP;
    const int ph = ph0 + py, pw = pw0 + px;
    if (ph < hp && pw < wpool) {
      float mx = -INFINITY;   // the window's centre (2 ph, 2 pw) is always inside the conv map
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) mx = fmaxf(mx, cbuf[((2 * py + dy) * STEM_TC + 2 * px + dx) * 64 + n]);
      out[((b * hp + ph) * (int64_t)wpool + pw) * 64 + n] = (_Float16)mx;
    }
  }
}

// ------------------------------------------------------------------ hcir_avgpool_nhwc_f16
// One workgroup per image; a thread owns channels t, t + 256, ... and adds their H*W values in index order with a
// Kahan-compensated fp32 sum (error 2 ulp of sum|x| whatever H*W is; plain fp32 chaining of 49 terms is bounded only by
// 48 ulp).  Optional F.normalize: sum of squares per thread in channel order, butterfly inside a wave, the four wave
// sums added in wave order: fixed order, no atomics.
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const _Float16* __restrict__ x, int hw, int c, int l2,
                                                           float eps, float* __restrict__ out) {
  __shared__ float wsum[4];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  const _Float16* xb = x + b * hw * (int64_t)c;
  float* ob = out + b * c;
  const float inv = 1.f / (float)hw;
  float ss = 0.f;
  for (int ch = t; ch < c; ch += 256) {
    float s = 0.f, comp = 0.f;
    for (int p = 0; p < hw; ++p) {
      const float y = (float)xb[(int64_t)p * c + ch] - comp;
      const float tt = s + y;
      comp = (tt - s) - y;
      s = tt;
    }
    const float mean = s * inv;
    ob[ch] = mean;
    ss += mean * mean;
  }
  if (!l2) return;
  ss = wave_sum(ss);
  if ((t & 63) == 0) wsum[t >> 6] = ss;
  __syncthreads();
  const float norm = sqrtf(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
  const float rn = 1.f / fmaxf(norm, eps);
  for (int ch = t; ch < c; ch += 256) ob[ch] *= rn;   // each thread rescales the values it wrote itself
}

}  // namespace

extern "C" int hcir_conv2d_f16(const void* x, int64_t b, int32_t h, int32_t w, int32_t cin, const void* wgt,
                               int32_t cout, int32_t r, int32_t s, int32_t stride, int32_t pad, const float* scale,
                               const float* bias, const void* resid, int relu, void* out, void* stream) {
  ConvPlan p;
  const int st = conv_plan(b, h, w, cin, cout, r, s, stride, pad, &p);   // host arithmetic only: no device needed
  if (st != HCIR_OK) return st;
  if (!x || !wgt || !scale || !bias || !out) return HCIR_ERR_INVALID;
  HCIR_ENTER();
  ConvArgs a;
  a.x = (const _Float16*)x;
  a.w = (const _Float16*)wgt;
  a.scale = scale;
  a.bias = bias;
  a.resid = (const _Float16*)resid;
  a.out = (_Float16*)out;
  a.h = h; a.w_px = w; a.cin = cin; a.cout = cout; a.s = s; a.stride = stride; a.pad = pad;
  a.ho = p.ho; a.wo = p.wo; a.k = p.k; a.relu = relu ? 1 : 0; a.grid_n = p.grid_n;
  a.m = p.m;
  const int64_t blocks = p.grid_m * p.grid_n;
  if (blocks > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  if (p.bn == 128)
    hipLaunchKernelGGL(conv2d_f16_kernel<128>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(conv2d_f16_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

// HOST: the N tile conv_plan picks for a shape (64 or 128), or the status hcir_conv2d_f16 would return for it.
extern "C" int32_t hcir_conv2d_tile_n(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r, int32_t s,
                                      int32_t stride, int32_t pad) {
  ConvPlan p;
  const int st = conv_plan(b, h, w, cin, cout, r, s, stride, pad, &p);
  return st != HCIR_OK ? st : p.bn;
}

extern "C" int hcir_resnet_stem(const float* img, int64_t b, int32_t h, int32_t w, const void* w_packed,
                                const float* scale, const float* bias, void* out, void* stream) {
  if (b < 1 || h < 1 || w < 1) return HCIR_ERR_INVALID;
  if (h < 7 || w < 7) return HCIR_ERR_UNSUPPORTED;
  if (!img || !w_packed || !scale || !bias || !out) return HCIR_ERR_INVALID;
  const int hc = stem_conv_size(h), wc = stem_conv_size(w), hp = stem_pool_size(h), wp = stem_pool_size(w);
  const int tiles_y = (hp + STEM_TP - 1) / STEM_TP, tiles_x = (wp + STEM_TP - 1) / STEM_TP;
  const int64_t blocks = b * tiles_x * tiles_y;
  if (blocks > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  HCIR_ENTER();
  hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img,
                     (const _Float16*)w_packed, scale, bias, (_Float16*)out, h, w, hc, wc, hp, wp, tiles_x, tiles_y);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_avgpool_nhwc_f16(const void* x, int64_t b, int32_t h, int32_t w, int32_t c, int l2_normalize,
                                     float eps, float* out, void* stream) {
  if (b < 1 || h < 1 || w < 1 || c < 1 || !x || !out) return HCIR_ERR_INVALID;
  if (b > INT32_MAX || (int64_t)h * w > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  HCIR_ENTER();
  hipLaunchKernelGGL(avgpool_nhwc_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x,
                     h * w, c, l2_normalize ? 1 : 0, eps, out);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}
