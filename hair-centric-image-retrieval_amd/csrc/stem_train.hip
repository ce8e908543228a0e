// stem_train.hip — the ResNet stem in training (hcir/conv_train.py stem_train, the `hip_train_stem` switch):
// Conv2d(3, 64, 7, stride 2, pad 3) to an fp16 NHWC pre-norm map, normalise + ReLU + MaxPool2d(3, 2, 1) in one pass,
// the backward of that pass down to the conv map, and the weight gradient of the Cin = 3 convolution.  The batch
// statistics and the BatchNorm backward between them are bn2d.hip's; the image needs no gradient, so there is no data
// gradient.  Geometry: stem_plan.h.  No atomics, no allocation, no synchronisation; two calls give the same bits.
#include "common.h"
#include "split_sum.h"
#include "stem_plan.h"
#include "tr_layout.h"

namespace {

// The 37 x 37 x 3 input patch under a 16 x 16 tile of conv pixels, rounded to fp16, zeros outside the image (the
// conv's padding): tap k = (c, ky, kx) of tile pixel (ly, lx) is patch[2 ly * 37 + 2 lx + c * 37^2 + ky * 37 + kx].
// Split in two so that a caller can issue the loads early: all of a thread's 17 loads are in flight together.
constexpr int STEMT_FILL = (STEMT_PATCH + 255) / 256;

__device__ __forceinline__ void stem_load_patch(float (&v)[STEMT_FILL], const float* __restrict__ img, int64_t b, int h,
                                                int w, int iy0, int ix0) {
#pragma unroll
  for (int u = 0; u < STEMT_FILL; ++u) {
    const int idx = threadIdx.x + 256 * u;   // idx >= STEMT_PATCH decodes to c == 3: rejected below
    const int c = idx / (STEMT_TI * STEMT_TI), rem = idx - c * (STEMT_TI * STEMT_TI);
    const int py = rem / STEMT_TI, px = rem - py * STEMT_TI;
    const int iy = iy0 + py, ix = ix0 + px;
    v[u] = 0.f;
    if (c < 3 && (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w)
      v[u] = img[((b * 3 + c) * h + iy) * (int64_t)w + ix];
  }
}

__device__ __forceinline__ void stem_store_patch(_Float16* patch, const float (&v)[STEMT_FILL]) {
#pragma unroll
  for (int u = 0; u < STEMT_FILL; ++u) {
    const int idx = threadIdx.x + 256 * u;
    if (idx < STEMT_PATCH) patch[idx] = (_Float16)v[u];
  }
}

__device__ __forceinline__ int stem_tap_offset(int k) {
  const int c = k / 49, rem = k - c * 49, ky = rem / 7, kx = rem - ky * 7;
  return k < STEM_K ? c * (STEMT_TI * STEMT_TI) + ky * STEMT_TI + kx : 0;   // padded taps re-read tap 0
}

__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const f16x2 v = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(uint32_t, v);
}

// ------------------------------------------------------------------ hcir_stem_conv_f16
// resnet_stem_kernel's MFMA scheme on non-overlapping 16 x 16 tiles of conv pixels (256 rows = 4 waves x 2 tiles of
// 32), with the operands swapped: A = the packed weight (rows = channels), B = the pixels' taps gathered from the
// patch, so that a lane's accumulator holds channels of ONE pixel - registers 4 g .. 4 g + 3 of lane-half hf are
// channels 8 g + 4 hf .. + 3.  The two halves exchange one group of four (lane ^ 32), after which every lane stores
// 8 contiguous channels: 16 bytes.
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ img, const _Float16* __restrict__ wp,
                                                        _Float16* __restrict__ out, int h, int w, int hc, int wc,
                                                        int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) _Float16 patch[STEMT_PATCH + 5];
  __shared__ __attribute__((aligned(16))) uint16_t tbl[STEM_KP];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, r32 = lane & 31, hf = lane >> 5;
  const int64_t blk = blockIdx.x;
  const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
  const int64_t b = blk / ((int64_t)tiles_x * tiles_y);
  const int cy0 = ty * STEMT_TC, cx0 = tx * STEMT_TC;
  float pv[STEMT_FILL];
  stem_load_patch(pv, img, b, h, w, 2 * cy0 - 3, 2 * cx0 - 3);
  stem_store_patch(patch, pv);
  if (t < STEM_KP) tbl[t] = (uint16_t)stem_tap_offset(t);
  __syncthreads();

  f32x16 acc[2][2];
  int base[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int p = (wv * 2 + i) * 32 + r32;
    base[i] = 2 * (p >> 4) * STEMT_TI + 2 * (p & 15);
  }
  for (int kk = 0; kk < STEM_KP / 16; ++kk) {
    const u32x4 o4 = *(const u32x4*)(&tbl[16 * kk + 8 * hf]);
    f16x8 wf[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) wf[j] = *(const f16x8*)(wp + ((int64_t)(kk * 2 + j) * 64 + lane) * 8);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f16x8 pf;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pf[2 * q] = patch[base[i] + (int)(o4[q] & 0xffffu)];
        pf[2 * q + 1] = patch[base[i] + (int)(o4[q] >> 16)];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], pf, acc[i][j], 0, 0, 0);
    }
  }

#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = (wv * 2 + i) * 32 + r32;
    const int cy = cy0 + (p >> 4), cx = cx0 + (p & 15);
    const bool inside = cy < hc && cx < wc;
    _Float16* po = out + ((b * hc + cy) * (int64_t)wc + cx) * 64 + 8 * hf;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        // groups 2 gp and 2 gp + 1: half 0 keeps the first and sends the second, half 1 the other way round
        const int e0 = 8 * gp, e1 = 8 * gp + 4;
        const uint32_t a0 = pack2(acc[i][j][e0], acc[i][j][e0 + 1]), a1 = pack2(acc[i][j][e0 + 2], acc[i][j][e0 + 3]);
        const uint32_t b0 = pack2(acc[i][j][e1], acc[i][j][e1 + 1]), b1 = pack2(acc[i][j][e1 + 2], acc[i][j][e1 + 3]);
        const uint32_t r0 = __shfl_xor(hf ? a0 : b0, 32), r1 = __shfl_xor(hf ? a1 : b1, 32);
        const u32x4 v = hf ? (u32x4){r0, r1, b0, b1} : (u32x4){a0, a1, r0, r1};
        if (inside) *(u32x4*)(po + j * 32 + gp * 16) = v;
      }
  }
}

// ------------------------------------------------------------------ hcir_stem_bn_relu_pool_f16
// One lane per pooled pixel and 8 channels: up to nine 16-byte loads of the conv map (the windows overlap, the second
// and third reads of a vector come from the caches), y in fp32, the max over the positions inside the map, ReLU after
// the max (max and ReLU commute), one rounding.  Eight lanes cover a pixel's 128 bytes; the grid strides over the map.
__global__ __launch_bounds__(256) void stem_bn_relu_pool_kernel(const f16x8* __restrict__ c, int64_t total, int hc,
                                                                int wc, int hp, int wp,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ rstd,
                                                                f16x8* __restrict__ out) {
  const int cs = threadIdx.x & 7;   // the stride is a multiple of 8: a lane keeps its channels
  float mu[8], sc[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[cs * 8 + j];
    sc[j] = rstd[cs * 8 + j] * gamma[cs * 8 + j];
    be[j] = beta[cs * 8 + j];
  }
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t pix = idx >> 3, row = pix / wp;
    const int pw = (int)(pix - row * wp), ph = (int)(row % hp);
    const int64_t b = row / hp;
    f16x8 v[9];
    bool ok[9];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int i = 2 * ph - 1 + dy, j = 2 * pw - 1 + dx;
        ok[dy * 3 + dx] = (unsigned)i < (unsigned)hc && (unsigned)j < (unsigned)wc;
        if (ok[dy * 3 + dx]) v[dy * 3 + dx] = c[((b * hc + i) * (int64_t)wc + j) * 8 + cs];
      }
    float mx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) mx[j] = -INFINITY;   // the window's centre is always inside the map
#pragma unroll
    for (int q = 0; q < 9; ++q)
      if (ok[q]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) mx[j] = fmaxf(mx[j], fmaf((float)v[q][j] - mu[j], sc[j], be[j]));
      }
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)fmaxf(mx[j], 0.f);
    out[idx] = o;
  }
}

// ------------------------------------------------------------------ hcir_stem_pool_relu_bwd_f16
// One workgroup per 16 x 16 tile of conv pixels = 8 x 8 pooled windows plus the one-window halo below and to the right
// (an odd conv row or column lies in two windows): 9 x 9 windows.  Pass 1, one lane per window and 8 channels: the
// selected position - torch's: the first, in row-major order, among the positions inside the map at which y is
// maximal.  y is monotone in c per channel, so the selection is made on the fp16 values of c themselves and is exact:
// first maximum where s = rstd * gamma > 0, first minimum where s < 0, first position where s == 0.  LDS gets the
// position's code and dp [y(selected) > 0].  Pass 2, one lane per conv pixel and 8 channels: the fp32 sum, in a fixed
// order, over its 1, 2 or 4 windows of the values whose code names this pixel; one rounding, one 16-byte store.
__global__ __launch_bounds__(256) void stem_pool_relu_bwd_kernel(
    const f16x8* __restrict__ dp, const f16x8* __restrict__ c, f16x8* __restrict__ g, int hc, int wc, int hp, int wp,
    int tiles_x, int tiles_y, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ rstd) {
  constexpr int NW = STEMT_TP + 1;
  __shared__ f16x8 wval[NW * NW * 8];
  __shared__ uint8_t wsel[NW * NW * 8][8];

  const int t = threadIdx.x, cs = t & 7;
  const int64_t blk = blockIdx.x;
  const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
  const int64_t b = blk / ((int64_t)tiles_x * tiles_y);
  const int ph0 = ty * STEMT_TP, pw0 = tx * STEMT_TP;
  float mu[8], sc[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[cs * 8 + j];
    sc[j] = rstd[cs * 8 + j] * gamma[cs * 8 + j];
    be[j] = beta[cs * 8 + j];
  }

  for (int item = t; item < NW * NW * 8; item += 256) {   // item & 7 == cs
    const int win = item >> 3, wy = win / NW, wx = win - wy * NW;
    const int ph = ph0 + wy, pw = pw0 + wx;
    f16x8 val;
    uint8_t sel[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) val[j] = (_Float16)0.f, sel[j] = 255;   // no window: no code matches
    if (ph < hp && pw < wp) {
      const f16x8 d = dp[((b * hp + ph) * (int64_t)wp + pw) * 8 + cs];
      float best[8], cbest[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) best[j] = cbest[j] = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int i = 2 * ph - 1 + dy, jx = 2 * pw - 1 + dx;
          if ((unsigned)i < (unsigned)hc && (unsigned)jx < (unsigned)wc) {
            const f16x8 v = c[((b * hc + i) * (int64_t)wc + jx) * 8 + cs];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float cv = (float)v[j], key = sc[j] > 0.f ? cv : sc[j] < 0.f ? -cv : 0.f;
              if (sel[j] == 255 || key > best[j]) best[j] = key, cbest[j] = cv, sel[j] = (uint8_t)(dy * 3 + dx);
            }
          }
        }
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = fmaf(cbest[j] - mu[j], sc[j], be[j]) > 0.f ? d[j] : (_Float16)0.f;
    }
    wval[item] = val;
#pragma unroll
    for (int j = 0; j < 8; ++j) wsel[item][j] = sel[j];
  }
  __syncthreads();

  for (int item = t; item < STEMT_TC * STEMT_TC * 8; item += 256) {
    const int pix = item >> 3, ly = pix >> 4, lx = pix & 15;
    const int i = 2 * ph0 + ly, jx = 2 * pw0 + lx;
    if (i >= hc || jx >= wc) continue;
    // an even row is the middle row (dy = 1) of window ly / 2; an odd one the last (dy = 2) of (ly - 1) / 2 and the
    // first (dy = 0) of (ly + 1) / 2.  Columns alike.
    const int ny = 1 + (ly & 1), nx = 1 + (lx & 1);
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    for (int a = 0; a < ny; ++a) {
      const int wy = (ly >> 1) + a, dy = (ly & 1) ? 2 - 2 * a : 1;
      for (int e = 0; e < nx; ++e) {
        const int wx = (lx >> 1) + e, dx = (lx & 1) ? 2 - 2 * e : 1;
        const int w8 = (wy * NW + wx) * 8 + cs;
        const f16x8 v = wval[w8];
        const uint8_t code = (uint8_t)(dy * 3 + dx);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += wsel[w8][j] == code ? (float)v[j] : 0.f;
      }
    }
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)s[j];
    g[((b * hc + i) * (int64_t)wc + jx) * 8 + cs] = o;
  }
}

// ------------------------------------------------------------------ hcir_stem_wgrad_f16
// dw[n][k] = sum_m dc[m][n] * patch(m)[k]: the contraction index m = (b, i, j) is the slow index of both operands, as
// in conv_bwd.hip.  Per 16 x 16 tile of conv pixels the dc tile is staged as stored, [256 m][64 n] fp16 (zeros for
// pixels outside the map), swizzled as tr_layout.h lays out 128-B rows, and read TRANSPOSED with
// ds_read_b64_tr_b16 (two reads = one 16x16x32 A operand); the B operand is gathered from the fp16 input patch through
// the forward's tap offsets: lane 16 g + l holds pixels 8 g .. 8 g + 7 of the step's 32 (one tile row: consecutive
// pixels are 2 halves apart) at tap k = 16 kt + l.  A wave owns three 16-wide k tiles (K = 147 padded to 4 x 48) and
// all 64 channels: 12 accumulator fragments.  The workgroups are persistent: part p loops over conv tiles
// [p, p + 1) * tiles_per_part with the accumulators in registers and writes one [64][147] partial, in torch's layout,
// to the workspace; a second kernel (split_sum.h) adds the partials in part order.

struct StemWgradArgs {
  const float* img;
  const _Float16* dc;
  float* part;   // [parts][64][147], or dw itself with one part
  int64_t tiles, tiles_per_part;
  int32_t h, w, hc, wc, tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void stem_wgrad_kernel(const StemWgradArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 patch[STEMT_PATCH + 5];
  __shared__ __attribute__((aligned(16))) char dcs[STEMT_TC * STEMT_TC * 128];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const TrLane ln = tr_lane(lane);
  const int g16 = ln.g16, l16 = lane & 15;
  int toff[3];
#pragma unroll
  for (int kt = 0; kt < 3; ++kt) toff[kt] = stem_tap_offset(16 * (3 * wv + kt) + l16);
  const int pbase = 2 * (g16 >> 1) * STEMT_TI + 16 * (g16 & 1);   // pixel 8 g16 of a step: row g16 >> 1, column 8 (g16 & 1)
  const int fc = t & 7, fr = t >> 3;                              // fill: 16-B chunk fc of rows fr + 32 i

  f32x4 acc[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) acc[i][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int64_t t0 = blockIdx.x * a.tiles_per_part;
  const int64_t t1 = t0 + a.tiles_per_part < a.tiles ? t0 + a.tiles_per_part : a.tiles;
  for (int64_t tile = t0; tile < t1; ++tile) {   // uniform over the workgroup: the transposed reads run with EXEC full
    const int tx = (int)(tile % a.tiles_x), ty = (int)((tile / a.tiles_x) % a.tiles_y);
    const int64_t b = tile / ((int64_t)a.tiles_x * a.tiles_y);
    const int cy0 = ty * STEMT_TC, cx0 = tx * STEMT_TC;
    // this tile's loads are issued before the barrier: they fly while the slower waves finish the previous tile
    float pv[STEMT_FILL];
    u32x4 dv[8];
    stem_load_patch(pv, a.img, b, a.h, a.w, 2 * cy0 - 3, 2 * cx0 - 3);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = fr + 32 * i, cy = cy0 + (row >> 4), cx = cx0 + (row & 15);
      dv[i] = (u32x4){0u, 0u, 0u, 0u};
      if (cy < a.hc && cx < a.wc) dv[i] = *(const u32x4*)(a.dc + ((b * a.hc + cy) * (int64_t)a.wc + cx) * 64 + fc * 8);
    }
    __syncthreads();   // the previous tile's reads are done
    stem_store_patch(patch, pv);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = fr + 32 * i;
      *(u32x4*)(dcs + tr_fill_off<128>(row, fc)) = dv[i];
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < 8; ++ks) {
      f16x8 af[4], bf[3];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int row = tr_lane_row(ln, ks, hf);
#pragma unroll
        for (int i = 0; i < 4; ++i) tr_read_half(af[i], hf, dcs + tr_read_off<128>(row, i, ln.p4));
      }
      const int pix = pbase + 4 * STEMT_TI * ks;   // two tile rows per step
#pragma unroll
      for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int j = 0; j < 8; ++j) bf[kt][j] = patch[pix + 2 * j + toff[kt]];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
          acc[i][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[kt], acc[i][kt], 0, 0, 0);
    }
  }

  // acc[i][kt][e] is dw[16 i + 4 (lane >> 4) + e][16 (3 wv + kt) + (lane & 15)]
  float* out = a.part + (int64_t)blockIdx.x * STEM_DW;
#pragma unroll
  for (int kt = 0; kt < 3; ++kt) {
    const int k = 16 * (3 * wv + kt) + l16;
    if (k < STEM_K) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) out[(16 * i + 4 * g16 + e) * STEM_K + k] = acc[i][kt][e];
    }
  }
}

}  // namespace

extern "C" int hcir_stem_conv_f16(const float* img, int64_t b, int32_t h, int32_t w, const void* w_packed, void* out,
                                  void* stream) {
  StemPlan p;
  const int st = stem_plan(b, h, w, &p);   // host arithmetic only: no device needed
  if (st != HCIR_OK) return st;
  if (!img || !w_packed || !out) return HCIR_ERR_INVALID;
  HCIR_ENTER();
  hipLaunchKernelGGL(stem_conv_kernel, dim3((unsigned)p.tiles), dim3(256), 0, (hipStream_t)stream, img,
                     (const _Float16*)w_packed, (_Float16*)out, h, w, p.hc, p.wc, p.tiles_x, p.tiles_y);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_stem_bn_relu_pool_f16(const void* c, int64_t b, int32_t hc, int32_t wc, const float* gamma,
                                          const float* beta, const float* save_mean, const float* save_rstd, void* out,
                                          void* stream) {
  int32_t hp, wp;
  const int st = stem_map_plan(b, hc, wc, &hp, &wp);
  if (st != HCIR_OK) return st;
  if (!c || !gamma || !beta || !save_mean || !save_rstd || !out) return HCIR_ERR_INVALID;
  const int64_t total = b * hp * wp * 8;
  const int64_t blocks = hcir_cdiv(total, 256);
  HCIR_ENTER();
  // memory-bound: the grid cap of the bn2d elementwise kernels, striding over the rest
  hipLaunchKernelGGL(stem_bn_relu_pool_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0,
                     (hipStream_t)stream, (const f16x8*)c, total, hc, wc, hp, wp, gamma, beta, save_mean, save_rstd,
                     (f16x8*)out);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_stem_pool_relu_bwd_f16(const void* dp, const void* c, int64_t b, int32_t hc, int32_t wc,
                                           const float* gamma, const float* beta, const float* save_mean,
                                           const float* save_rstd, void* g, void* stream) {
  int32_t hp, wp;
  const int st = stem_map_plan(b, hc, wc, &hp, &wp);
  if (st != HCIR_OK) return st;
  if (!dp || !c || !gamma || !beta || !save_mean || !save_rstd || !g) return HCIR_ERR_INVALID;
  const int tiles_y = (hc + STEMT_TC - 1) / STEMT_TC, tiles_x = (wc + STEMT_TC - 1) / STEMT_TC;
  const int64_t blocks = b * tiles_y * tiles_x;
  if (blocks > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  HCIR_ENTER();
  hipLaunchKernelGGL(stem_pool_relu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const f16x8*)dp, (const f16x8*)c, (f16x8*)g, hc, wc, hp, wp, tiles_x, tiles_y, gamma, beta,
                     save_mean, save_rstd);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" size_t hcir_stem_wgrad_workspace_bytes(int64_t b, int32_t h, int32_t w) {
  StemPlan s;
  StemWgradPlan p;
  if (stem_plan(b, h, w, &s) != HCIR_OK) return 0;
  stem_wgrad_plan(s, &p);
  return stem_wgrad_workspace_bytes(p);
}

// HOST: the number of persistent parts the weight gradient runs the shape with, or the status it returns for it.
extern "C" int32_t hcir_stem_wgrad_parts(int64_t b, int32_t h, int32_t w) {
  StemPlan s;
  StemWgradPlan p;
  const int st = stem_plan(b, h, w, &s);
  if (st != HCIR_OK) return st;
  stem_wgrad_plan(s, &p);
  return p.parts;
}

extern "C" int hcir_stem_wgrad_f16(const float* img, const void* dc, int64_t b, int32_t h, int32_t w, float* dw,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  StemPlan s;
  StemWgradPlan p;
  const int st = stem_plan(b, h, w, &s);
  if (st != HCIR_OK) return st;
  stem_wgrad_plan(s, &p);
  if (!img || !dc || !dw) return HCIR_ERR_INVALID;
  const size_t need = stem_wgrad_workspace_bytes(p);
  if (need && (!workspace || workspace_bytes < need)) return HCIR_ERR_WORKSPACE;
  HCIR_ENTER();
  hipStream_t hs = (hipStream_t)stream;
  StemWgradArgs a;
  a.img = img;
  a.dc = (const _Float16*)dc;
  a.part = p.parts > 1 ? (float*)workspace : dw;
  a.tiles = s.tiles;
  a.tiles_per_part = p.tiles_per_part;
  a.h = h; a.w = w; a.hc = s.hc; a.wc = s.wc; a.tiles_x = s.tiles_x; a.tiles_y = s.tiles_y;
  hipLaunchKernelGGL(stem_wgrad_kernel, dim3((unsigned)p.parts), dim3(256), 0, hs, a);
  HCIR_LAUNCH_CHECK();
  if (p.parts > 1) {
    split_sum((const float*)workspace, p.parts, STEM_DW, dw, hs);   // STEM_DW = 64 * 147 is a multiple of 4
    HCIR_LAUNCH_CHECK();
  }
  return HCIR_OK;
}
