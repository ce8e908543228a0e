// view.hip — everything of a SimCLR view behind the crop + resize (include/hcir.h "SimCLR training views").
//
// Stands where the loader workers of HP/mainpretrain.py:130 / HP/utils/dataloader.py:36-38 run lightly's
// SimCLRTransform on a PIL image: flip, colour jitter (four ops in a drawn order), grayscale, Gaussian blur, ToTensor,
// Normalize.  One workgroup of 1024 threads per view.  The 224 x 224 RGB8 crop (150 528 B) is read from HBM once, lives
// in LDS as three planes of 224 rows with a 228-byte pitch (57 dwords: a thread per row walks its row without bank
// conflicts, a thread per column reads consecutive bytes) and leaves as fp32 CHW: 150 KB in, 602 KB out per view.
// LDS: 3 * 224 * 228 + 68 = 153 284 of the CU's 163 840 bytes, i.e. one workgroup (16 waves) per CU by construction.
//   - per-pixel ops: a thread takes the same 4 adjacent pixels in every op (one dword per plane), so consecutive ops
//     need no barrier between them;
//   - contrast: its degenerate value is the rounded mean of L over the image as it is at that moment, an exact integer
//     sum reduced over the workgroup;
//   - blur: three box passes along the rows, then three down the columns, in place, one thread per line: with r <= 1
//     an output needs the two bytes on either side, and the bytes already overwritten are kept in registers.
// The arithmetic of every op is view_core.h (compiled for the host and compared with Pillow in tests/).
#include <math.h>

#include "common.h"
#include "view_core.h"

namespace {

constexpr int kS = HCIR_VIEW_SIZE;
constexpr int kPitch = 228;
constexpr int kPlane = kS * kPitch;
constexpr int kPix = kS * kS;
constexpr int kRowWords = kS / 4;
constexpr int kThreads = 1024;
static_assert(kPitch % 4 == 0 && kPitch >= kS && kS % 4 == 0, "rows are walked as dwords");
static_assert(3 * kPlane + 17 * 4 <= 160 * 1024, "the view must fit the LDS of one CU");

struct ViewArgs {
  const uint8_t* crops;
  const hcir_view_params* params;
  float* out;
  float mean[3], std[3];
};

// f(r, g, b) over the 4-pixel groups this thread owns; kWrite: store what f left in r, g, b
template <bool kWrite, typename F>
__device__ __forceinline__ void for_pixels(uint8_t* img, F f) {
  for (int g = threadIdx.x; g < kS * kRowWords; g += kThreads) {
    const int y = g / kRowWords, xw = g - y * kRowWords;
    uint32_t* pr = reinterpret_cast<uint32_t*>(img + y * kPitch) + xw;
    uint32_t* pg = pr + kPlane / 4;
    uint32_t* pb = pg + kPlane / 4;
    const uint32_t R = *pr, G = *pg, B = *pb;
    uint32_t oR = 0, oG = 0, oB = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t r = (R >> (8 * k)) & 255u, gg = (G >> (8 * k)) & 255u, b = (B >> (8 * k)) & 255u;
      f(r, gg, b);
      oR |= r << (8 * k), oG |= gg << (8 * k), oB |= b << (8 * k);
    }
    if (kWrite) *pr = oR, *pg = oG, *pb = oB;
  }
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // red[] of an earlier reduction has been read by everyone
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int i = 0; i < kThreads / 64; ++i) s += red[i];
    red[16] = s;
  }
  __syncthreads();
  return red[16];
}

__global__ __launch_bounds__(kThreads) void simclr_view_kernel(ViewArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[3 * kPlane];
  __shared__ uint32_t red[17];
  const hcir_view_params p = a.params[blockIdx.x];
  const int tid = threadIdx.x;

  // load, the flip folded in: 4 bytes of the HWC crop per thread and step
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.crops + (size_t)blockIdx.x * kPix * 3);
  const bool flip = p.flip != 0;
  for (int w = tid; w < kPix * 3 / 4; w += kThreads) {
    const uint32_t v = __builtin_nontemporal_load(src + w);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * w + k, pix = i / 3, c = i - 3 * pix, y = pix / kS, x = pix - y * kS;
      img[c * kPlane + y * kPitch + (flip ? kS - 1 - x : x)] = (uint8_t)(v >> (8 * k));
    }
  }
  __syncthreads();

  if (p.jitter != 0) {
    for (int k = 0; k < 4; ++k) {
      switch (a.params[blockIdx.x].order[k] & 3) {  // not p.order[k]: a dynamic index would put p into scratch
        case HCIR_VIEW_BRIGHTNESS: {
          const float f = p.brightness;
          for_pixels<true>(img, [f](uint32_t& r, uint32_t& g, uint32_t& b) {
            r = view_blend(0, r, f), g = view_blend(0, g, f), b = view_blend(0, b, f);
          });
          break;
        }
        case HCIR_VIEW_CONTRAST: {
          uint32_t s = 0;
          for_pixels<false>(img, [&s](uint32_t& r, uint32_t& g, uint32_t& b) { s += view_luma(r, g, b); });
          s = block_sum(s, red);
          const uint32_t m = (2 * s + kPix) / (2 * kPix);  // int(mean + 0.5)
          const float f = p.contrast;
          for_pixels<true>(img, [f, m](uint32_t& r, uint32_t& g, uint32_t& b) {
            r = view_blend(m, r, f), g = view_blend(m, g, f), b = view_blend(m, b, f);
          });
          break;
        }
        case HCIR_VIEW_SATURATION: {
          const float f = p.saturation;
          for_pixels<true>(img, [f](uint32_t& r, uint32_t& g, uint32_t& b) {
            const uint32_t l = view_luma(r, g, b);
            r = view_blend(l, r, f), g = view_blend(l, g, f), b = view_blend(l, b, f);
          });
          break;
        }
        default: {
          const uint32_t shift = view_hue_shift(p.hue);
          for_pixels<true>(img, [shift](uint32_t& r, uint32_t& g, uint32_t& b) { view_hue(shift, r, g, b); });
          break;
        }
      }
    }
  }
  if (p.gray != 0)
    for_pixels<true>(img, [](uint32_t& r, uint32_t& g, uint32_t& b) { r = g = b = view_luma(r, g, b); });

  if (p.blur != 0) {
    const int32_t r = p.blur_r != 0 ? 1 : 0;
    const uint32_t ww = p.blur_ww, fw = p.blur_fw;
    const int c = tid / kS, line = tid - c * kS;
    __syncthreads();  // the per-pixel ops wrote with another thread mapping
    if (c < 3) {
      uint8_t* row = img + c * kPlane + line * kPitch;
      for (int pass = 0; pass < 3; ++pass) view_box_line(row, kS, 1, r, ww, fw);
    }
    __syncthreads();
    if (c < 3) {
      uint8_t* col = img + c * kPlane + line;
      for (int pass = 0; pass < 3; ++pass) view_box_line(col, kS, kPitch, r, ww, fw);
    }
  }
  __syncthreads();

  // ToTensor + Normalize: 4 pixels of a plane per thread and step, one 16-byte store
  float* out = a.out + (size_t)blockIdx.x * 3 * kPix;
  for (int g = tid; g < 3 * kS * kRowWords; g += kThreads) {
    const int c = g / (kS * kRowWords), rem = g - c * (kS * kRowWords), y = rem / kRowWords, xw = rem - y * kRowWords;
    const uint32_t v = reinterpret_cast<const uint32_t*>(img + c * kPlane + y * kPitch)[xw];
    const float mean = c == 0 ? a.mean[0] : (c == 1 ? a.mean[1] : a.mean[2]);
    const float std = c == 0 ? a.std[0] : (c == 1 ? a.std[1] : a.std[2]);
    f32x4 o;
    o.x = view_normalize(v & 255u, mean, std);
    o.y = view_normalize((v >> 8) & 255u, mean, std);
    o.z = view_normalize((v >> 16) & 255u, mean, std);
    o.w = view_normalize(v >> 24, mean, std);
    *reinterpret_cast<f32x4*>(out + c * kPix + y * kS + 4 * xw) = o;
  }
}

bool flag01(int32_t v) { return v == 0 || v == 1; }

bool params_ok(const hcir_view_params& p) {
  if (!flag01(p.flip) || !flag01(p.jitter) || !flag01(p.gray) || !flag01(p.blur)) return false;
  int seen = 0;
  for (int k = 0; k < 4; ++k) {
    if (p.order[k] < 0 || p.order[k] > 3) return false;
    seen |= 1 << p.order[k];
  }
  if (seen != 15) return false;
  const float f[3] = {p.brightness, p.contrast, p.saturation};
  for (float v : f)
    if (!(v >= 0.f) || !isfinite(v)) return false;
  if (!(p.hue >= -0.5f && p.hue <= 0.5f)) return false;
  if (p.blur) {
    if (p.blur_r < 0 || p.blur_r > 1) return false;
    // 255 * (all weights) + 2^23 must stay inside 32 bits, as in BoxBlur.c
    if ((uint64_t)(2 * p.blur_r + 1) * p.blur_ww + 2ull * p.blur_fw > (1ull << 24)) return false;
  }
  return true;
}

}  // namespace

extern "C" int hcir_view_blur_weights(float sigma, int32_t* r, uint32_t* ww, uint32_t* fw) {
  if (!r || !ww || !fw || !(sigma > 0.f) || !isfinite(sigma)) return HCIR_ERR_INVALID;
  if (sigma > 2.3f) return HCIR_ERR_UNSUPPORTED;
  view_blur_weights(sigma, *r, *ww, *fw);
  return *r >= 0 && *r <= 1 ? HCIR_OK : HCIR_ERR_UNSUPPORTED;
}

extern "C" int hcir_simclr_view_f32(const uint8_t* crops, const hcir_view_params* params_dev,
                                    const hcir_view_params* params_host, int64_t n, const float* mean3,
                                    const float* std3, float* out, void* stream) {
  HCIR_ENTER();
  if (!crops || !params_dev || !params_host || !mean3 || !std3 || !out || n <= 0 || n > (int64_t(1) << 24))
    return HCIR_ERR_INVALID;
  if (((uintptr_t)crops & 3) || ((uintptr_t)out & 15) || ((uintptr_t)params_dev & 3)) return HCIR_ERR_INVALID;
  for (int64_t i = 0; i < n; ++i)
    if (!params_ok(params_host[i])) return HCIR_ERR_INVALID;
  ViewArgs a{};
  a.crops = crops;
  a.params = params_dev;
  a.out = out;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean3[c];
    a.std[c] = std3[c];
    if (!(a.std[c] != 0.f)) return HCIR_ERR_INVALID;
  }
  hipLaunchKernelGGL(simclr_view_kernel, dim3((unsigned)n), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}
