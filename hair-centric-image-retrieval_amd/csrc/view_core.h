// view_core.h — the per-pixel arithmetic of one SimCLR view (include/hcir.h "SimCLR training views"), usable from host
// and device: csrc/view.hip runs it on the LDS image of a view, tests/view_emul.cpp compiles it with g++ and compares
// it with live Pillow byte for byte.
//
// Every function restates what Pillow executes for the op torchvision / lightly call on a PIL image
// (HP/mainpretrain.py:130: lightly SimCLRTransform(input_size=224); HP/utils/dataloader.py:36-38):
//   ImageEnhance.Brightness / Contrast / Color -> Image.blend -> libImaging/Blend.c      view_blend
//   Image.convert("L")                           libImaging/Convert.c L24                 view_luma
//   Image.convert("HSV") / convert("RGB")        libImaging/Convert.c rgb2hsv / hsv2rgb   view_rgb2hsv / view_hsv2rgb
//   ImageFilter.GaussianBlur                     libImaging/BoxBlur.c                     view_blur_weights, view_box_line
// C promotes float operands of an expression with a double literal to double; where Pillow's source does that the
// code below says `double` in so many words.  No statement here may be contracted into an fma.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VHD __host__ __device__ __forceinline__
#else
#define VHD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// Convert.c: #define L24(rgb) ((rgb)[0] * 19595 + (rgb)[1] * 38470 + (rgb)[2] * 7471 + 0x8000); L = L24 >> 16
VHD uint32_t view_luma(uint32_t r, uint32_t g, uint32_t b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }

// Blend.c, in1 = the degenerate image's value d, in2 = the pixel's x, alpha = the enhancement factor (a float):
// inside [0, 1] the sum cannot leave 0..255 and is truncated; outside, it is clipped first.
VHD uint32_t view_blend(uint32_t d, uint32_t x, float f) {
  const float diff = (float)((int32_t)x - (int32_t)d);
  const float prod = f * diff;
  const float t = (float)(int32_t)d + prod;
  if (f >= 0.f && f <= 1.0f) return (uint32_t)(int32_t)t & 255u;
  if (t <= 0.f) return 0u;
  if (t >= 255.0f) return 255u;
  return (uint32_t)(int32_t)t;
}

VHD uint32_t view_clip8(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// Convert.c rgb2hsv_row
VHD void view_rgb2hsv(uint32_t r, uint32_t g, uint32_t b, uint32_t& uh, uint32_t& us, uint32_t& uv) {
  const uint32_t maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const uint32_t minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  uv = maxc;
  if (minc == maxc) {
    uh = us = 0;
    return;
  }
  const float cr = (float)(int32_t)(maxc - minc);
  const float s = cr / (float)(int32_t)maxc;
  const float rc = (float)(int32_t)(maxc - r) / cr;
  const float gc = (float)(int32_t)(maxc - g) / cr;
  const float bc = (float)(int32_t)(maxc - b) / cr;
  float h;
  if (r == maxc) {
    h = bc - gc;
  } else if (g == maxc) {
    const double a = 2.0 + (double)rc;
    h = (float)(a - (double)bc);
  } else {
    const double a = 4.0 + (double)gc;
    h = (float)(a - (double)rc);
  }
  const double q = (double)h / 6.0;
  const double w = q + 1.0;              // in [5/6, 11/6]: fmod(w, 1.0) == w - floor(w), exactly
  h = (float)(w - floor(w));
  uh = view_clip8((int32_t)((double)h * 255.0));
  us = view_clip8((int32_t)((double)s * 255.0));
}

// Convert.c hsv2rgb: round() of a non-negative double is floor(x + 0.5)
VHD uint32_t view_round8(double x) { return view_clip8((int32_t)floor(x + 0.5)); }

VHD void view_hsv2rgb(uint32_t h, uint32_t s, uint32_t v, uint32_t& r, uint32_t& g, uint32_t& b) {
  if (s == 0) {
    r = g = b = v;
    return;
  }
  const double h6 = (double)(float)(int32_t)h * 6.0 / 255.0;
  const int32_t i = (int32_t)floor(h6);
  const float f = (float)(h6 - (double)(float)i);
  const float fs = (float)((double)(float)(int32_t)s / 255.0);
  const double fv = (double)(float)(int32_t)v;
  const double ep = 1.0 - (double)fs;
  const double mq = (double)fs * (double)f;
  const double eq = 1.0 - mq;
  const double ft = 1.0 - (double)f;
  const double mt = (double)fs * ft;
  const double et = 1.0 - mt;
  const uint32_t p = view_round8(fv * ep), q = view_round8(fv * eq), t = view_round8(fv * et);
  switch (i % 6) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
}

// torchvision adjust_hue on a PIL image: H += uint8(hue_factor * 255) modulo 256, S and V kept
VHD uint32_t view_hue_shift(float hue) { return (uint32_t)(int32_t)((double)hue * 255.0) & 255u; }

VHD void view_hue(uint32_t shift, uint32_t& r, uint32_t& g, uint32_t& b) {
  uint32_t h, s, v;
  view_rgb2hsv(r, g, b, h, s, v);
  view_hsv2rgb((h + shift) & 255u, s, v, r, g, b);
}

// BoxBlur.c: ImagingGaussianBlur(radius = sigma, passes = 3) -> _gaussian_blur_radius -> ImagingLineBoxBlur8's
// weights.  r = whole pixels each side, ww = 2^24 / (2 rho + 1), fw = what the two far pixels get.
VHD void view_blur_weights(float sigma, int32_t& r, uint32_t& ww, uint32_t& fw) {
  const float sigma2 = sigma * sigma / 3;
  const float L = (float)sqrt(12.0 * (double)sigma2 + 1.0);
  const float l = (float)floor(((double)L - 1.0) / 2.0);
  float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
  a /= 6 * (sigma2 - (l + 1) * (l + 1));
  const float rho = l + a;
  r = (int32_t)rho;
  ww = (uint32_t)((float)(1u << 24) / (rho * 2 + 1));
  fw = ((1u << 24) - (uint32_t)(r * 2 + 1) * ww) / 2;
}

// One output of a box pass with 0 <= r <= 1.  m2 .. p2 = in[x - 2] .. in[x + 2], already clamped at the line's ends.
VHD uint32_t view_box(uint32_t m2, uint32_t m1, uint32_t c, uint32_t p1, uint32_t p2, int32_t r, uint32_t ww,
                      uint32_t fw) {
  const uint32_t acc = r ? m1 + c + p1 : c;
  const uint32_t far = r ? m2 + p2 : m1 + p1;
  return (acc * ww + far * fw + (1u << 23)) >> 24;
}

// One box pass over a line of n >= 1 bytes at stride `step`, in place: the inputs a later output still needs are the
// last three bytes read, kept in registers.
template <typename P>
VHD void view_box_line(P line, int32_t n, int32_t step, int32_t r, uint32_t ww, uint32_t fw) {
  uint32_t m2 = line[0], m1 = m2, c = m2;
  uint32_t p1 = line[(n > 1 ? 1 : 0) * step], p2 = line[(n > 2 ? 2 : n - 1) * step];
  for (int32_t x = 0; x < n; ++x) {
    const uint32_t o = view_box(m2, m1, c, p1, p2, r, ww, fw);
    const int32_t nx = x + 3 < n ? x + 3 : n - 1;
    const uint32_t p3 = line[nx * step];
    line[x * step] = (uint8_t)o;
    m2 = m1, m1 = c, c = p1, p1 = p2, p2 = p3;
  }
}

// ToTensor + Normalize: hcir_knn_transform_u8's arithmetic (IEEE fp32 division)
VHD float view_normalize(uint32_t x, float mean, float std) {
  const float v = (float)(int32_t)x / 255.0f;
  return (v - mean) / std;
}
