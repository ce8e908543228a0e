// conv_plan.h — host-side geometry of the ResNet convolution kernels (conv.hip, conv_bwd.hip): which requests a kernel
// exists for, output sizes, tile choice, M splits and launch grid.  Plain C++, no device code, so that the arithmetic
// can be read (and restated in Python, hcir/resnet_engine.py) without the kernels.
#pragma once
#include <stdint.h>

#include "../../include/hcir.h"

struct ConvPlan {
  int32_t ho, wo;     // output height / width
  int64_t m;          // GEMM rows: B * ho * wo
  int32_t k;          // GEMM depth: R * S * Cin, in (r, s, c) order
  int32_t bn;         // N tile: 128 when Cout % 128 == 0 and the grid still covers the chip, else 64
  int64_t grid_m;     // M tiles of CONV_BM rows
  int32_t grid_n;
};

constexpr int CONV_BM = 128;   // output pixels per workgroup
constexpr int CONV_BK = 64;    // K step: 64 channels of ONE tap (Cin % 64 == 0, so a step never crosses a tap)

static inline int32_t conv_out_size(int32_t in, int32_t r, int32_t stride, int32_t pad) {
  return (in + 2 * pad - r) / stride + 1;
}

// HCIR_OK and *p filled, or the status the entry point returns.
static inline int conv_plan(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r, int32_t s,
                            int32_t stride, int32_t pad, ConvPlan* p) {
  if (b < 1 || h < 1 || w < 1 || cin < 1 || cout < 1) return HCIR_ERR_INVALID;
  const bool k1 = (r == 1 && s == 1 && pad == 0), k3 = (r == 3 && s == 3 && pad == 1);
  if (!(k1 || k3) || (stride != 1 && stride != 2) || cin % 64 != 0 || cout % 64 != 0) return HCIR_ERR_UNSUPPORTED;
  p->ho = conv_out_size(h, r, stride, pad);
  p->wo = conv_out_size(w, s, stride, pad);
  p->m = b * (int64_t)p->ho * p->wo;
  p->k = r * s * cin;
  // 32-bit indices inside the kernel: pixel rows and weight rows are addressed as int32 row * pitch in int64
  if (p->m > (int64_t)1 << 30 || b * (int64_t)h * w > (int64_t)1 << 30) return HCIR_ERR_UNSUPPORTED;
  p->grid_m = (p->m + CONV_BM - 1) / CONV_BM;
  // the wider tile halves the A re-reads, but only once 128-wide tiles still give every CU (256) two workgroups
  p->bn = (cout % 128 == 0 && p->grid_m * (cout / 128) >= 512) ? 128 : 64;
  p->grid_n = cout / p->bn;
  return HCIR_OK;
}

// Weight gradient (conv_bwd.hip): per tap a [Cout] x [Cin] product contracted over the M = B * ho * wo output pixels.
struct WgradPlan {
  int32_t ho, wo;
  int64_t m;
  int32_t k;               // row length of dw: R * S * Cin
  int32_t tn, tc;          // output tile: tn output channels x tc input channels of one tap
  int32_t taps;            // R * S
  int32_t tiles;           // (Cout / tn) * (Cin / tc) * taps
  int32_t splits;          // workgroups along M per tile
  int64_t rows_per_split;  // multiple of WGRAD_BM; only the last split may hold fewer
};

constexpr int WGRAD_BM = 64;        // output pixels per main-loop step
constexpr int WGRAD_TARGET = 512;   // workgroups wanted at least: two per CU

static inline int wgrad_plan(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r, int32_t s,
                             int32_t stride, int32_t pad, WgradPlan* p) {
  ConvPlan f;
  const int st = conv_plan(b, h, w, cin, cout, r, s, stride, pad, &f);   // the forward's shapes, the forward's statuses
  if (st != HCIR_OK) return st;
  p->ho = f.ho;
  p->wo = f.wo;
  p->m = f.m;
  p->k = f.k;
  p->tn = cout % 128 == 0 ? 128 : 64;
  p->tc = cin % 128 == 0 ? 128 : 64;
  p->taps = r * s;
  const int64_t tiles = (int64_t)(cout / p->tn) * (cin / p->tc) * p->taps;
  if (tiles > (1 << 20)) return HCIR_ERR_UNSUPPORTED;
  p->tiles = (int32_t)tiles;
  // layer1's 3x3 is 9 tiles: M is cut until the grid has WGRAD_TARGET workgroups, but never below one step per split
  const int64_t steps = (p->m + WGRAD_BM - 1) / WGRAD_BM;
  int64_t splits = (WGRAD_TARGET + tiles - 1) / tiles;
  splits = splits > steps ? steps : splits;
  p->rows_per_split = ((steps + splits - 1) / splits) * WGRAD_BM;
  p->splits = (int32_t)((p->m + p->rows_per_split - 1) / p->rows_per_split);
  return HCIR_OK;
}

static inline size_t wgrad_workspace_bytes(const WgradPlan& p, int32_t cout) {
  return p.splits > 1 ? (size_t)p.splits * cout * p.k * sizeof(float) : 0;   // one split writes dw itself
}

// Stem: conv 7x7 / 2 / pad 3 then maxpool 3x3 / 2 / pad 1.
constexpr int STEM_TP = 7;                     // pooled tile edge per workgroup
constexpr int STEM_TC = 2 * STEM_TP + 1;       // conv tile edge (15): pooled row p reads conv rows 2p-1 .. 2p+1
constexpr int STEM_TI = 2 * (STEM_TC - 1) + 7; // input patch edge (35)
constexpr int STEM_K = 147, STEM_KP = 160;     // 3 * 7 * 7 taps, padded to 10 MFMA steps of 16

static inline int32_t stem_conv_size(int32_t in) { return (in - 1) / 2 + 1; }       // (in + 6 - 7) / 2 + 1
static inline int32_t stem_pool_size(int32_t in) { return (stem_conv_size(in) - 1) / 2 + 1; }
