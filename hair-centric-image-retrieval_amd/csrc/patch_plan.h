// patch_plan.h — host-side route decision of hcir_patch_embed_fused (gemm.hip): whether a patch embedding runs on the
// persistent 256 x 256 tile engine, how many tiles it has, and which token row a patch row is stored to.  Plain C++,
// no device code, so that the arithmetic can be read (and asked for: hcir_patch_embed_route) without the kernels.
#pragma once
#include <stdint.h>

#include "../../include/hcir.h"

constexpr int PATCH_BIG_TN = 256, PATCH_BIG_TM = 256;  // the G256 tile of gemm.hip
constexpr int PATCH_BIG_GRID = 256;                    // persistent: one workgroup per CU

struct PatchPlan {
  int route;      // hcir_patch_route_kind
  int np, t;      // patches and tokens (np + 1) per image
  int64_t rows;   // GEMM rows = b * np (patch rows; the b class-token rows are written by their own kernel)
  int tn, tm;     // BIG: 256 x 256 tiles over d x rows
  int grid;       // BIG: workgroups of the persistent launch
};

// GEMM row m (image m / np, patch m % np) is stored to token row bi * T + 1 + pi = m + m / np + 1: one class-token
// row in front of every image's patches.
static inline int64_t patch_token_row(int64_t m, int np) { return m + m / np + 1; }

// The big route: P == 16 (a 16-B LDS slot = 8 pixels of one image row), fp16 tokens, whole 256-feature n-tiles and a
// weight matrix without k padding (ldw == c * 256: every 64-wide k chunk is four whole image rows of one channel).
// Token rows are indexed in 32 bits by the kernel: b * T stays below 2^31 less one tile.
static inline PatchPlan patch_embed_plan(int64_t b, int c, int h, int w_px, int p, int d, int64_t ldw, int tok_dtype) {
  PatchPlan q;
  q.route = HCIR_PATCH_ROUTE_TILE128;
  q.np = 0;
  q.t = 0;
  q.rows = 0;
  q.tn = q.tm = q.grid = 0;
  if (b <= 0 || c <= 0 || p <= 0 || h <= 0 || w_px <= 0 || d <= 0 || h % p || w_px % p) return q;
  q.np = (h / p) * (w_px / p);
  q.t = q.np + 1;
  q.rows = b * q.np;
  if (p != 16 || tok_dtype != HCIR_F16 || d % PATCH_BIG_TN || ldw != (int64_t)c * 256) return q;
  if (b * q.t > 0x7fffffff - PATCH_BIG_TM) return q;
  // the gather addresses a tile's rows by 32-bit byte offsets from the image of its first row: a tile spans at most
  // 256 / np + 2 images of c * np * 1024 bytes
  if ((int64_t)c * (256 + 2 * (int64_t)q.np) * 1024 > 0x7fffffff) return q;
  const int64_t tiles = (int64_t)(d / PATCH_BIG_TN) * ((q.rows + PATCH_BIG_TM - 1) / PATCH_BIG_TM);
  if (tiles > 0x7fffffff) return q;
  q.route = HCIR_PATCH_ROUTE_BIG;
  q.tn = d / PATCH_BIG_TN;
  q.tm = (int)((q.rows + PATCH_BIG_TM - 1) / PATCH_BIG_TM);
  q.grid = tiles < PATCH_BIG_GRID ? (int)tiles : PATCH_BIG_GRID;
  return q;
}
