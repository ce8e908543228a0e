// stem_plan.h — host-side geometry of the train-mode stem kernels (stem_train.hip): sizes of the conv and pooled maps,
// the tiles the workgroups take, and how the weight gradient's conv tiles are dealt to its persistent parts.  Plain
// C++, no device code, so that the arithmetic can be read without the kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hcir.h"
#include "conv_plan.h"   // stem_conv_size, stem_pool_size, STEM_K, STEM_KP

constexpr int STEMT_TC = 16;                       // conv tile edge: 256 conv pixels = 8 MFMA row tiles, no overlap
constexpr int STEMT_TI = 2 * (STEMT_TC - 1) + 7;   // input patch edge (37)
constexpr int STEMT_PATCH = 3 * STEMT_TI * STEMT_TI;   // 4107 halves; pixel base <= 1140, tap offset <= 2966
constexpr int STEMT_TP = 8;                        // pooled tile edge of the pool backward: 16 x 16 conv pixels,
                                                   // 9 x 9 windows with the one-window halo
constexpr int STEM_WG_MIN_TILES = 4;               // a part is at least this many conv tiles (when there are that many):
                                                   // its 37 KB partial tile is then the smaller part of its traffic
constexpr int STEM_WG_PARTS_CAP = 2 * 256;         // persistent parts: two workgroups of 200 VGPRs a lane fit a CU, 256 CUs
constexpr int STEM_DW = 64 * STEM_K;               // dw elements, torch's [64][3][7][7]

struct StemPlan {
  int32_t hc, wc, hp, wp;      // conv map, pooled map
  int32_t tiles_y, tiles_x;    // conv tiles of STEMT_TC per image
  int64_t tiles;               // b * tiles_y * tiles_x
};

// Statuses of the entry points that take the image's size.
static inline int stem_plan(int64_t b, int32_t h, int32_t w, StemPlan* p) {
  if (b < 1 || h < 1 || w < 1) return HCIR_ERR_INVALID;
  if (h < 7 || w < 7) return HCIR_ERR_UNSUPPORTED;
  p->hc = stem_conv_size(h);
  p->wc = stem_conv_size(w);
  p->hp = stem_pool_size(h);
  p->wp = stem_pool_size(w);
  p->tiles_y = (p->hc + STEMT_TC - 1) / STEMT_TC;
  p->tiles_x = (p->wc + STEMT_TC - 1) / STEMT_TC;
  p->tiles = b * (int64_t)p->tiles_y * p->tiles_x;
  // 32-bit block indices, and b * h * w * 64 halves addressed in int64 from int32 coordinates
  if (p->tiles > INT32_MAX || b > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  return HCIR_OK;
}

// Statuses of the entry points that take the conv map's size: hc < 4 is an image with H < 7.
static inline int stem_map_plan(int64_t b, int32_t hc, int32_t wc, int32_t* hp, int32_t* wp) {
  if (b < 1 || hc < 1 || wc < 1) return HCIR_ERR_INVALID;
  if (hc < 4 || wc < 4) return HCIR_ERR_UNSUPPORTED;
  *hp = (hc - 1) / 2 + 1;
  *wp = (wc - 1) / 2 + 1;
  if (b * (int64_t)hc * wc > ((int64_t)1 << 34) || b > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  return HCIR_OK;
}

struct StemWgradPlan {
  int64_t tiles_per_part;   // only the last part may hold fewer
  int32_t parts;
};

static inline void stem_wgrad_plan(const StemPlan& s, StemWgradPlan* p) {
  int64_t per = (s.tiles + STEM_WG_PARTS_CAP - 1) / STEM_WG_PARTS_CAP;
  per = per < STEM_WG_MIN_TILES ? STEM_WG_MIN_TILES : per;
  p->tiles_per_part = per;
  p->parts = (int32_t)((s.tiles + per - 1) / per);
}

static inline size_t stem_wgrad_workspace_bytes(const StemWgradPlan& p) {
  return p.parts > 1 ? (size_t)p.parts * STEM_DW * sizeof(float) : 0;   // one part writes dw itself
}
