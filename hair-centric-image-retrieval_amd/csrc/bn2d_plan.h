// bn2d_plan.h — host-side geometry of the batch-statistics BatchNorm2d kernels (bn2d.hip): which shapes have a kernel,
// how a workgroup's 256 lanes lie over the [M][C] map, how the M rows are cut into chunks, the launch grids and the
// workspace.  Plain C++, no device code: tests/bn2d_plan_emul.cpp compiles it for the host.
//
// The map is fp16 [M = B*H*W][C], a row is C / 8 vectors of 16 bytes.  A wavefront covers `wv` vectors of a row:
// 64 (512 channels of one row) when C % 512 == 0, else the largest of 32, 16, 8 that divides C / 8, over 64 / wv
// consecutive rows.  At C = 64, 128, 256 and every multiple of 512 a wavefront's 1 KB is therefore contiguous; at the
// other multiples of 64 (192, 320, ...) it is 64 / wv segments of wv * 16 >= 128 bytes.  The four wavefronts of a
// workgroup take the same `wv * 8` channels (one slab) of the next rows, so a workgroup covers `rpp` = 4 * 64 / wv rows
// per pass.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hcir.h"

constexpr int BN2D_THREADS = 256;
constexpr int BN2D_GRID_CAP = 8 * 256;   // memory-bound: about 8 workgroups per CU over 256 CUs, striding over the rest
constexpr int BN2D_MIN_PASSES = 4;       // a chunk is at least this many passes of its workgroup (when M allows)

struct Bn2dPlan {
  int32_t cv;               // vectors per row: C / 8
  int32_t wv_log2;          // log2 of the vectors of one row a wavefront covers: 3 .. 6
  int32_t slabs;            // channel slabs: cv >> wv_log2
  int32_t rpp;              // rows a workgroup covers per pass: 4 * (64 >> wv_log2)
  int32_t chunks;           // contiguous row ranges of the reductions
  int64_t rows_per_chunk;   // multiple of rpp; only the last chunk may hold fewer
  int32_t apply_blocks;     // row blocks of the elementwise kernels (grid = apply_blocks * slabs)
};

// HCIR_OK and *p filled, or the status the entry points return for the shape.
static inline int bn2d_plan(int64_t m, int32_t c, Bn2dPlan* p) {
  if (m < 1 || c < 1) return HCIR_ERR_INVALID;
  if (c < 64 || c % 64 != 0 || c > (1 << 16) || m > INT32_MAX) return HCIR_ERR_UNSUPPORTED;
  if (m < 2) return HCIR_ERR_INVALID;   // one value per channel has no variance: torch refuses it in training too
  p->cv = c / 8;
  p->wv_log2 = p->cv % 64 == 0 ? 6 : p->cv % 32 == 0 ? 5 : p->cv % 16 == 0 ? 4 : 3;
  p->slabs = p->cv >> p->wv_log2;
  p->rpp = 4 * (64 >> p->wv_log2);
  const int64_t cap = BN2D_GRID_CAP / p->slabs > 0 ? BN2D_GRID_CAP / p->slabs : 1;   // row blocks the grid cap allows
  const int64_t passes = (m + p->rpp - 1) / p->rpp;
  int64_t chunks = (passes + BN2D_MIN_PASSES - 1) / BN2D_MIN_PASSES;
  chunks = chunks > cap ? cap : chunks;
  p->rows_per_chunk = ((passes + chunks - 1) / chunks) * p->rpp;
  p->chunks = (int32_t)((m + p->rows_per_chunk - 1) / p->rows_per_chunk);
  p->apply_blocks = (int32_t)(passes > cap ? cap : passes);
  return HCIR_OK;
}

// Rows [*r0, *r1) of a chunk.
static inline void bn2d_chunk_rows(const Bn2dPlan& p, int64_t m, int32_t chunk, int64_t* r0, int64_t* r1) {
  *r0 = chunk * p.rows_per_chunk;
  *r1 = *r0 + p.rows_per_chunk < m ? *r0 + p.rows_per_chunk : m;
}

// workspace[chunk][C][2] fp32: (mean, M2) in the forward, (sum g, sum g (x - mean)) in the backward.
static inline size_t bn2d_workspace_bytes(const Bn2dPlan& p, int32_t c) {
  return (size_t)p.chunks * c * 2 * sizeof(float);
}
