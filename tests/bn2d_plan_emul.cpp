// bn2d_plan_emul.cpp — csrc/bn2d_plan.h (everything the BatchNorm2d entry points decide before they launch) compiled
// for the host, so that tests/test_bn2d_host.py can check the plan of a table of shapes without a GPU.
#include <stdint.h>

#include "../hair-centric-image-retrieval_amd/csrc/bn2d_plan.h"

extern "C" {

// the status, and the plan's fields in the order of FIELDS in tests/test_bn2d_host.py
int emul_bn2d_plan(int64_t m, int32_t c, int64_t* out) {
  Bn2dPlan p{};
  const int st = bn2d_plan(m, c, &p);
  if (st != HCIR_OK) return st;
  const int64_t f[] = {p.cv, p.wv_log2, p.slabs, p.rpp, p.chunks, p.rows_per_chunk, p.apply_blocks,
                       (int64_t)bn2d_workspace_bytes(p, c)};
  for (unsigned i = 0; i < sizeof(f) / sizeof(f[0]); ++i) out[i] = f[i];
  return st;
}

void emul_bn2d_chunk_rows(int64_t m, int32_t c, int32_t chunk, int64_t* r0, int64_t* r1) {
  Bn2dPlan p{};
  bn2d_plan(m, c, &p);
  bn2d_chunk_rows(p, m, chunk, r0, r1);
}

int emul_bn2d_grid_cap() { return BN2D_GRID_CAP; }

}  // extern "C"
