// patch_plan_emul.cpp — csrc/patch_plan.h (what hcir_patch_embed_fused decides before it launches) compiled for the
// host, so that tests/test_patch_embed_plan_host.py can check the route, the tile counts and the row remap without a GPU.
#include <stdint.h>

#include "../hair-centric-image-retrieval_amd/csrc/patch_plan.h"

extern "C" {

// route, np, t, rows, tn, tm, grid
void emul_patch_embed_plan(int64_t b, int32_t c, int32_t h, int32_t w_px, int32_t p, int32_t d, int64_t ldw,
                           int tok_dtype, int64_t* out) {
  const PatchPlan q = patch_embed_plan(b, c, h, w_px, p, d, ldw, tok_dtype);
  const int64_t f[] = {q.route, q.np, q.t, q.rows, q.tn, q.tm, q.grid};
  for (unsigned i = 0; i < sizeof(f) / sizeof(f[0]); ++i) out[i] = f[i];
}

int64_t emul_patch_token_row(int64_t m, int32_t np) { return patch_token_row(m, np); }

}  // extern "C"
