// sim_plan_emul.cpp — csrc/sim_plan.h (everything hcir_sim_topk decides before it launches) compiled for the host, so
// that tests/test_sim_plan_host.py can pin the plan of a table of shapes without a GPU.
#include <stdint.h>

#include "../hair-centric-image-retrieval_amd/csrc/sim_plan.h"

extern "C" {

// the plan's fields in the order of FIELDS in tests/test_sim_plan_host.py
void emul_sim_topk_plan(int64_t nq, int64_t ng, int32_t d, int32_t k, int dtype, int has_q_norm, int has_g_norm,
                        int64_t* out) {
  const SimTopkPlan p = sim_topk_plan(nq, ng, d, k, dtype, has_q_norm != 0, has_g_norm != 0);
  const int64_t f[] = {p.flow, p.kp, p.qb, p.gm, p.npass, p.S, p.grid_a, p.grid_b, p.fallback_phases, p.phase_a_done,
                       p.G, p.cand_qb, p.cand_grid_a, p.cand_grid_b, p.select, p.cand_cap, p.cand_alloc, p.big_grid_x,
                       p.big_grid_y, (int64_t)p.ws_bytes};
  for (unsigned i = 0; i < sizeof(f) / sizeof(f[0]); ++i) out[i] = f[i];
}

// byte offsets of the workspace buffers, in the order they are carved, then the overflow flag's and the total
void emul_sim_workspace_layout(int64_t nq, int32_t kp, int32_t cand_alloc, int64_t* out) {
  SimTopkPlan p{};
  p.kp = kp;
  p.cand_alloc = cand_alloc;
  const SimWorkspace w = sim_workspace(nullptr, nq, p);
  const void* f[] = {w.part_val, w.part_idx, w.pre_val,  w.pre_idx,  w.floor_val, w.ceil_val,
                     w.ceil_idx, w.cand_val, w.cand_idx, w.cand_cnt, w.overflow};
  for (unsigned i = 0; i < sizeof(f) / sizeof(f[0]); ++i) out[i] = (int64_t)reinterpret_cast<uintptr_t>(f[i]);
  out[11] = (int64_t)w.bytes;
}

// the candidate flow's own guard on a plan whose list part is filled in: 1 when the flow was planned
int emul_sim_plan_candidate(int64_t nq, int64_t ng, int32_t k, int64_t* S) {
  SimTopkPlan p = sim_topk_plan(nq, ng, 768, k, HCIR_F16, false, false);
  p.flow = -1;
  p.S = -1;
  const bool ok = sim_plan_candidate(p, nq, ng, k);
  *S = p.S;
  return ok ? 1 : 0;
}

int emul_geom(int32_t kp, int32_t qb, int32_t* gm, int32_t* max_wg) {
  const SimGeom g = sim_geom(kp, qb);
  *gm = g.gm;
  *max_wg = g.max_wg;
  return g.kp == kp && g.qb == qb && kp != 0;
}

int emul_max_parts() { return kMaxParts; }

}  // extern "C"
