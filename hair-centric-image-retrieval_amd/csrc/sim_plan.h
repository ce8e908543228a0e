// sim_plan.h — everything hcir_sim_topk decides before it launches: which flow runs, with which kernel geometry,
// prefix, grids and workspace layout (DESIGN.md "sim_topk: which flow runs when").  Plain C++17 without HIP, so that
// tests/sim_plan_emul.cpp compiles it with g++ and tests/test_sim_plan_host.py pins the plan of a table of shapes on
// the CPU: a wrong grid or prefix still gives exact answers, only slower, and no GPU test would notice.
// csrc/sim_topk.hip fills argument structs from the plan and launches; it derives nothing again.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hcir.h"

static inline int64_t sim_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ----- kernel geometry ------------------------------------------------------
// sim_topk_scan<T, KP, QT, WQ, WGG> serves qb = 32 QT WQ queries per workgroup on tiles of gm = 64 WGG gallery rows
// (sim_core.h SimCfg).  One row per instantiated (list capacity, queries per workgroup); launch_scan / launch_cand in
// sim_topk.hip check their template arguments against it.  The candidate-append kernel keeps no lists: it is the
// KP = 16 instantiation of the same geometry and shares those rows.
struct SimGeom {
  int kp, qb;
  int gm;      // gallery rows per workgroup tile
  int max_wg;  // resident workgroups of a streaming launch (behind a floor); 512 = 2 per CU
};
// Launches that fill their lists from nothing (prefix and single scans, the k > 64 passes) run the batch-insertion
// kernel, two workgroups per CU in every geometry; also <= 576 lists per merge pass.
constexpr int kMaxGridX = 512;
constexpr SimGeom kSimGeom[] = {
    {16, 32, 256, 512},   // <1, 1, 4>
    // 33..64 queries with k <= 16 run as <one query tile x two wave columns> workgroups on 128-row tiles: 24 KB
    // stages, THREE workgroups per CU for the streaming launches (768 workgroups; the floorless launches get the
    // batch-insertion kernel of the one-query-tile geometry, two per CU) instead of two <two query tiles> workgroups
    // with 40 KB stages.  Same-box A/B, 1 M x 768 fp16, 64 queries (tools/ab_sim.py): 318 -> 307 us (the prefix launch
    // 52 -> 38 us; the main scan unchanged at 5.7 TB/s).  Candidate-append scan, C5 at 64 queries: 719 -> 706 us.
    {16, 64, 128, 768},   // <1, 2, 2>
    {16, 128, 128, 512},  // <2, 2, 2>
    {32, 32, 256, 512},   // <1, 1, 4>
    {32, 64, 256, 512},   // <2, 1, 4>
    {32, 128, 128, 512},  // <2, 2, 2>
    {64, 32, 256, 512},   // <1, 1, 4>: 64-entry lists fit one query tile per wave only
};
constexpr SimGeom sim_geom(int kp, int qb) {
  for (const SimGeom& g : kSimGeom)
    if (g.kp == kp && g.qb == qb) return g;
  return SimGeom{0, 0, 0, 0};
}
constexpr int sim_max_parts() {
  int m = kMaxGridX;
  for (const SimGeom& g : kSimGeom) m = g.max_wg > m ? g.max_wg : m;
  return m;
}
constexpr int kMaxParts = sim_max_parts();  // partial lists per query a scan launch can leave in the workspace

constexpr int sim_queries_per_wg(int64_t nq) { return nq <= 32 ? 32 : (nq <= 64 ? 64 : 128); }

// Workgroups along the gallery for `qblocks` query blocks.  Every query block scans every gallery tile; the
// grid is sized so that ALL (tile run, query block) workgroups are resident at once (max_wg slots) and the blocks
// of one tile run sit on the same XCD (linear id = x + grid_x * y, grid_x a multiple of 8): they stream the
// same tiles in step and all but the first read them from that XCD's L2.  (With 512 workgroups per query
// block the blocks ran one after the other and the gallery came from HBM once per block.)
inline int sim_grid_x(int64_t tiles, int64_t qblocks, int max_wg) {
  int64_t cap = max_wg / (qblocks < 1 ? 1 : qblocks);
  cap = cap < 8 ? 8 : (cap & ~int64_t(7));
  return (int)(tiles < cap ? tiles : cap);
}

// ----- candidate buffers ----------------------------------------------------
// candidates per query the big-tile scan can hold: one-element lists of the final merge (with the prefix list 961
// lists, the four-wave kernel at four lists per lane), or the 16 slots per lane of the one-wave select, the last
// of which takes the prefix list
constexpr int kCandLPL = 16;
constexpr int kCandCap = 64 * kCandLPL - 64;  // 960
// candidate-append scans of <= 128 queries with 16 < k <= 64: the floor is the minimum of ceil(k/16) group floors
// (weaker than one k-th score), so more rows clear it
constexpr int kSelLPLBig = 48;
constexpr int kCandCapBig = 64 * kSelLPLBig - 64;  // 3008
constexpr int kSelLPLSmall = 8;
constexpr int kCandCapSmall = 64 * kSelLPLSmall - 64;  // 448: long prefix, k <= 16 (one buffer size for scan AND select)
constexpr int kMaxFloorGroups = 4;

// ----- merge routing ----------------------------------------------------------
// Which kernel of topk_merge.h merges `total_lists` sorted lists per query (the optional extra list counted) into
// `kout` ranks, and how many lists that launch can hold: a launch with fewer slots than lists would silently drop
// lists and return wrong neighbours, so every launcher checks capacity >= total_lists.
enum SimMergeKind {
  SIM_MERGE_NONE = 0,    // no kernel serves the request (capacity 0)
  SIM_MERGE_FOUR_WAVES,  // topk_merge32q_kernel<lpl>: kout <= 16, lane slot j of wave w = list w + 4 (lane + 64 j)
  SIM_MERGE_WAVE,        // topk_merge32_kernel<kMergeLPL>: one wave per query, lane slot j = list lane + 64 j
  SIM_MERGE_SELECT       // topk_merge_sel_kernel<kMergeLPL>: ngroups > 1 interleaved groups of 16-entry lists, kout <= 16
};
constexpr int kMergeLPL = 9;       // lists per lane of the one-wave kernels -> 576 lists (per group)
constexpr int kMergeQuadMaxLPL = 4;  // ... of the four-wave kernel -> up to 1024 lists
struct SimMergeRoute {
  int kind;      // SimMergeKind
  int lpl;       // the kernel's template argument
  int capacity;  // lists the launch reads (all groups together)
};
inline SimMergeRoute sim_merge_route(int total_lists, int kout, int ngroups) {
  if (ngroups > 1)
    return kout <= 16 ? SimMergeRoute{SIM_MERGE_SELECT, kMergeLPL, 64 * kMergeLPL * ngroups} : SimMergeRoute{SIM_MERGE_NONE, 0, 0};
  if (kout <= 16 && total_lists <= 256 * kMergeQuadMaxLPL) {
    const int lpl = total_lists <= 256 ? 1 : (int)sim_cdiv(total_lists, 256);
    return SimMergeRoute{SIM_MERGE_FOUR_WAVES, lpl, 256 * lpl};
  }
  return SimMergeRoute{SIM_MERGE_WAVE, kMergeLPL, 64 * kMergeLPL};
}

// ----- the plan ---------------------------------------------------------------
enum SimFlow {
  SIM_FLOW_SINGLE_SCAN = 0,  // no prefix: one list scan + one merge
  SIM_FLOW_LIST_TWO_PHASE,   // prefix scan -> floor -> list scan behind the floor
  SIM_FLOW_CANDIDATE,        // <= 128 queries: prefix -> floor(s) -> candidate-append scan -> select; gated fallback
  SIM_FLOW_BIG_TILE,         // > 128 queries: list prefix -> 256 x 256 tile scan -> candidate merge; gated fallback
  SIM_FLOW_MULTIPASS         // k > 64: passes of <= 64 ranks below a moving ceiling
};
enum SimSelect {
  SIM_SELECT_NONE = 0,
  SIM_SELECT_WAVE_SMALL,  // topk_select_kernel<kSelLPLSmall>
  SIM_SELECT_WAVE,        // topk_select_kernel<kCandLPL>
  SIM_SELECT_FOUR_WAVES   // topk_select4_kernel: 3008 candidates, four waves per query, 12 + 1 slots per lane
};

struct SimWorkspace {  // the caller's workspace, carved by sim_workspace; every buffer starts on a multiple of 256 bytes
  float* part_val;  // [kMaxParts][nq][kp] partial lists
  int* part_idx;
  float* pre_val;  // [nq][kp] prefix / previous-pass result
  int* pre_idx;
  float* floor_val;  // [kMaxFloorGroups][nq]
  float* ceil_val;   // [nq]
  int* ceil_idx;     // [nq]
  float* cand_val;   // [cand_alloc][nq] candidates behind the prefix floor
  int* cand_idx;
  int* cand_cnt;  // [nq]
  int* overflow;  // [1] behind it
  size_t bytes;
};

struct SimTopkPlan {
  int flow;        // SimFlow
  int kp, qb, gm;  // the list kernel of the list launches (the flow itself, or its fallback): sim_geom(kp, qb)
  int npass;       // passes for k > 64
  int64_t S;       // prefix rows: the flow's first scan covers rows [0, S); == ng without a prefix
  int grid_a;      // workgroups (x) of the floorless list scan: rows [0, S) of two phases, every row of one
  int grid_b;      // ... of the list scan of rows [S, ng) behind the floor (0: one phase)
  // the list launches as fallback of the candidate / big-tile flow, gated by the device overflow flag
  int fallback_phases;  // 0: no fallback; 1: one scan over every row + merge; 2: the two-phase list flow
  int phase_a_done;     // two phases: the flow itself has left phase A's prefix list and floor in the workspace
  // candidate-append flow
  int G;                         // floor groups: 1 (k <= 16) or ceil(k / 16)
  int cand_qb;                   // queries per workgroup of its KP = 16 prefix scan and of the candidate scan
  int cand_grid_a, cand_grid_b;  // workgroups (x) of those two
  int select;                    // SimSelect
  int cand_cap;    // candidates per query the flow's scan may append: kCandCapSmall or cand_alloc
  int cand_alloc;  // ... the workspace holds
  int big_grid_x, big_grid_y;  // big-tile scan
  size_t ws_bytes;             // sim_workspace(...).bytes
};

// The buffers of a call with this plan's list capacity and candidate allocation inside `base` (null: sizes only).
inline SimWorkspace sim_workspace(void* base, int64_t nq, const SimTopkPlan& p) {
  SimWorkspace w{};
  size_t off = 0;
  auto take = [&](size_t n) {
    void* r = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(base) + off);
    off += (n + 255) & ~size_t(255);
    return r;
  };
  const size_t part = (size_t)kMaxParts * nq * p.kp;
  w.part_val = static_cast<float*>(take(part * 4));
  w.part_idx = static_cast<int*>(take(part * 4));
  w.pre_val = static_cast<float*>(take((size_t)nq * p.kp * 4));
  w.pre_idx = static_cast<int*>(take((size_t)nq * p.kp * 4));
  w.floor_val = static_cast<float*>(take((size_t)nq * 4 * kMaxFloorGroups));
  w.ceil_val = static_cast<float*>(take((size_t)nq * 4));
  w.ceil_idx = static_cast<int*>(take((size_t)nq * 4));
  w.cand_val = static_cast<float*>(take((size_t)p.cand_alloc * nq * 4));
  w.cand_idx = static_cast<int*>(take((size_t)p.cand_alloc * nq * 4));
  w.cand_cnt = static_cast<int*>(take(((size_t)nq + 1) * 4));
  w.overflow = w.cand_cnt + nq;
  w.bytes = off;
  return w;
}

// <= 128 queries, k <= 64, big gallery: the candidate-append flow (docs/LAB_NOTEBOOK.md "sim_topk: candidate flow").
// False (plan untouched) when its prefix does not fit the gallery.
inline bool sim_plan_candidate(SimTopkPlan& p, int64_t nq, int64_t ng, int k) {
  const int G = k <= 16 ? 1 : (k + 15) / 16;
  const int qb = sim_queries_per_wg(nq);
  // the prefix is a whole number of 256-row units (128 at 128 queries): whole tiles of both kernels of this qb
  const int unit = qb == 128 ? 128 : 256;
  int cap = p.cand_alloc;
  int64_t S;
  if (G == 1) {
    // Without lists behind the floor a longer prefix costs little (one round of <= 512 one-tile workgroups
    // takes the same ~55 us as half a round) and pays twice: fewer rows for the main scan and r = 7 instead of
    // 15, i.e. <= 38 * 7 candidates per query, a 7-slot select instead of a 15-slot one.
    // (measured, 1 M x 768 fp16: 32 queries 0.314 -> 0.306 ms; at 64 queries the 2-tile-deep list prefix costs
    // what the shorter main scan and select save, 0.330 -> 0.335 ms: N/16 kept there)
    S = qb == 32 ? ng / 8 : ng / 16;
    S = S < 8192 ? 8192 : (S > 131072 ? 131072 : S);
    S = sim_cdiv(S, unit) * unit;
    // expected candidates <= 38 (N - S) / S per query: a small select when the prefix is long
    if (S < ng && 38 * ((ng - S) / S + 1) <= kCandCapSmall) cap = kCandCapSmall;
  } else {
    // Rows at or above the floor, r + 1 = N / S.  The tail probability at a group's 16th best of n rows is
    // ~ Gamma(16) / n (mean 16, sd 4), the floor is the weakest of the G groups: the count is ~ X G (r + 1) with
    // X the largest of G Gamma(16) draws.  P(X > 38) ~ 1e-5 per draw: sized for 38 G (r + 1) <= cap (an
    // earlier 16 G + 5 sigma sizing overflowed a few percent of the QUERIES, and one overflow reruns the call).
    const float per = 38.0f * G;
    int64_t rp1 = (int64_t)((float)cap / per);
    rp1 = rp1 < 2 ? 2 : rp1;
    S = sim_cdiv(ng, rp1);
    S = S < 8192 ? 8192 : S;
    S = sim_cdiv(S, unit) * unit;
  }
  // at least four tiles per floor group, and rows left behind the prefix (both hold for every gallery sim_topk_plan
  // gives a prefix at all, ng >= 32768: 8192 <= S <= max(8192, ng / 8) rounded up)
  if (!(S < ng && sim_cdiv(S, unit) >= 4 * G)) return false;
  const int64_t qblocks = sim_cdiv(nq, qb);
  const SimGeom geo = sim_geom(16, qb);
  p.flow = SIM_FLOW_CANDIDATE;
  p.S = S;
  p.G = G;
  p.cand_qb = qb;
  p.cand_cap = cap;
  p.select = cap == kCandCapSmall ? SIM_SELECT_WAVE_SMALL : (k <= 16 ? SIM_SELECT_WAVE : SIM_SELECT_FOUR_WAVES);
  p.cand_grid_a = sim_grid_x(sim_cdiv(S, geo.gm), qblocks, kMaxGridX);
  // G = 1 scans rows [S, N) with `> floor`, G > 1 ALL rows with `>= floor` (the group lists do not hold the prefix's top-k)
  p.cand_grid_b = sim_grid_x(sim_cdiv(G == 1 ? ng - S : ng, geo.gm), qblocks, geo.max_wg);
  // A gallery whose later rows systematically beat the prefix overflows a buffer: the device flag then gates the
  // list-keeping flow, whose launches are empty otherwise.  G = 1: its second phase only - phase A is exactly the
  // prefix above (same kernel, rows [0, S)).  G > 1 (overflow ~1e-5 per call): the ONE-phase list scan over all rows
  // + one merge - two gated launches that exit at once in the common case, where the two-phase flow cost four
  // (~4.5 us each even when empty: 3 % of a 64-query C5 call).
  const int64_t list_qblocks = sim_cdiv(nq, p.qb);
  p.fallback_phases = G == 1 ? 2 : 1;
  p.phase_a_done = G == 1;
  p.grid_a = G == 1 ? p.cand_grid_a : sim_grid_x(sim_cdiv(ng, p.gm), list_qblocks, kMaxGridX);
  p.grid_b = G == 1 ? sim_grid_x(sim_cdiv(ng - S, p.gm), list_qblocks, sim_geom(p.kp, p.qb).max_wg) : 0;
  return true;
}

// The whole decision for one hcir_sim_topk call (arguments as validated there; any positive sizes are safe).
inline SimTopkPlan sim_topk_plan(int64_t nq, int64_t ng, int d, int k, int dtype, bool has_q_norm, bool has_g_norm) {
  SimTopkPlan p{};
  p.kp = k <= 16 ? 16 : (k <= 32 ? 32 : 64);
  p.npass = (k + 63) / 64;
  p.qb = p.kp == 64 ? 32 : sim_queries_per_wg(nq);
  const SimGeom geo = sim_geom(p.kp, p.qb);
  p.gm = geo.gm;
  p.cand_alloc = (k > 16 && k <= 64 && nq <= 128) ? kCandCapBig : kCandCap;
  p.ws_bytes = sim_workspace(nullptr, nq, p).bytes;
  const int64_t qblocks = sim_cdiv(nq, p.qb);
  p.S = ng;
  p.grid_a = sim_grid_x(sim_cdiv(ng, p.gm), qblocks, kMaxGridX);
  if (p.npass > 1) {
    p.flow = SIM_FLOW_MULTIPASS;
    return p;
  }
  // prefix: ~1/16 of the gallery, at least 64 rows per list-k, in whole tiles
  int64_t S = ng;
  if (ng >= 32768) {
    int64_t s = ng / 16;
    // 64-entry lists: a workgroup's fixed cost (filling the lists from its first tile, then the in-workgroup
    // merge: ~85 us) dwarfs its streaming time, so the prefix is ONE round of at most 64 workgroups x 1 tile;
    // 16 K rows still put the floor within ~k ln(N/16K) insertions per query of the final k-th score
    const int64_t lo = 8192, hi = p.kp == 64 ? 16384 : 131072;
    s = s < lo ? lo : (s > hi ? hi : s);
    s = sim_cdiv(s, p.gm) * p.gm;
    if (s < ng) S = s;
  }
  if (S == ng) {
    p.flow = SIM_FLOW_SINGLE_SCAN;
    return p;
  }
  // Candidate flow against the list-keeping flow, same-box A/B (tools/ab_sim.py, 1 M x 768 fp16, k = 16): 1 query
  // 313 -> 302 us, 32 queries 327 -> 318 us, but 64 queries 333 -> 352 us and 128 queries 443 -> 453 us (two query
  // tiles per wave: the list kernel's main scan is as fast there, and the flow adds two gated launches): k <= 16 takes
  // the candidate flow up to 32 queries only.  k > 16 (1.25 M x 1024, top-50): 1001 -> 639 us at 32 queries,
  // 1662 -> 742 us at 64: always.
  if (nq <= 128 && (k > 16 || nq <= 32) && sim_plan_candidate(p, nq, ng, k)) return p;
  // Many queries (MFMA-bound): the 256 x 256 tile scan collects the rare rows above the prefix floor.  The
  // prefix itself runs on the list-keeping kernel at half that rate, so it is only as long as the candidate
  // buffers require.  With r = rows behind the prefix / prefix rows, the number of rows that beat the
  // prefix's k-th score is negative-binomial: mean k r, variance k r (1 + r) ~ (r sqrt k)^2; r is chosen so that
  // mean + 5 sigma fits the buffer (overflow ~1e-6 per query for a gallery in random order; it is handled: the
  // list scan behind the floor then runs, device-gated, as fallback).
  if (dtype != HCIR_F32 && nq > 128 && k <= 16 && d % 64 == 0 && !has_q_norm && !has_g_norm && ng - S >= 4096) {
    // (measured flat in r = 8..26 at 220 queries: a shorter prefix is paid back by a longer candidate merge;
    // r is capped at 15 - the 1/16 prefix of the list-keeping path - which leaves 11 sigma of headroom)
    int64_t rr = (int64_t)((float)kCandCap / ((float)k + 5.0f * sqrtf((float)k)));
    rr = rr > 15 ? 15 : rr;
    int64_t s = sim_cdiv(ng, (rr < 1 ? 1 : rr) + 1);
    s = s < 8192 ? 8192 : s;
    s = sim_cdiv(s, p.gm) * p.gm;
    if (s < S) S = s;
    p.flow = SIM_FLOW_BIG_TILE;
    p.fallback_phases = 2;
    p.phase_a_done = 1;
    p.cand_cap = kCandCap;
    p.big_grid_y = (int)sim_cdiv(nq, 256);
    // one 128 KB workgroup per CU, every query block of a tile run resident
    p.big_grid_x = sim_grid_x(sim_cdiv(ng - S, 256), p.big_grid_y, 256);
  } else {
    p.flow = SIM_FLOW_LIST_TWO_PHASE;
  }
  p.S = S;
  p.grid_a = sim_grid_x(sim_cdiv(S, p.gm), qblocks, kMaxGridX);
  p.grid_b = sim_grid_x(sim_cdiv(ng - S, p.gm), qblocks, geo.max_wg);
  return p;
}
