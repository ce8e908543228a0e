// topk_merge.h — the merge and select kernels behind the sim_topk scans (device code, included by sim_topk.hip).
//
//   topk_merge32_kernel<9>      sorted partial lists -> top-k, one wave per query (16 < kout <= 64)
//   topk_merge32q_kernel<1..4>  the same with four waves per query (kout <= 16, up to 1024 lists)
//   topk_merge_sel_kernel<9>    sorted 16-entry lists -> per-group top-k by selection (group floors of the k > 16 prefix)
//   topk_select_kernel<8|16>    UNSORTED candidate buffer (+ the sorted prefix list) -> top-k, one wave per query
//   topk_select4_kernel<13>     the same with four waves per query (3008-entry buffers)
//   topk_merge_kernel           64-bit indices: the cross-shard merge behind hcir_topk_merge
// Which one a launch gets is sim_merge_route / SimTopkPlan::select in sim_plan.h; the pieces they are made of - list
// reader, round loop, rank by counting, result writer, prologue - each exist once, below.
#pragma once
#include "common.h"
#include "sim_plan.h"

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

// (score, row) as ONE 64-bit key: [orderable(score) : ~row]; "better" (score desc, row asc) is the unsigned
// maximum, an empty slot is key 0.  Used by the in-workgroup and the final merges.
__device__ __forceinline__ uint64_t merge_key(float v, int id) {
  if (id < 0) return 0ull;
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
}
__device__ __forceinline__ float merge_key_val(uint64_t k) {
  uint32_t u = (uint32_t)(k >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ int merge_key_idx(uint64_t k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }

// ----- wave primitives --------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_max_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, true);
  const uint64_t o = ((uint64_t)hi << 32) | lo;
  return o > v ? o : v;
}
// maximum over the 64 lanes, returned wave-uniform: 4 DPP butterfly steps inside each row of 16 lanes + 4 v_readlane
// + scalar max (instead of 18 ds_bpermute per round)
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = dpp_max_u64<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_max_u64<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_max_u64<0x141>(v);  // row_half_mirror
  v = dpp_max_u64<0x140>(v);  // row_mirror: every lane of a 16-lane row now holds the row maximum
  uint64_t m = 0;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 16 * row);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 16 * row);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    m = o > m ? o : m;
  }
  return m;
}
// wave-uniform sum of an int over the 64 lanes: four DPP steps inside each row of 16 lanes, then four v_readlane.
// (A __shfl_xor butterfly is six dependent ds_bpermute round trips: the 32-step searches below spent 11 us in them.)
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror: every lane holds its row's sum
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}
// rank by counting: how many of the wave's 64 keys are larger than this lane's (64 readlane compares).  Distinct
// nonzero keys get the ranks 0, 1, ...; every empty lane (key 0) gets the number of nonzero keys.
// UNROLL: the selects run it 8 steps at a time, the four-wave merge fully unrolled (as measured when they were written).
template <int UNROLL>
__device__ __forceinline__ int wave_rank_u64(uint64_t key) {
  int rank = 0;
#pragma unroll UNROLL
  for (int i = 0; i < 64; ++i) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), i);
    rank += ((((uint64_t)hi << 32) | lo) > key) ? 1 : 0;
  }
  return rank;
}
// lanes below this one whose bit is set in a ballot mask
__device__ __forceinline__ int lanes_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ----- arguments, prologue, result writer ----------------------------------------
struct TopkOut {
  float* val;        // [rows][k]
  int64_t* idx;      // final output (idx_base added; -1 stays -1), and / or
  int* idx32;        // intermediate output
  float* kth_val;    // optional [rows]: value of rank k - 1 (floor for the main scan)
  int* kth_idx;      // optional [rows]
  int k;             // (in front of idx_base: the round loops wait for k, and one 64-B scalar load of a merge kernel's
  int64_t idx_base;  //  arguments ends here; idx_base is needed by the final stores only)
};
struct TopkGate {
  const int* flag;   // optional device flag: the launch runs only if (*flag != 0) == (want != 0)
  int want;
};

struct MergeArgs {
  const float* vals;     // lists [nlists][nq][kin] sorted (score desc, row asc), empty slots have idx < 0
  const int* idx;
  TopkOut out;           // out.k = kout
  int64_t nq;
  int nlists, kin;
  // optional extra list per query (the prefix result), [nq][kin_extra]
  const float* extra_val;
  const int* extra_idx;
  int kin_extra;
  const int* nlists_q;   // optional [nq]: lists of this query = min(nlists_q[q], nlists) (candidate buffers)
  TopkGate gate;
  int* zero_cnt;         // optional [nq + 1]: cleared here (candidate counters + overflow flag of the big scan)
  int ngroups;           // topk_merge_sel_kernel only, > 1: blockIdx.y = group g merges lists g, g + ngroups, ... into
                         //      out[g][nq][kout], kth_val[g][nq] (group floors of the prefix); 0 / 1: one group
};

// select: the candidate buffers a candidate-append scan leaves, cap = 64 (LPL - 1)
struct SelectArgs {
  const float* cand_val;   // [nq][cap] (query-major: a query's candidates are contiguous)
  const int* cand_idx;
  const int* cand_cnt;
  int cap;
  const float* pre_val;  // optional [nq][kpre], sorted
  const int* pre_idx;
  int kpre;
  TopkOut out;           // the caller's output only
  int64_t nq;
  TopkGate gate;
};

// Prologue of every merge / select kernel: false when the launch is gated off (uniform: every wave of the grid
// reads the same flag) or has no rank to write; `clears` names the one thread per query that zeroes the counters.
// (The test of k also brings k in with the kernel's other arguments: left to its first use, the bound of the round
// loop, hipcc loads it alone right in front of the loop, one more scalar-load round trip on a 9 us kernel.)
__device__ __forceinline__ bool topk_enter(const TopkGate& g, const TopkOut& out, int* zero_cnt, int64_t qi, int64_t nq,
                                           bool clears) {
  if (g.flag && ((*g.flag != 0) != (g.want != 0))) return false;
  if (out.k <= 0) return false;
  if (zero_cnt && clears) {
    zero_cnt[qi] = 0;
    if (qi == 0) zero_cnt[nq] = 0;
  }
  return true;
}

// Output `slot` of row `row`; key 0 is an empty slot: -inf, -1 (and -1 WITHOUT idx_base in the 64-bit output).
__device__ __forceinline__ void store_result(const TopkOut& o, int64_t row, int slot, uint64_t key) {
  const bool none = key == 0ull;
  const float wv = none ? kNegInf : merge_key_val(key);
  const int wi = none ? -1 : merge_key_idx(key);
  o.val[row * o.k + slot] = wv;
  if (o.idx) o.idx[row * o.k + slot] = none ? -1 : (int64_t)wi + o.idx_base;
  if (o.idx32) o.idx32[row * o.k + slot] = wi;
  if (slot == o.k - 1) {
    if (o.kth_val) o.kth_val[row] = wv;
    if (o.kth_idx) o.kth_idx[row] = wi;
  }
}

// ----- list reader ------------------------------------------------------------------
struct ListSpan {
  const float* val;
  const int* idx;
  int len;  // 0: no such list
};
// List `list` of query qi in group `grp` of `ngroups`: lists [0, nl) are the group's partial lists, list nl is the
// optional extra list.
__device__ __forceinline__ ListSpan merge_list_span(const MergeArgs& a, int64_t qi, int list, int nl, int ngroups = 1,
                                                    int grp = 0) {
  if (list < nl) {
    const int64_t o = ((int64_t)(list * ngroups + grp) * a.nq + qi) * a.kin;
    return ListSpan{a.vals + o, a.idx + o, a.kin};
  }
  if (a.extra_val && list == nl) return ListSpan{a.extra_val + qi * a.kin_extra, a.extra_idx + qi * a.kin_extra, a.kin_extra};
  return ListSpan{nullptr, nullptr, 0};
}
// entries [pos, pos + 4) of a list as keys (0 where the list has ended)
__device__ __forceinline__ void fetch4(const ListSpan& s, int pos, uint64_t (&k4)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) k4[e] = 0ull;
  if (pos + 4 <= s.len && (s.len & 3) == 0) {  // whole 16-B groups (lists of 16 / 32 / 64 entries)
    const f32x4 v = *reinterpret_cast<const f32x4*>(s.val + pos);
    const u32x4 id = *reinterpret_cast<const u32x4*>(s.idx + pos);
#pragma unroll
    for (int e = 0; e < 4; ++e) k4[e] = merge_key(v[e], (int)id[e]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (pos + e < s.len) k4[e] = merge_key(s.val[pos + e], s.idx[pos + e]);
  }
}

// ----- round loop -----------------------------------------------------------------------
// out.k rounds of wave maximum over the cached heads of the wave's lists; slot j of this lane holds list list_of(j).
//   * the first FOUR entries of each list are fetched up front as two 16-B loads: the rounds then run from registers
//     (re-fetching the winner's next entry from memory in every round cost ~1.5 us each); a list whose four are
//     used up is refilled in place (rare);
//   * sink(o, key) receives the winner of round o (0: the lists are exhausted), wave-uniform.  The sink must NOT
//     store to global memory in every round: the refill load shares the counter, so hipcc puts `s_waitcnt vmcnt(0)`
//     in front of every round and each waits for a store round trip (~1.1 us per round, 18-23 us per merge of 16 ranks
//     and 55 us per merge of 50).  Winners are kept in registers and leave 64 per store instruction.
template <int LPL, typename ListOf, typename Sink>
__device__ __forceinline__ void merge_rounds(const MergeArgs& a, int64_t qi, int nl, ListOf list_of, Sink sink) {
  uint64_t kq[LPL][4];
  int used[LPL];
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    used[j] = 0;
    fetch4(merge_list_span(a, qi, list_of(j), nl), 0, kq[j]);
  }
  for (int o = 0; o < a.out.k; ++o) {
    uint64_t best = kq[0][0];
    int bj = 0;
#pragma unroll
    for (int j = 1; j < LPL; ++j) {
      const bool take = kq[j][0] > best;
      best = take ? kq[j][0] : best;
      bj = take ? j : bj;
    }
    const uint64_t wm = wave_max_u64(best);
    sink(o, wm);
    if (wm != 0ull && best == wm) {  // row indices are unique: exactly one lane and one list hold the winner
#pragma unroll
      for (int j = 0; j < LPL; ++j) {
        if (j == bj) {
          kq[j][0] = kq[j][1];
          kq[j][1] = kq[j][2];
          kq[j][2] = kq[j][3];
          kq[j][3] = 0ull;
          used[j] += 1;
          if ((used[j] & 3) == 0) fetch4(merge_list_span(a, qi, list_of(j), nl), used[j], kq[j]);  // used up: refill
        }
      }
    }
  }
}
// lists of query qi: the launch's, or fewer where the query's counter says so
__device__ __forceinline__ int merge_nlists(const MergeArgs& a, int64_t qi) {
  int nl = a.nlists;
  if (a.nlists_q) nl = a.nlists_q[qi] < nl ? a.nlists_q[qi] : nl;
  return nl;
}

// --------------------------------------------------------------------------
// merge32: one wave per query; lane l owns lists l, l + 64, ... (<= LPL of them, 64 LPL lists in all).
// Winner o is kept by lane o & 63 and a full wave of results leaves after every 64th round and after the last.
// --------------------------------------------------------------------------
template <int LPL>
__global__ __launch_bounds__(256) void topk_merge32_kernel(MergeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= a.nq) return;
  if (!topk_enter(a.gate, a.out, a.zero_cnt, qi, a.nq, lane == 0)) return;
  uint64_t mine = 0ull;
  merge_rounds<LPL>(
      a, qi, merge_nlists(a, qi), [&](int j) { return lane + 64 * j; },
      [&](int o, uint64_t wm) {
        mine = (lane == (o & 63)) ? wm : mine;
        if ((o & 63) == 63 || o == a.out.k - 1) {
          const int oo = (o & ~63) + lane;
          if (oo <= o) store_result(a.out, qi, oo, mine);
        }
      });
}

// --------------------------------------------------------------------------
// merge32q: merge32 with FOUR waves per query (kout <= 16, 256 LPL lists).  The one-wave merge is a serial chain:
// every one of the k rounds walks all LPL cached list heads of a lane (9 - 13 compare-select steps) before the wave
// maximum - 17 - 26 us per launch for 512 - 768 lists, whatever the number of queries (<= 128 of them keep 16 - 32 CUs
// busy).  Here wave w of the workgroup takes lists w, w + 4, ... (a quarter of the heads per lane), lane o keeps
// winner o, the four 16-entry results meet in LDS as 64 keys, and wave 0 ranks them by counting: rank r < kout stores
// output r.  Keys are all distinct (row indices are unique), so ranks are a permutation; the empty lanes take the
// slots behind them (fewer than kout entries in all lists together).
// --------------------------------------------------------------------------
template <int LPL>
__global__ __launch_bounds__(256) void topk_merge32q_kernel(MergeArgs a) {
  __shared__ uint64_t part[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t qi = blockIdx.x;
  if (!topk_enter(a.gate, a.out, a.zero_cnt, qi, a.nq, threadIdx.x == 0)) return;
  uint64_t mine = 0ull;
  merge_rounds<LPL>(
      a, qi, merge_nlists(a, qi), [&](int j) { return wave + 4 * (lane + 64 * j); },
      [&](int o, uint64_t wm) { mine = (lane == o) ? wm : mine; });
  if (lane < 16) part[wave][lane] = lane < a.out.k ? mine : 0ull;
  __syncthreads();
  if (wave != 0) return;
  const uint64_t key = part[lane >> 4][lane & 15];
  const int rank = wave_rank_u64<64>(key);   // of an empty lane: the number of entries found
  const int slot = key != 0ull ? rank : rank + lanes_below(__ballot(key == 0ull));
  if (slot < a.out.k) store_result(a.out, qi, slot, key);
}

// --------------------------------------------------------------------------
// select: top-k of an UNSORTED candidate buffer (what the candidate-append scans leave: [nq][cap], cnt[nq]) plus an
// optional sorted list per query (the prefix result).  One wave per query, every entry a 64-bit (score, ~row) key
// in a register (lane l owns candidates l, l + 64, ...; its last slot takes entry l of the sorted list).
//   1. the k-th largest SCORE by a bitwise search (32 steps of "how many scores are >= t": one compare-and-count
//      per slot and a wave sum) - no key ever moves;
//   2. ties at that score (rare) are cut by the same search on the row half of the key: exactly k keys selected;
//   3. the selected keys are compacted to one per lane through LDS (ballot / mbcnt positions) and ranked by
//      counting, lane i comparing with every other lane's key (64 readlane steps); lane i stores at its rank.
// (k rounds of wave maximum over all slots - the first version - cost 14.6 us at 15 slots and 72-78 us at 47.)
// --------------------------------------------------------------------------
// The k largest of the wave's keys kq[LPL] (0 = empty slot), one per lane (unsorted) plus its rank among them:
// steps 1-3 above.  `compact` is the wave's 64-entry LDS scratch.  Returns the number of keys found
// (min(k, live keys)); lanes >= that hold key 0.
template <int LPL>
__device__ __forceinline__ int select_keys(const uint64_t (&kq)[LPL], int kwant, int lane, uint64_t* compact,
                                           uint64_t& mine, int& rank) {
  int live = 0;
#pragma unroll
  for (int j = 0; j < LPL; ++j) live += kq[j] != 0ull ? 1 : 0;
  live = wave_sum_i32(live);
  const int k = kwant < live ? kwant : live;
  // 1. T = k-th largest score half
  uint32_t T = 0u;
  if (k > 0) {
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t t = T | (1u << bit);
      int c = 0;
#pragma unroll
      for (int j = 0; j < LPL; ++j) c += (uint32_t)(kq[j] >> 32) >= t ? 1 : 0;
      if (wave_sum_i32(c) >= k) T = t;
    }
  }
  // 2. keys above T are in; `need` of the keys AT T are in, largest row half (= smallest row) first
  int cgt = 0, ceq = 0;
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    const uint32_t u = (uint32_t)(kq[j] >> 32);
    cgt += u > T ? 1 : 0;
    ceq += (u == T && kq[j] != 0ull) ? 1 : 0;
  }
  cgt = wave_sum_i32(cgt);
  ceq = wave_sum_i32(ceq);
  const int need = k - cgt;
  uint32_t Lo = 0u;  // smallest accepted row half among the ties
  if (need < ceq) {
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t t = Lo | (1u << bit);
      int c = 0;
#pragma unroll
      for (int j = 0; j < LPL; ++j) c += ((uint32_t)(kq[j] >> 32) == T && (uint32_t)kq[j] >= t && kq[j] != 0ull) ? 1 : 0;
      if (wave_sum_i32(c) >= need) Lo = t;
    }
  }
  // 3. compaction: position = keys selected in earlier slots + selected lanes below this one in this slot
  int base = 0;
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    const uint32_t u = (uint32_t)(kq[j] >> 32);
    const bool sel = k > 0 && kq[j] != 0ull && (u > T || (u == T && (uint32_t)kq[j] >= Lo));
    const uint64_t m = __ballot(sel);
    if (sel) compact[base + lanes_below(m)] = kq[j];
    base += __builtin_popcountll(m);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same wave wrote and reads: LDS is in order, this pins the compiler
  mine = lane < k ? compact[lane] : 0ull;
  rank = wave_rank_u64<8>(mine);
  return k;
}
// what lane `lane` stores after select_keys found `found` keys: key `mine` at its rank, or an empty slot at `lane`
__device__ __forceinline__ void store_selected(const TopkOut& o, int64_t row, int lane, int found, int rank,
                                               uint64_t mine) {
  if (lane < o.k) store_result(o, row, lane < found ? rank : lane, mine);
}

// slots j < LPL - 1 of a lane: candidates first + step * (lane + 64 j); the last slot: entry `lane` of the sorted list
template <int LPL>
__device__ __forceinline__ void select_load(const SelectArgs& a, int64_t qi, int lane, int first, int step,
                                            bool with_pre, uint64_t (&kq)[LPL]) {
  int cnt = a.cand_cnt[qi];
  cnt = cnt < a.cap ? cnt : a.cap;
#pragma unroll
  for (int j = 0; j < LPL - 1; ++j) {
    const int e = first + step * (lane + 64 * j);
    kq[j] = 0ull;
    if (e < cnt) kq[j] = merge_key(a.cand_val[qi * a.cap + e], a.cand_idx[qi * a.cap + e]);
  }
  kq[LPL - 1] = 0ull;
  if (with_pre && a.pre_val && lane < a.kpre)
    kq[LPL - 1] = merge_key(a.pre_val[qi * a.kpre + lane], a.pre_idx[qi * a.kpre + lane]);
}

template <int LPL>
__global__ __launch_bounds__(256) void topk_select_kernel(SelectArgs a) {
  __shared__ uint64_t compact[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
  if (qi >= a.nq) return;
  if (!topk_enter(a.gate, a.out, nullptr, qi, a.nq, false)) return;
  uint64_t kq[LPL];
  select_load<LPL>(a, qi, lane, 0, 1, true, kq);
  uint64_t mine;
  int rank;
  const int k = select_keys<LPL>(kq, a.out.k, lane, compact[wave], mine, rank);
  store_selected(a.out, qi, lane, k, rank, mine);
}

// select with FOUR waves per query (big candidate buffers: 16 < k <= 64): wave w selects the k best of candidates
// w, w + 4, ... (wave 0 also holds the sorted extra list), the four results meet in LDS and wave 0 selects and ranks
// the k best of those <= 4k keys.  LPLQ = slots per lane of a wave = ceil(cap / 256) + 1.
template <int LPLQ>
__global__ __launch_bounds__(256) void topk_select4_kernel(SelectArgs a) {
  __shared__ uint64_t compact[4][64];
  __shared__ uint64_t stage[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t qi = blockIdx.x;
  if (!topk_enter(a.gate, a.out, nullptr, qi, a.nq, false)) return;
  uint64_t kq[LPLQ];
  select_load<LPLQ>(a, qi, lane, wave, 4, wave == 0, kq);
  uint64_t mine;
  int rank;
  select_keys<LPLQ>(kq, a.out.k, lane, compact[wave], mine, rank);
  stage[wave][lane] = mine;   // 0 beyond the wave's count
  __syncthreads();
  if (wave != 0) return;
  uint64_t k2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) k2[j] = stage[j][lane];
  const int k = select_keys<4>(k2, a.out.k, lane, compact[0], mine, rank);
  store_selected(a.out, qi, lane, k, rank, mine);
}

// --------------------------------------------------------------------------
// merge of SORTED partial lists (the prefix lists: nlists x [nq][16]) by selection instead of k rounds of wave
// maximum: (a) the kout lists with the largest HEAD keys are found with select_keys on the heads (one slot per
// list); an entry of any other list is below its own head, hence below kout entries of those lists, and cannot be
// in the top kout: (b) only those kout x 16 <= 256 entries are loaded (4 slots per lane) and (c) selected and ranked.
// Exact under the (score desc, row asc) order (keys are unique).  ~8 us where the rounds took 17-19 us.
// The only merge with groups (MergeArgs::ngroups, blockIdx.y): 64 HLPL lists per group; kin == 16, kout <= 16.
// --------------------------------------------------------------------------
template <int HLPL>
__global__ __launch_bounds__(256) void topk_merge_sel_kernel(MergeArgs a) {
  __shared__ uint64_t compact[4][64];
  __shared__ int sel_list[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
  if (qi >= a.nq) return;
  const int ng_ = a.ngroups > 1 ? a.ngroups : 1, grp = (int)blockIdx.y;
  if (!topk_enter(a.gate, a.out, a.zero_cnt, qi, a.nq, lane == 0 && grp == 0)) return;
  const int nl = (a.nlists - grp + ng_ - 1) / ng_;   // lists of this group
  const int64_t gout = (int64_t)grp * a.nq;          // output row offset of the group
  // (a) heads: slot j of lane l = list l + 64 j of this group, as TRUE keys (a tie between heads must resolve by
  //     row index exactly as in the final order); the kout-th largest head key is then the admission bar
  uint64_t hk[HLPL];
#pragma unroll
  for (int j = 0; j < HLPL; ++j) {
    const int list = lane + 64 * j;
    hk[j] = 0ull;
    if (list < nl) {
      const ListSpan s = merge_list_span(a, qi, list, nl, ng_, grp);
      hk[j] = merge_key(s.val[0], s.idx[0]);
    }
  }
  uint64_t mine;
  int rank;
  const int nsel = select_keys<HLPL>(hk, a.out.k, lane, compact[wave], mine, rank);
  if (lane < nsel && rank == nsel - 1) compact[wave][0] = mine;   // the bar (keys are unique: one lane writes)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const uint64_t bar = nsel > 0 ? compact[wave][0] : ~0ull;
  int nlist = 0;
#pragma unroll
  for (int j = 0; j < HLPL; ++j) {
    const bool sel = hk[j] != 0ull && hk[j] >= bar;
    const uint64_t m = __ballot(sel);
    if (sel) sel_list[wave][nlist + lanes_below(m)] = lane + 64 * j;
    nlist += __builtin_popcountll(m);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // (b) the entries of the selected lists: entry e = lane + 64 j -> list e / 16, position e % 16
  uint64_t kq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane + 64 * j;
    kq[j] = 0ull;
    if ((e >> 4) < nlist) {
      const ListSpan s = merge_list_span(a, qi, sel_list[wave][e >> 4], nl, ng_, grp);
      kq[j] = merge_key(s.val[e & 15], s.idx[e & 15]);
    }
  }
  // (c)
  const int k = select_keys<4>(kq, a.out.k, lane, compact[wave], mine, rank);
  store_selected(a.out, gout + qi, lane, k, rank, mine);
}

// --------------------------------------------------------------------------
// The merge behind hcir_topk_merge (per-shard results of a sharded gallery): 64-bit indices, (value, index) pairs
// under `better` instead of keys.  One wave per query; lists [nlists][nq][kin] sorted (desc, idx asc), empty slots
// have idx < 0.  Lane l owns lists l, l + 64, ... (<= kMergeLPL of them) and caches each list's head; kout rounds of
// wave arg-max, the winner's next entry re-read from memory.
// --------------------------------------------------------------------------
struct Merge64Args {
  const float* vals;
  const int64_t* idx;
  float* out_val;
  int64_t* out_idx;
  int64_t nq;
  int nlists, kin, kout;
};

__global__ __launch_bounds__(256) void topk_merge_kernel(Merge64Args a) {
  constexpr int LPL = kMergeLPL;
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= a.nq) return;

  float cv[LPL];
  int64_t ci[LPL];
  int hd[LPL];
  auto fetch = [&](int list, int pos, float& v, int64_t& id) {
    v = kNegInf;
    id = -1;
    if (list < a.nlists && pos < a.kin) {
      const int64_t o = ((int64_t)list * a.nq + qi) * a.kin + pos;
      v = a.vals[o];
      id = a.idx[o];
    }
    if (id < 0) v = kNegInf;
  };
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    hd[j] = 0;
    fetch(lane + 64 * j, 0, cv[j], ci[j]);
  }
  float keep_v = kNegInf;
  int64_t keep_i = -1;
  for (int o = 0; o < a.kout; ++o) {
    float bv = cv[0];
    int64_t bi = ci[0];
    int bj = 0;
#pragma unroll
    for (int j = 1; j < LPL; ++j) {
      const bool take = (ci[j] >= 0) && (bi < 0 || better(cv[j], ci[j], bv, bi));
      bv = take ? cv[j] : bv;
      bi = take ? ci[j] : bi;
      bj = take ? j : bj;
    }
    // wave arg-max under (score desc, idx asc); empty = idx < 0
    float wv = bv;
    int64_t wi = bi;
    int wl = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(wv, off);
      const int64_t oi = __shfl_xor(wi, off);
      const int ol = __shfl_xor(wl, off);
      const bool take = (oi >= 0) && (wi < 0 || better(ov, oi, wv, wi));
      wv = take ? ov : wv;
      wi = take ? oi : wi;
      wl = take ? ol : wl;
    }
    // winner o kept by lane o & 63, stored once per 64 rounds (see merge_rounds: no store inside the loop)
    if (lane == (o & 63)) {
      keep_v = wv;
      keep_i = wi;
    }
    if ((o & 63) == 63 || o == a.kout - 1) {
      const int oo = (o & ~63) + lane;
      if (oo <= o) {
        a.out_val[qi * a.kout + oo] = keep_i < 0 ? kNegInf : keep_v;
        a.out_idx[qi * a.kout + oo] = keep_i < 0 ? -1 : keep_i;
      }
    }
    if (lane == wl && wi >= 0) {
#pragma unroll
      for (int j = 0; j < LPL; ++j) {
        if (j == bj) {
          hd[j] += 1;
          fetch(lane + 64 * j, hd[j], cv[j], ci[j]);
        }
      }
    }
  }
}

}  // namespace
