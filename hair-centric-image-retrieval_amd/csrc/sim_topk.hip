// sim_topk.hip — brute-force query x gallery cosine / inner-product top-k.
//
// Replaces sklearn KNeighborsClassifier(metric="cosine").kneighbors
// (HP/src/classification_engine.py:80-82), cosine_similarity + argsort
// (src/models/hair_encoder.py:193-194) and torch.mm + torch.sort
// (HP/src/neg_sampling.py:37,45-51).  See include/hcir.h for the contract.
//
// Structure (DESIGN.md "sim_topk"):
//   scan   : every workgroup streams gallery tiles (sim_core.h) against one block
//            of <=128 queries; each lane owns one query column and keeps a sorted
//            top-KP list in registers; lists of a workgroup are merged through LDS
//            and written as one partial list per (workgroup, query).
//   merge  : one or four waves per query merge the partial lists (k rounds of wave
//            arg-max over per-lane cached list heads): topk_merge.h.
//   prefix : for big galleries the first S rows are scanned and merged first; the
//            k-th score of that prefix is a per-query floor for the main scan, so
//            that register-list insertions become rare there (a gallery row with
//            score <= floor can never enter the final top-k: every prefix row has
//            a smaller index and wins the tie).
//   k > 64 : repeated passes, each taking the next <=64 ranks below a per-query
//            ceiling (val, idx) left by the previous pass.
//   > 128 queries (k <= 16, fp16/bf16): the rows behind the prefix go through
//            sim_scan_big_kernel - the GEMM's 256 x 256 tile, no lists: the rare rows above
//            the floor are appended to per-query candidate buffers; a device flag gates the
//            list-keeping scan as fallback if a buffer overflows.
#include "sim_core.h"
#include "sim_plan.h"
#include "topk_merge.h"
#include <math.h>
#include <stdlib.h>
#include <type_traits>

constexpr int kScanAux = 2;  // cache policy of the once-read gallery stream: 2 = nt (non-temporal), +5 % GB/s

#ifdef HCIR_DIAG_STAMPS
// diagnostic build only (tools/build_variant.sh stamps "-DHCIR_DIAG_STAMPS"): wall-clock stamps (100 MHz) of the
// floorless (prefix) launches, 8 per workgroup, read back through hcir_debug_stamps
__device__ unsigned long long g_stamps[1024 * 8];
#define HCIR_STAMP(i)                                                                              \
  do {                                                                                             \
    if (!a.floor_val && threadIdx.x == 0 && blockIdx.x < 512)                                      \
      g_stamps[(blockIdx.y * 512 + blockIdx.x) * 8 + (i)] = __builtin_amdgcn_s_memrealtime();     \
  } while (0)
#else
#define HCIR_STAMP(i) \
  do {                \
  } while (0)
#endif

namespace {

// Sorted (score desc, arrival order) register list.  Callers feed increasing row
// indices, so equal scores keep the smaller index first.  Precondition: s > v[KP-1].
template <int KP>
__device__ __forceinline__ void topk_insert(float (&v)[KP], int (&id)[KP], float s, int i) {
#pragma unroll
  for (int j = KP - 1; j > 0; --j) {
    const bool up = s > v[j - 1];
    const bool here = s > v[j];
    v[j] = up ? v[j - 1] : (here ? s : v[j]);
    id[j] = up ? id[j - 1] : (here ? i : id[j]);
  }
  const bool top = s > v[0];
  v[0] = top ? s : v[0];
  id[0] = top ? i : id[0];
}
template <int KP>
__device__ __forceinline__ float topk_kth(const float (&v)[KP], int k) {
  // select chain kept opaque: hipcc otherwise rewrites it as v[k-1] through scratch
  float t = v[KP - 1];
#pragma unroll
  for (int j = 0; j < KP - 1; ++j) {
    t = (j == k - 1) ? v[j] : t;
    asm volatile("" : "+v"(t));
  }
  return t;
}

// Batch insertion (scan epilogue): when many of a lane's 16 scores of one 32 x 32 MFMA tile are candidates - every
// one of them while the lists fill from a workgroup's first tile - the slot-by-slot insertion costs ~115 VALU
// instructions per slot for the whole wave.  The batch path sorts the 16 keys with a bitonic network (80
// compare-exchanges), takes max(list[j], batch[KP-1-j]) - the KP best of the union, as a bitonic sequence - and
// finishes with one bitonic merge: ~130 (KP = 16) compare-exchanges of 5 instructions, whatever the number of
// candidates.  Keys are merge_key's (score, row) words: all distinct, so the network needs no stability.
__device__ __forceinline__ void key_ce_desc(uint64_t& a, uint64_t& b) {  // a <- better, b <- worse
  const bool sw = b > a;
  const uint64_t t = sw ? b : a;
  b = sw ? a : b;
  a = t;
}
template <int N>
__device__ __forceinline__ void key_bitonic_merge_desc(uint64_t (&x)[N]) {  // bitonic -> sorted, best first
#pragma unroll
  for (int st = N / 2; st >= 1; st >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i)
      if ((i & st) == 0) key_ce_desc(x[i], x[i + st]);
}
__device__ __forceinline__ void key_bitonic_sort16_desc(uint64_t (&x)[16]) {
#pragma unroll
  for (int k = 2; k <= 16; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int l = i ^ j;
        if (l > i) {
          if ((i & k) == 0)
            key_ce_desc(x[i], x[l]);
          else
            key_ce_desc(x[l], x[i]);
        }
      }
}
constexpr int kBatchMin = 8;  // candidates slots (wave union) from which the batch path is taken

struct ScanArgs {
  const void* q;
  const void* g;
  const float* qn;         // [nq] or null
  const float* gn;         // [ng] or null
  const float* floor_val;  // [nq] or null: only scores > floor are candidates
  const float* ceil_val;   // [nq] or null: only (score, idx) strictly after
  const int* ceil_idx;     //   (ceil_val, ceil_idx) in (desc, asc) order are candidates
  float* part_val;         // [nparts][nq][KP]
  int* part_idx;
  int64_t nq, row_begin, row_end;  // gallery rows [row_begin, row_end)
  int d, k;
  int shared_stream;  // > 1 query block reads every gallery tile: keep the stream in L2 (no `nt`)
  const int* gate;    // optional device flag: the launch does nothing unless *gate != 0 (fallback of the big scan)
  // candidate-append mode (template CAND): no lists; every score above the floor goes to the query's buffer
  float* cand_val;    // [cap][nq]
  int* cand_idx;      // [cap][nq]
  int* cand_cnt;      // [nq]
  int* overflow;      // [1]
  int cap;
  int cand_query_major;  // 1: buffers are [nq][cap] (what the select kernels read, coalesced); 0: [cap][nq]
  int floor_groups;   // floor = min over this many [nq] arrays behind floor_val (group floors of the prefix)
  int floor_inclusive;  // 1: candidates are scores >= floor (the scan covers the rows the floor came from)
};

// BATCH: the launch fills its lists from nothing (no floor: prefix scans, single scans of small galleries, the
// k > 64 passes) - the epilogue gets the batch-insertion path.  A separate instantiation, and only of the
// one-query-tile geometry: the path's ~100 extra live registers spill in the two-query-tile kernels at two
// workgroups per CU (measured: the 64-query main scan 260 -> 780 us) and at one workgroup per CU they lose what the
// batch gains (64-query call 333 -> 340 us); running a 64-query prefix as two 32-query blocks of this kernel was a
// wash (prefix 52 -> 49 us).  The streaming launches behind a floor keep the lean kernel.
// (KP = 16, one query tile x two wave columns, two row groups: 24 KB stages -> THREE workgroups per CU; the 64-query
// geometry of the streaming launches, see kSimGeom in sim_plan.h)
template <typename T, int KP, int QT, int WQ, int WGG, bool GLDS, bool CAND = false, bool BATCH = false>
__global__ __launch_bounds__(256, ((KP == 16 && QT == 1 && WQ == 2 && WGG == 2 && GLDS && !BATCH)
                                       ? 3
                                       : ((KP <= 32 && GLDS) ? 2 : 1))) void sim_topk_scan(ScanArgs a) {
  using Cfg = SimCfg<T, WGG, WQ, QT>;
  constexpr int EPS = SimElem<T>::kPerStage;
  constexpr int NSRC = 2 * WGG;  // lists per query inside a workgroup
  // queries merged per LDS round (power of two, the lists must fit the staging LDS)
  constexpr int QR_FIT = Cfg::LDS_BYTES / (NSRC * KP * 8);
  constexpr int QR = QR_FIT >= Cfg::QB ? Cfg::QB : (QR_FIT >= 64 ? 64 : (QR_FIT >= 32 ? 32 : 16));
  static_assert(QR * NSRC * KP * 8 <= Cfg::LDS_BYTES, "merge round must fit LDS");
  // LDS-DMA stage ring.  KP = 64 runs one workgroup per CU (128 list registers per lane): a 4-slot ring keeps
  // three stages (108 KB) in flight per CU instead of one; the 2-workgroup configurations keep two slots each.
  // (A 4-slot ring for the one-tile-per-workgroup prefix launches of the other configurations was measured:
  // no gain - their ~80 us is not the stage-latency chain.)
  constexpr int NST = (GLDS && KP == 64) ? 4 : 2;
  static_assert(NST * Cfg::STAGE_BYTES <= 160 * 1024, "stage ring must fit the CU's LDS");
  __shared__ __attribute__((aligned(16))) char lds[NST * Cfg::STAGE_BYTES];

  if (a.gate && *a.gate == 0) return;  // uniform: every wave of the grid reads the same flag
  HCIR_STAMP(0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_g = wave / WQ, wave_q = wave % WQ;
  const int r = lane & 31, h = lane >> 5;
  const T* __restrict__ g = static_cast<const T*>(a.g);
  const T* __restrict__ q = static_cast<const T*>(a.q);
  const int64_t q_row0 = (int64_t)blockIdx.y * Cfg::QB;
  const int64_t q_last = a.nq - 1;

  // per-lane query state (CAND keeps no lists: one dummy entry)
  constexpr int KL = CAND ? 1 : KP;
  float lv[QT][KL];
  int li[QT][KL];
  float thr[QT], qnv[QT], cval[QT];
  int cidx[QT];
  int64_t myq[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int j = 0; j < KL; ++j) {
      lv[qt][j] = kNegInf;
      li[qt][j] = -1;
    }
    myq[qt] = q_row0 + wave_q * (32 * QT) + qt * 32 + r;
    const bool live = myq[qt] < a.nq;
    const int64_t qc = live ? myq[qt] : q_last;
    qnv[qt] = a.qn ? a.qn[qc] : 1.0f;
    thr[qt] = a.floor_val ? a.floor_val[qc] : kNegInf;
    if constexpr (CAND) {
      // group floors of the prefix: every group holds >= k/groups rows at or above its floor, so the minimum
      // is a valid floor for k; padding queries never match
      for (int gidx = 1; gidx < a.floor_groups; ++gidx) thr[qt] = fminf(thr[qt], a.floor_val[gidx * a.nq + qc]);
      if (!live) thr[qt] = __builtin_huge_valf();
    }
    cval[qt] = a.ceil_val ? a.ceil_val[qc] : __builtin_huge_valf();
    cidx[qt] = a.ceil_val ? a.ceil_idx[qc] : -1;
  }
  float floorv[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) floorv[qt] = thr[qt];

  const int nkc = (a.d + EPS - 1) / EPS;
  const int64_t nrows = a.row_end - a.row_begin;
  const int64_t ntiles = (nrows + Cfg::GM - 1) / Cfg::GM;
  const int64_t my_tiles = blockIdx.x < ntiles ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  const int64_t nsteps = my_tiles * nkc;
  const int64_t g_last = a.row_end - 1;

  f32x16 acc[2][QT];
#pragma unroll
  for (int gt = 0; gt < 2; ++gt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[gt][qt][i] = 0.f;

  // Staging.  GLDS (d a multiple of the 128-B stage): LDS-DMA straight into the double buffer,
  // stage step+1 issued right after the barrier that retires stage step.  Otherwise register
  // staging one stage ahead with zero fill past d.
  u32x4 regs[GLDS ? 1 : Cfg::NLOAD];
  auto tile_row0 = [&](int64_t ti) { return a.row_begin + ((int64_t)blockIdx.x + ti * gridDim.x) * Cfg::GM; };
  // DMA sources as 32-bit per-lane byte offsets from a wave-uniform base (tile's first gallery row / block's first
  // query row, + 128 B per k chunk): computed ONCE - they are the same for every full tile - so a stage issues
  // NLOAD loads and nothing else.  (Re-deriving row, clamp and a 64-bit product per piece and stage cost ~300
  // VALU instructions per stage: with one stage in flight per workgroup that was on the critical path of both the
  // one-tile prefix workgroups and the streaming main scan.)  Only the gallery's last tile can be partial: its
  // rows are clamped to the last row when the issue cursor reaches it (it is the last tile of its workgroup).
  constexpr int NPG = Cfg::GM / 32, NPQ = Cfg::QB / 32;  // pieces of a stage: gallery rows, then query rows
  static_assert(NPG + NPQ == Cfg::NLOAD, "pieces");
  constexpr int EPC_ = SimElem<T>::kPerChunk;
  uint32_t goff[NPG], qoff[NPQ];
  auto set_goff = [&](int64_t rows_valid) {  // rows_valid >= GM: full tile
#pragma unroll
    for (int i = 0; i < NPG; ++i) {
      const int slot = tid + Cfg::NT * i;
      int row = slot >> 3;
      const int chunk = (slot & 7) ^ ((row >> 1) & 7);
      row = row < rows_valid ? row : (int)rows_valid - 1;
      goff[i] = (uint32_t)(((int64_t)row * a.d + chunk * EPC_) * (int64_t)sizeof(T));
    }
  };
  if constexpr (GLDS) {
    set_goff(Cfg::GM);
#pragma unroll
    for (int i = 0; i < NPQ; ++i) {
      const int slot = tid + Cfg::NT * (NPG + i);
      const int row = (slot >> 3) - Cfg::GM;
      const int chunk = (slot & 7) ^ (((slot >> 3) >> 1) & 7);
      int64_t qr = q_row0 + row;
      qr = qr > q_last ? q_last : qr;
      qoff[i] = (uint32_t)(((qr - q_row0) * a.d + chunk * EPC_) * (int64_t)sizeof(T));
    }
  }
  // stage s of this workgroup = (tile s / nkc, chunk s % nkc); the issue cursor runs NST-1 stages ahead
  int64_t issue_tile = 0;
  int issue_kc = 0;
  auto issue_stage = [&](int slot) {
    const int64_t r0 = tile_row0(issue_tile);
    if (issue_kc == 0 && r0 + Cfg::GM > a.row_end) set_goff(a.row_end - r0);
    const char* gb = reinterpret_cast<const char*>(g) + (r0 * a.d) * (int64_t)sizeof(T) + issue_kc * 128;
    const char* qb = reinterpret_cast<const char*>(q) + (q_row0 * a.d) * (int64_t)sizeof(T) + issue_kc * 128;
    char* dst = lds + slot * Cfg::STAGE_BYTES + (tid & ~63) * 16;
#pragma unroll
    for (int i = 0; i < NPG; ++i) {
      if (a.shared_stream || kScanAux == 0)
        lds_dma16_v(gb + goff[i], lds_addr(dst) + Cfg::NT * i * 16);
      else
        lds_dma16_v_nt(gb + goff[i], lds_addr(dst) + Cfg::NT * i * 16);
    }
#pragma unroll
    for (int i = 0; i < NPQ; ++i) lds_dma16_v(qb + qoff[i], lds_addr(dst) + Cfg::NT * (NPG + i) * 16);
    if (++issue_kc == nkc) {
      issue_kc = 0;
      ++issue_tile;
    }
  };
  if (nsteps > 0) {
    if constexpr (GLDS) {
#pragma unroll
      for (int s0 = 0; s0 < NST - 1; ++s0)
        if (s0 < nsteps) issue_stage(s0);
    } else {
      sim_stage_load<T, Cfg>(regs, g, tile_row0(0), g_last, q, q_row0, q_last, a.d, 0, tid);
      sim_stage_store<Cfg>(regs, lds, tid);
    }
  }
  if constexpr (!GLDS) __syncthreads();
  HCIR_STAMP(1);

  int64_t tile_i = 0;  // index among my tiles
  int kc = 0;
  int cur = 0;         // ring slot of stage `step`
  for (int64_t step = 0; step < nsteps; ++step) {
    // next stage (possibly first chunk of my next tile)
    int nkc_next = kc + 1;
    int64_t ntile_i = tile_i;
    if (nkc_next == nkc) {
      nkc_next = 0;
      ntile_i = tile_i + 1;
    }
    const bool has_next = step + 1 < nsteps;
    if constexpr (GLDS) {
      // Stage `step` landed for every wave: the NST-2 younger stages may stay in flight (vmcnt retires in
      // order; the only other vector-memory operations of the loop are the optional gallery-norm loads of the
      // tile epilogue, whose consumers already waited for everything older).  Near the tail fewer stages
      // are outstanding than the count allows: wait for all.
      if (NST > 2 && !a.gn && step + NST - 1 <= nsteps) {
        if constexpr (NST == 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * Cfg::NLOAD) : "memory");
        __syncthreads();
      } else {
        sim_glds_retire_and_sync();
      }
      // the slot read in step-1 is free after this barrier: issue stage step+NST-1 into it
      if (step == 0) HCIR_STAMP(2);
      if (step + NST - 1 < nsteps) issue_stage((cur + NST - 1) % NST);
      sim_stage_mfma<T, Cfg, QT>(acc, lds + cur * Cfg::STAGE_BYTES, wave_g, wave_q, lane);
      if (step == nsteps - 1) HCIR_STAMP(3);
    } else {
      if (has_next)
        sim_stage_load<T, Cfg>(regs, g, tile_row0(ntile_i), g_last, q, q_row0, q_last, a.d, nkc_next, tid);
      sim_stage_mfma<T, Cfg, QT>(acc, lds + cur * Cfg::STAGE_BYTES, wave_g, wave_q, lane);
      if (has_next) sim_stage_store<Cfg>(regs, lds + (cur ^ 1) * Cfg::STAGE_BYTES, tid);
    }

    if (kc == nkc - 1) {
      // ---- per-tile epilogue: scale the 16 scores of each 32x32 tile, mask the ones
      //      above the lane's threshold, then pop candidates in row order into the list
      const int64_t row0 = tile_row0(tile_i);
#pragma unroll
      for (int gt = 0; gt < 2; ++gt) {
        const int64_t rbase = row0 + wave_g * 64 + gt * 32 + 4 * h;
        float gnv[16];
        if (a.gn) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int64_t row = rbase + (i & 3) + 8 * (i >> 2);
            gnv[i] = a.gn[row < a.row_end ? row : g_last];
          }
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          unsigned mask = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int64_t row = rbase + (i & 3) + 8 * (i >> 2);
            float s = acc[gt][qt][i];
            if (a.gn) s = s * gnv[i];
            if (a.qn) s = s * qnv[qt];
            acc[gt][qt][i] = s;
            bool cand = (row < a.row_end) && (s > thr[qt]);
            if constexpr (CAND) cand = cand || ((row < a.row_end) && a.floor_inclusive && s == thr[qt]);
            if (a.ceil_val)
              cand = cand && ((s < cval[qt]) || (s == cval[qt] && (int)row > cidx[qt]));
            mask |= cand ? (1u << i) : 0u;
          }
          // common case behind the prefix floor: no lane has a candidate -> one ballot, no work.
          // Otherwise a wave-uniform slot loop: acc[..][i] with a scalar i stays in registers
          // (movrel), a per-lane index would be lowered through scratch.
          unsigned any = 0u;
          if (__ballot(mask != 0u) != 0ull) {
            any = mask;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) any |= __shfl_xor(any, off);
            any = __builtin_amdgcn_readfirstlane(any);
          }
          if constexpr (!CAND && BATCH) {
            if (__builtin_popcount(any) >= kBatchMin) {  // wave-uniform
              uint64_t bk[16];
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const bool c = ((mask >> i) & 1u) && acc[gt][qt][i] > thr[qt];
                bk[i] = c ? merge_key(acc[gt][qt][i], (int)(rbase + (i & 3) + 8 * (i >> 2))) : 0ull;
              }
              key_bitonic_sort16_desc(bk);
              uint64_t lk[KP];
#pragma unroll
              for (int j = 0; j < KP; ++j) lk[j] = merge_key(lv[qt][j], li[qt][j]);
#pragma unroll
              for (int j = 0; j < 16; ++j) {
                const uint64_t o = bk[15 - j];
                lk[KP - 16 + j] = o > lk[KP - 16 + j] ? o : lk[KP - 16 + j];
              }
              key_bitonic_merge_desc<KP>(lk);
#pragma unroll
              for (int j = 0; j < KP; ++j) {
                lv[qt][j] = lk[j] ? merge_key_val(lk[j]) : kNegInf;
                li[qt][j] = lk[j] ? merge_key_idx(lk[j]) : -1;
              }
              thr[qt] = fmaxf(floorv[qt], topk_kth<KP>(lv[qt], a.k));
              any = 0u;
            }
          }
          while (any != 0u) {
            const int i = __builtin_ctz(any);
            any &= any - 1u;
            const float s = acc[gt][qt][i];
            if constexpr (CAND) {
              if ((mask >> i) & 1u) {  // rare behind the floor: one global atomic per candidate
                const int pos = atomicAdd(a.cand_cnt + myq[qt], 1);
                if (pos < a.cap) {
                  const int64_t at = a.cand_query_major ? myq[qt] * a.cap + pos : (int64_t)pos * a.nq + myq[qt];
                  a.cand_val[at] = s;
                  a.cand_idx[at] = (int)(rbase + (i & 3) + 8 * (i >> 2));
                } else {
                  *a.overflow = 1;
                }
              }
            } else {
              if (((mask >> i) & 1u) && s > thr[qt]) {
                topk_insert<KP>(lv[qt], li[qt], s, (int)(rbase + (i & 3) + 8 * (i >> 2)));
                thr[qt] = fmaxf(floorv[qt], topk_kth<KP>(lv[qt], a.k));
              }
            }
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[gt][qt][i] = 0.f;
        }
      }
    }
    if constexpr (!GLDS) __syncthreads();
    kc = nkc_next;
    tile_i = ntile_i;
    cur = (cur + 1 == NST) ? 0 : cur + 1;
  }
  HCIR_STAMP(4);
  if constexpr (!CAND) {  // (CAND: nothing to merge, the candidates are already in the per-query buffers)
  __syncthreads();  // every wave is done with the stage buffers before they are re-used below

  // ---- merge the NSRC lists of each query through LDS, one thread per query,
  //      QR queries per round
  float* mv = reinterpret_cast<float*>(lds);
  int* mi = reinterpret_cast<int*>(lds + QR * NSRC * KP * 4);
  for (int q0r = 0; q0r < Cfg::QB; q0r += QR) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const int ql = wave_q * (32 * QT) + qt * 32 + r - q0r;
      const int src = wave_g * 2 + h;
      if (ql >= 0 && ql < QR) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          mv[(ql * NSRC + src) * KP + j] = lv[qt][j];
          mi[(ql * NSRC + src) * KP + j] = li[qt][j];
        }
      }
    }
    __syncthreads();
    if (tid < QR && q_row0 + q0r + tid < a.nq) {
      const float* lv = mv + tid * NSRC * KP;
      const int* li = mi + tid * NSRC * KP;
      // list heads live in registers as 64-bit keys; only the winner's next entry is re-read from LDS
      // (re-reading all NSRC heads per output through dependent LDS loads took 21 us per workgroup)
      uint64_t hk[NSRC];
      int hp[NSRC];
#pragma unroll
      for (int s = 0; s < NSRC; ++s) {
        hp[s] = 0;
        hk[s] = merge_key(lv[s * KP], li[s * KP]);
      }
      // the merged list is collected in registers and stored once, as 16-B pieces: with a store inside the
      // loop hipcc put `s_waitcnt vmcnt(0)` into every iteration (16 store round trips = 21 us per workgroup)
      float* ov = a.part_val + ((int64_t)blockIdx.x * a.nq + q_row0 + q0r + tid) * KP;
      int* oi = a.part_idx + ((int64_t)blockIdx.x * a.nq + q_row0 + q0r + tid) * KP;
      for (int o0 = 0; o0 < KP; o0 += 16) {  // 16 outputs at a time in registers
        float ovr[16];
        int oir[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) {
          uint64_t best = hk[0];
          int bs = 0;
#pragma unroll
          for (int s = 1; s < NSRC; ++s) {
            const bool take = hk[s] > best;
            best = take ? hk[s] : best;
            bs = take ? s : bs;
          }
          ovr[o] = best ? merge_key_val(best) : kNegInf;
          oir[o] = best ? merge_key_idx(best) : -1;
          // advance the winner's list: ONE LDS read pair at a per-lane address, then select-chain updates
          // (a branch per source serialised eight LDS round trips per output across the divergent lanes)
          int np = 0;
#pragma unroll
          for (int s = 0; s < NSRC; ++s) np = (s == bs) ? hp[s] + 1 : np;
          const bool more = best != 0ull && np < KP;
          const int at = bs * KP + (more ? np : 0);
          const uint64_t nk = more ? merge_key(lv[at], li[at]) : 0ull;
#pragma unroll
          for (int s = 0; s < NSRC; ++s) {
            const bool upd = best != 0ull && s == bs;
            hp[s] = upd ? np : hp[s];
            hk[s] = upd ? nk : hk[s];
          }
        }
#pragma unroll
        for (int o = 0; o < 16; o += 4) {
          *reinterpret_cast<f32x4*>(ov + o0 + o) = (f32x4){ovr[o], ovr[o + 1], ovr[o + 2], ovr[o + 3]};
          *reinterpret_cast<u32x4*>(oi + o0 + o) =
              (u32x4){(uint32_t)oir[o], (uint32_t)oir[o + 1], (uint32_t)oir[o + 2], (uint32_t)oir[o + 3]};
        }
      }
    }
    __syncthreads();
  }
  }  // !CAND
  HCIR_STAMP(5);
}

// --------------------------------------------------------------------------
// Big-tile scan of the rows behind the prefix, for MANY queries (nq > 128, k <= 16, fp16 / bf16, d % 64 == 0).
//
// With >128 queries the scan is MFMA-bound and the 128 x 128 tile of sim_topk_scan (64 x 64 per wave) tops
// out near 0.45-0.55 PFLOP/s; the 256 x 256 tile of the ViT GEMM (gemm.hip: 8 waves, 128 x 64 per wave, two
// 64 KB LDS slots filled by LDS-DMA) runs the same product at about twice that.  Its 128 accumulators leave no
// room for per-lane top-k lists, and it does not need them: behind the prefix floor a candidate is RARE
// (a row enters only if it beats the k-th score of the first rows: ~15 k rows per query in a gallery in
// random order), so the kernel keeps no lists at all - a lane that sees score > floor appends (score, row) to
// the query's candidate buffer through an atomic counter.  The final merge takes the prefix list plus the
// <= cap candidates as one-element lists.  If any query overflows its buffer (a gallery whose later rows
// systematically beat its first ones) a device flag is raised and the list-keeping scan runs instead, gated
// on that flag: exact either way, no host round trip.
//
// MFMA operands, k-order and accumulation are those of sim_topk_scan (32x32x16, gallery row on the MFMA row,
// query on the column, chunks 2ks+h of a 64-wide stage): the scores are bit-identical to that kernel's.
// --------------------------------------------------------------------------
struct BigScanArgs {
  const void* q;
  const void* g;
  const float* floor_val;  // [nq] k-th score of the prefix
  float* cand_val;         // [cap][nq]
  int* cand_idx;           // [cap][nq]
  int* cand_cnt;           // [nq], zeroed by the caller
  int* overflow;           // [1],  zeroed by the caller
  int64_t nq, row_begin, row_end;
  int d, cap;
};

template <typename T>
__global__ __launch_bounds__(512, 2) void sim_scan_big_kernel(BigScanArgs a) {
  constexpr int STAGE = 512 * 128;  // 256 gallery rows then 256 query rows, 128 B (64 elements) each
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_g = wave >> 2, wave_q = wave & 3;
  const int r = lane & 31, h = lane >> 5;
  const int64_t q_row0 = (int64_t)blockIdx.y * 256;
  const int nkc = a.d / 64;
  const int64_t nrows = a.row_end - a.row_begin;
  const int64_t ntiles = (nrows + 255) / 256;
  const int64_t my_tiles =
      (int64_t)blockIdx.x < ntiles ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  const int64_t nsteps = my_tiles * nkc;
  auto tile_row0 = [&](int64_t ti) { return a.row_begin + ((int64_t)blockIdx.x + ti * gridDim.x) * 256; };

  float flo[2];
  int64_t myq[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    myq[qt] = q_row0 + wave_q * 64 + qt * 32 + r;
    flo[qt] = myq[qt] < a.nq ? a.floor_val[myq[qt]] : __builtin_huge_valf();  // padding queries never match
  }

  // DMA sources: piece = tid + 512 i -> LDS row piece>>3, physical 16-B slot piece&7 holding logical chunk
  // slot ^ ((row>>1)&7).  Pieces 0..3 are gallery rows (offsets from the tile's first row, clamped to the last
  // gallery row), 4..7 query rows (the same for every tile, clamped to the last query).
  const char* qbase = static_cast<const char*>(a.q) + q_row0 * a.d * (int64_t)sizeof(T);
  const char* gbase = nullptr;
  uint32_t goff[4], qoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = tid + 512 * (4 + i);
    const int row = (piece >> 3) - 256, chunk = (piece & 7) ^ ((((piece >> 3)) >> 1) & 7);
    int64_t qr = row;
    qr = q_row0 + qr > a.nq - 1 ? a.nq - 1 - q_row0 : qr;
    qoff[i] = (uint32_t)((qr * a.d + chunk * 8) * (int64_t)sizeof(T));
  }
  int64_t issue_tile = 0;
  int issue_kc = 0;
  auto set_gallery_sources = [&](int64_t ti) {
    const int64_t r0 = tile_row0(ti);
    gbase = static_cast<const char*>(a.g) + r0 * a.d * (int64_t)sizeof(T);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int piece = tid + 512 * i;
      const int row = piece >> 3, chunk = (piece & 7) ^ ((row >> 1) & 7);
      int64_t gr = row;
      gr = r0 + gr > a.row_end - 1 ? a.row_end - 1 - r0 : gr;
      goff[i] = (uint32_t)((gr * a.d + chunk * 8) * (int64_t)sizeof(T));
    }
  };
  auto issue_piece = [&](int slot, int i) {  // i is a constant after unrolling
    // the transfer outside the compiler's view (common.h lds_dma16): big scan +3.8 %, streaming scans +0.7..1.4 %
    // against __builtin_amdgcn_global_load_lds
    lds_dma16((i < 4 ? gbase : qbase) + issue_kc * 128, i < 4 ? goff[i & 3] : qoff[i & 3],
              lds_addr(lds) + slot * STAGE + ((tid & ~63) + 512 * i) * 16);
  };
  auto issue_advance = [&]() {
    if (++issue_kc == nkc) {
      issue_kc = 0;
      ++issue_tile;
      if (issue_tile < my_tiles) set_gallery_sources(issue_tile);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[gt][qt][i] = 0.f;

  if (nsteps > 0) {
    set_gallery_sources(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) issue_piece(0, i);
    issue_advance();
  }

  int kc = 0;
  int64_t ti = 0;
  for (int64_t step = 0; step < nsteps; ++step) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // explicit: see sim_glds_retire_and_sync()
    __builtin_amdgcn_s_barrier();
    const char* st = lds + (step & 1) * STAGE;
    const bool do_issue = step + 1 < nsteps;
    const int islot = (int)((step + 1) & 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int chunk = 2 * ks + h;
      u32x4 af[4], bf[2];
#pragma unroll
      for (int gt = 0; gt < 4; ++gt)
        af[gt] = *reinterpret_cast<const u32x4*>(st + sim_slot_off(wave_g * 128 + gt * 32 + r, chunk));
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
        bf[qt] = *reinterpret_cast<const u32x4*>(st + sim_slot_off(256 + wave_q * 64 + qt * 32 + r, chunk));
      if (do_issue && ks < 2) {  // four of the eight DMA pieces of stage step+1 per early k-substep
#pragma unroll
        for (int i = 0; i < 4; ++i) issue_piece(islot, 4 * ks + i);
      }
#pragma unroll
      for (int gt = 0; gt < 4; ++gt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          if constexpr (__is_same(T, _Float16))
            acc[gt][qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[gt]),
                                                                 __builtin_bit_cast(f16x8, bf[qt]), acc[gt][qt], 0, 0, 0);
          else
            acc[gt][qt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[gt]),
                                                                  __builtin_bit_cast(bf16x8, bf[qt]), acc[gt][qt], 0, 0, 0);
        }
    }
    if (do_issue) issue_advance();

    if (++kc == nkc) {
      // ---- tile epilogue: compare against the floor; candidates are rare -> one ballot per 32 x 32 tile
      const int64_t row0 = tile_row0(ti) + wave_g * 128;
#pragma unroll
      for (int gt = 0; gt < 4; ++gt) {
        const int64_t rbase = row0 + gt * 32 + 4 * h;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          unsigned mask = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int64_t row = rbase + (i & 3) + 8 * (i >> 2);
            const bool cand = (row < a.row_end) && (acc[gt][qt][i] > flo[qt]);
            mask |= cand ? (1u << i) : 0u;
          }
          if (__ballot(mask != 0u) != 0ull) {
            unsigned any = mask;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) any |= __shfl_xor(any, off);
            any = __builtin_amdgcn_readfirstlane(any);
            while (any != 0u) {  // wave-uniform slot loop: acc[..][i] with a scalar i stays in registers
              const int i = __builtin_ctz(any);
              any &= any - 1u;
              const float sc = acc[gt][qt][i];
              if ((mask >> i) & 1u) {
                const int pos = atomicAdd(a.cand_cnt + myq[qt], 1);
                if (pos < a.cap) {
                  a.cand_val[(int64_t)pos * a.nq + myq[qt]] = sc;
                  a.cand_idx[(int64_t)pos * a.nq + myq[qt]] = (int)(rbase + (i & 3) + 8 * (i >> 2));
                } else {
                  *a.overflow = 1;
                }
              }
            }
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[gt][qt][i] = 0.f;
        }
      }
      kc = 0;
      ++ti;
    }
  }
}

__global__ void pass_copy_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int64_t nq,
                                 int kk, int k, int done, int64_t idx_base,
                                 float* __restrict__ out_val, int64_t* __restrict__ out_idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq * kk) return;
  const int64_t qi = t / kk;
  const int j = (int)(t % kk);
  out_val[qi * k + done + j] = pv[t];
  out_idx[qi * k + done + j] = pi[t] < 0 ? -1 : (int64_t)pi[t] + idx_base;
}

// ----- host-side planning ---------------------------------------------------
// Which flow a call takes, with which kernel geometry, prefix, grids and workspace layout, is decided once by
// sim_topk_plan (sim_plan.h: plain C++, pinned on the CPU by tests/test_sim_plan_host.py).  The code below fills
// argument structs from that plan and launches: one function per flow, no state passed between them.

// the merge of `nlists` (+ the extra) sorted 32-bit-index lists by the kernel sim_merge_route names; a launch that
// could not read every list is refused
int launch_merge(const MergeArgs& m, hipStream_t st) {
  const int total = m.nlists + (m.extra_val ? 1 : 0);
  const SimMergeRoute r = sim_merge_route(total, m.out.k, m.ngroups);
  if (r.capacity < total) return HCIR_ERR_UNSUPPORTED;
  const unsigned merge_grid = (unsigned)hcir_cdiv(m.nq, 4);
  switch (r.kind) {
    case SIM_MERGE_FOUR_WAVES:
      static_assert(kMergeQuadMaxLPL == 4, "one instantiation per lists-per-lane count of sim_merge_route");
      if (r.lpl == 1)
        hipLaunchKernelGGL(topk_merge32q_kernel<1>, dim3((unsigned)m.nq), dim3(256), 0, st, m);
      else if (r.lpl == 2)
        hipLaunchKernelGGL(topk_merge32q_kernel<2>, dim3((unsigned)m.nq), dim3(256), 0, st, m);
      else if (r.lpl == 3)
        hipLaunchKernelGGL(topk_merge32q_kernel<3>, dim3((unsigned)m.nq), dim3(256), 0, st, m);
      else if (r.lpl == 4)
        hipLaunchKernelGGL(topk_merge32q_kernel<4>, dim3((unsigned)m.nq), dim3(256), 0, st, m);
      else
        return HCIR_ERR_UNSUPPORTED;
      break;
    case SIM_MERGE_WAVE:
      if (r.lpl != kMergeLPL) return HCIR_ERR_UNSUPPORTED;
      hipLaunchKernelGGL(topk_merge32_kernel<kMergeLPL>, dim3(merge_grid), dim3(256), 0, st, m);
      break;
    case SIM_MERGE_SELECT:
      if (r.lpl != kMergeLPL || m.kin != 16) return HCIR_ERR_UNSUPPORTED;
      hipLaunchKernelGGL(topk_merge_sel_kernel<kMergeLPL>, dim3(merge_grid, (unsigned)m.ngroups), dim3(256), 0, st, m);
      break;
    default: return HCIR_ERR_UNSUPPORTED;
  }
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

template <typename T, int KP, int QT, int WQ, int WGG>
void launch_scan_cfg(const ScanArgs& a, int grid_x, hipStream_t st) {
  static_assert(sim_geom(KP, 32 * QT * WQ).gm == 64 * WGG, "sim_plan.h kSimGeom");
  const int grid_y = (int)hcir_cdiv(a.nq, 32 * QT * WQ);
  if (QT == 1 && a.d % SimElem<T>::kPerStage == 0 && !a.floor_val)
    hipLaunchKernelGGL((sim_topk_scan<T, KP, QT, WQ, WGG, true, false, (QT == 1)>), dim3(grid_x, grid_y), dim3(256), 0,
                       st, a);
  else if (a.d % SimElem<T>::kPerStage == 0)
    hipLaunchKernelGGL((sim_topk_scan<T, KP, QT, WQ, WGG, true>), dim3(grid_x, grid_y), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((sim_topk_scan<T, KP, QT, WQ, WGG, false>), dim3(grid_x, grid_y), dim3(256), 0, st, a);
}

template <typename T>
void launch_scan(int kp, int qb, const ScanArgs& a, int grid_x, hipStream_t st) {
  if (kp == 64) {
    launch_scan_cfg<T, 64, 1, 1, 4>(a, grid_x, st);
  } else if (kp == 32) {
    if (qb == 32)
      launch_scan_cfg<T, 32, 1, 1, 4>(a, grid_x, st);
    else if (qb == 64)
      launch_scan_cfg<T, 32, 2, 1, 4>(a, grid_x, st);
    else
      launch_scan_cfg<T, 32, 2, 2, 2>(a, grid_x, st);
  } else if (qb == 32) {
    launch_scan_cfg<T, 16, 1, 1, 4>(a, grid_x, st);
  } else if (qb == 64) {
    launch_scan_cfg<T, 16, 1, 2, 2>(a, grid_x, st);
  } else {
    launch_scan_cfg<T, 16, 2, 2, 2>(a, grid_x, st);
  }
}

// candidate-append scan (no lists): geometry by query count only
template <typename T, int QT, int WQ, int WGG>
void launch_cand_cfg(const ScanArgs& a, int grid_x, hipStream_t st) {
  static_assert(sim_geom(16, 32 * QT * WQ).gm == 64 * WGG, "sim_plan.h kSimGeom");
  const int grid_y = (int)hcir_cdiv(a.nq, 32 * QT * WQ);
  if (a.d % SimElem<T>::kPerStage == 0)
    hipLaunchKernelGGL((sim_topk_scan<T, 16, QT, WQ, WGG, true, true>), dim3(grid_x, grid_y), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((sim_topk_scan<T, 16, QT, WQ, WGG, false, true>), dim3(grid_x, grid_y), dim3(256), 0, st, a);
}
template <typename T>
void launch_cand(int qb, const ScanArgs& a, int grid_x, hipStream_t st) {
  if (qb == 32)
    launch_cand_cfg<T, 1, 1, 4>(a, grid_x, st);
  else if (qb == 64)
    launch_cand_cfg<T, 1, 2, 2>(a, grid_x, st);
  else
    launch_cand_cfg<T, 2, 2, 2>(a, grid_x, st);
}

// f(T{}) with the element type of `dtype` (validated by the caller)
template <typename F>
void with_dtype(int dtype, F&& f) {
  if (dtype == HCIR_F32)
    f(float{});
  else if (dtype == HCIR_F16)
    f(_Float16{});
  else
    f(__bf16{});
}

struct Call {  // the caller's arguments
  const void *q, *g;
  const float *qn, *gn;
  int64_t nq, ng, idx_base;
  int d, k, dtype;
  float* out_val;
  int64_t* out_idx;
  hipStream_t st;
};

// list-keeping scan of rows [row_begin, row_end) by workgroups of `qb` queries
ScanArgs list_scan_args(const Call& c, const SimWorkspace& w, int qb, int k, int64_t row_begin, int64_t row_end) {
  ScanArgs a{};
  a.q = c.q;
  a.g = c.g;
  a.qn = c.qn;
  a.gn = c.gn;
  a.part_val = w.part_val;
  a.part_idx = w.part_idx;
  a.nq = c.nq;
  a.d = c.d;
  a.k = k;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.shared_stream = c.nq > qb ? 1 : 0;
  return a;
}
// (candidate scan first: the kernels sit in the code object in order of instantiation, which tools/cmp_device_asm.py
// and a plain diff of the device assembly rely on)
void launch_cand_scan(const Call& c, int qb, const ScanArgs& a, int grid_x) {
  with_dtype(c.dtype, [&](auto t) { launch_cand<decltype(t)>(qb, a, grid_x, c.st); });
}
void launch_list_scan(const Call& c, int kp, int qb, const ScanArgs& a, int grid_x) {
  with_dtype(c.dtype, [&](auto t) { launch_scan<decltype(t)>(kp, qb, a, grid_x, c.st); });
}

// partial lists -> the list of the `kout` best in the workspace (prefix / previous pass), rank kout - 1 to kth_val
MergeArgs merge_to_workspace(const Call& c, const SimWorkspace& w, int nlists, int kin, int kout, float* kth_val) {
  MergeArgs m{};
  m.vals = w.part_val;
  m.idx = w.part_idx;
  m.nq = c.nq;
  m.nlists = nlists;
  m.kin = kin;
  m.out.k = kout;
  m.out.val = w.pre_val;
  m.out.idx32 = w.pre_idx;
  m.out.kth_val = kth_val;
  return m;
}
// partial lists (+ the prefix list) -> the caller's output
MergeArgs merge_to_output(const Call& c, const SimWorkspace& w, int nlists, int kin, bool with_prefix,
                               const int* gate, int gate_want) {
  MergeArgs m{};
  m.vals = w.part_val;
  m.idx = w.part_idx;
  m.nq = c.nq;
  m.nlists = nlists;
  m.kin = kin;
  m.out.k = c.k;
  if (with_prefix) {
    m.extra_val = w.pre_val;
    m.extra_idx = w.pre_idx;
    m.kin_extra = c.k;
  }
  m.out.val = c.out_val;
  m.out.idx = c.out_idx;
  m.out.idx_base = c.idx_base;
  m.gate = TopkGate{gate, gate_want};
  return m;
}

// One list scan over every row + one merge.  With `gate`: the fallback of the group-floor candidate flow.
int run_single_scan(const SimTopkPlan& p, const SimWorkspace& w, const Call& c, const int* gate) {
  ScanArgs a = list_scan_args(c, w, p.qb, c.k, 0, c.ng);
  a.gate = gate;
  launch_list_scan(c, p.kp, p.qb, a, p.grid_a);
  HCIR_LAUNCH_CHECK();
  return launch_merge(merge_to_output(c, w, p.grid_a, p.kp, false, gate, 1), c.st);
}

// phase A of the list flow: rows [0, S) -> the prefix top-k list and its k-th score, the floor of what follows
int run_list_prefix(const SimTopkPlan& p, const SimWorkspace& w, const Call& c, int* zero_cnt) {
  launch_list_scan(c, p.kp, p.qb, list_scan_args(c, w, p.qb, c.k, 0, p.S), p.grid_a);
  HCIR_LAUNCH_CHECK();
  MergeArgs m = merge_to_workspace(c, w, p.grid_a, p.kp, c.k, w.floor_val);
  m.zero_cnt = zero_cnt;
  return launch_merge(m, c.st);
}

// The list flow: phase A unless the caller's flow has run it; phase B: rows [S, ng) with the prefix k-th score as
// floor, merged with the prefix list.  With `gate`, phase B is the fallback of a flow whose candidate buffer overflowed.
int run_list_two_phase(const SimTopkPlan& p, const SimWorkspace& w, const Call& c, const int* gate, bool phase_a_done) {
  if (!phase_a_done) {
    const int rc = run_list_prefix(p, w, c, nullptr);
    if (rc != HCIR_OK) return rc;
  }
  ScanArgs a = list_scan_args(c, w, p.qb, c.k, p.S, c.ng);
  a.floor_val = w.floor_val;
  a.gate = gate;
  launch_list_scan(c, p.kp, p.qb, a, p.grid_b);
  HCIR_LAUNCH_CHECK();
  return launch_merge(merge_to_output(c, w, p.grid_b, p.kp, true, gate, gate ? 1 : 0), c.st);
}

// <= 128 queries, k <= 64, big gallery (docs/LAB_NOTEBOOK.md "sim_topk: candidate flow").
//   A  rows [0, S): the 16-entry list kernel (its fixed cost is 53 us; the 64-entry one costs 131 us), workgroup
//      x in group x % G, G = 1 (k <= 16) or ceil(k / 16); one merge launch gives every group's floor - the
//      k-th (G = 1) or 16th best score of the group - and, for G = 1, the prefix top-k list;
//   B  a scan WITHOUT lists appends every row at / above the floor (min over the groups: >= k rows sit at or
//      above it) to the query's candidate buffer: G = 1 over rows [S, N) with `> floor` (a tie loses to the k
//      prefix rows with smaller indices), G > 1 over ALL rows with `>= floor` (the group lists do not hold the
//      prefix's top-k);
//   C  select: top-k of the candidates (+ the prefix list), one wave per query;
//   then the list flow as fallback, gated by the overflow flag (sim_plan_candidate).
int run_candidate_flow(const SimTopkPlan& p, const SimWorkspace& w, const Call& c) {
  const int merge_grid = (int)hcir_cdiv(c.nq, 4);
  ScanArgs s = list_scan_args(c, w, p.cand_qb, p.G == 1 ? c.k : 16, 0, p.S);
  launch_list_scan(c, 16, p.cand_qb, s, p.cand_grid_a);
  HCIR_LAUNCH_CHECK();
  MergeArgs m = merge_to_workspace(c, w, p.cand_grid_a, 16, s.k, w.floor_val);
  m.zero_cnt = w.cand_cnt;
  m.ngroups = p.G;
  // G = 1: four waves per query (the selection merge took 21.6 us there at 32 queries); G > 1: the selection merge
  if (const int rc = launch_merge(m, c.st)) return rc;
  s.row_begin = p.G == 1 ? p.S : 0;
  s.row_end = c.ng;
  s.floor_val = w.floor_val;
  s.floor_groups = p.G;
  s.floor_inclusive = p.G > 1 ? 1 : 0;
  s.cand_val = w.cand_val;
  s.cand_idx = w.cand_idx;
  s.cand_cnt = w.cand_cnt;
  s.overflow = w.overflow;
  s.cap = p.cand_cap;
  s.cand_query_major = 1;
  launch_cand_scan(c, p.cand_qb, s, p.cand_grid_b);
  HCIR_LAUNCH_CHECK();
  SelectArgs sa{};
  sa.cand_val = w.cand_val;
  sa.cand_idx = w.cand_idx;
  sa.cand_cnt = w.cand_cnt;
  sa.cap = p.cand_cap;
  if (p.G == 1) {
    sa.pre_val = w.pre_val;
    sa.pre_idx = w.pre_idx;
    sa.kpre = c.k;
  }
  sa.out.val = c.out_val;
  sa.out.idx = c.out_idx;
  sa.out.idx_base = c.idx_base;
  sa.out.k = c.k;
  sa.nq = c.nq;
  sa.gate = TopkGate{w.overflow, 0};
  // slots of a select launch: 64 (LPL - 1) candidates per wave (x 4 waves), the last slot of a lane is the prefix list's
  constexpr int kSel4LPL = (kCandCapBig + 255) / 256 + 1;
  static_assert(64 * (kSelLPLSmall - 1) >= kCandCapSmall && 64 * (kCandLPL - 1) >= kCandCap &&
                    256 * (kSel4LPL - 1) >= kCandCapBig, "a select kernel reads fewer candidates than its scan may append");
  if (p.select == SIM_SELECT_WAVE_SMALL && p.cand_cap <= kCandCapSmall)
    hipLaunchKernelGGL(topk_select_kernel<kSelLPLSmall>, dim3(merge_grid), dim3(256), 0, c.st, sa);
  else if (p.select == SIM_SELECT_WAVE && p.cand_cap <= kCandCap)
    hipLaunchKernelGGL(topk_select_kernel<kCandLPL>, dim3(merge_grid), dim3(256), 0, c.st, sa);
  else if (p.select == SIM_SELECT_FOUR_WAVES && p.cand_cap <= kCandCapBig)
    hipLaunchKernelGGL(topk_select4_kernel<kSel4LPL>, dim3((unsigned)c.nq), dim3(256), 0, c.st, sa);
  else
    return HCIR_ERR_UNSUPPORTED;
  HCIR_LAUNCH_CHECK();
  return p.fallback_phases == 2 ? run_list_two_phase(p, w, c, w.overflow, p.phase_a_done)
                                : run_single_scan(p, w, c, w.overflow);
}

// > 128 queries (MFMA-bound): list prefix, then the 256 x 256 tile scan collects the rare rows above the floor and one
// merge ranks them with the prefix list; the list-keeping phase B only runs (device-side gate) if a buffer overflowed.
int run_big_tile_flow(const SimTopkPlan& p, const SimWorkspace& w, const Call& c) {
  const int rc = run_list_prefix(p, w, c, w.cand_cnt);  // (the big scan's counters and overflow flag start at zero)
  if (rc != HCIR_OK) return rc;
  BigScanArgs b{};
  b.q = c.q;
  b.g = c.g;
  b.floor_val = w.floor_val;
  b.cand_val = w.cand_val;
  b.cand_idx = w.cand_idx;
  b.cand_cnt = w.cand_cnt;
  b.overflow = w.overflow;
  b.nq = c.nq;
  b.row_begin = p.S;
  b.row_end = c.ng;
  b.d = c.d;
  b.cap = p.cand_cap;
  with_dtype(c.dtype, [&](auto t) {
    using T = decltype(t);
    if constexpr (!std::is_same<T, float>::value)   // (fp32 never gets this flow)
      hipLaunchKernelGGL(sim_scan_big_kernel<T>, dim3((unsigned)p.big_grid_x, (unsigned)p.big_grid_y), dim3(512), 0,
                         c.st, b);
  });
  HCIR_LAUNCH_CHECK();
  MergeArgs m = merge_to_output(c, w, p.cand_cap, 1, true, w.overflow, 0);
  m.vals = w.cand_val;
  m.idx = w.cand_idx;
  m.nlists_q = w.cand_cnt;
  if (const int rc = launch_merge(m, c.st)) return rc;
  return run_list_two_phase(p, w, c, w.overflow, p.phase_a_done);
}

// k > 64: successive passes of <= 64 ranks below a moving ceiling.
int run_multipass(const SimTopkPlan& p, const SimWorkspace& w, const Call& c) {
  int done = 0;
  for (int pass = 0; pass < p.npass; ++pass) {
    const int kk = (c.k - done) < 64 ? (c.k - done) : 64;
    ScanArgs a = list_scan_args(c, w, p.qb, kk, 0, c.ng);
    a.ceil_val = pass ? w.ceil_val : nullptr;
    a.ceil_idx = pass ? w.ceil_idx : nullptr;
    launch_list_scan(c, p.kp, p.qb, a, p.grid_a);
    HCIR_LAUNCH_CHECK();
    MergeArgs m = merge_to_workspace(c, w, p.grid_a, p.kp, kk, w.ceil_val);
    m.out.kth_idx = w.ceil_idx;
    if (const int rc = launch_merge(m, c.st)) return rc;
    // scatter this pass's [nq][kk] block into out[:, done:done+kk]
    hipLaunchKernelGGL(pass_copy_kernel, dim3((unsigned)hcir_cdiv(c.nq * kk, 256)), dim3(256), 0, c.st,
                       w.pre_val, w.pre_idx, c.nq, kk, c.k, done, c.idx_base, c.out_val, c.out_idx);
    HCIR_LAUNCH_CHECK();
    done += kk;
  }
  return HCIR_OK;
}

}  // namespace

extern "C" {

#ifdef HCIR_DIAG_STAMPS
int hcir_debug_stamps(unsigned long long* host_dst) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 1024 * 8);
}
#endif

size_t hcir_sim_topk_workspace_bytes(int64_t nq, int64_t ng, int32_t d, int32_t k, int dtype) {
  if (nq <= 0 || ng <= 0 || k <= 0) return 0;
  return sim_topk_plan(nq, ng, d, k, dtype, false, false).ws_bytes;  // (the layout does not depend on the norms)
}

int hcir_sim_topk(const void* q, int64_t nq, const void* g, int64_t ng, int32_t d, int32_t k,
                  int dtype, const float* q_inv_norm, const float* g_inv_norm, int64_t idx_base,
                  float* out_val, int64_t* out_idx, void* workspace, size_t workspace_bytes,
                  void* stream) {
  HCIR_ENTER();
  if (!q || !g || !out_val || !out_idx) return HCIR_ERR_INVALID;
  if (nq <= 0 || ng <= 0 || d <= 0 || (d & 7) || k <= 0 || k > HCIR_TOPK_MAX) return HCIR_ERR_INVALID;
  if (k > ng || ng >= (int64_t(1) << 31)) return HCIR_ERR_INVALID;
  if (dtype != HCIR_F32 && dtype != HCIR_F16 && dtype != HCIR_BF16) return HCIR_ERR_UNSUPPORTED;
  const SimTopkPlan p = sim_topk_plan(nq, ng, d, k, dtype, q_inv_norm != nullptr, g_inv_norm != nullptr);
  if (!workspace || workspace_bytes < p.ws_bytes) return HCIR_ERR_WORKSPACE;
  const SimWorkspace w = sim_workspace(workspace, nq, p);
  const Call c{q, g, q_inv_norm, g_inv_norm, nq, ng, idx_base, d, k, dtype, out_val, out_idx,
               static_cast<hipStream_t>(stream)};
  switch (p.flow) {
    case SIM_FLOW_SINGLE_SCAN: return run_single_scan(p, w, c, nullptr);
    case SIM_FLOW_LIST_TWO_PHASE: return run_list_two_phase(p, w, c, nullptr, false);
    case SIM_FLOW_CANDIDATE: return run_candidate_flow(p, w, c);
    case SIM_FLOW_BIG_TILE: return run_big_tile_flow(p, w, c);
    default: return run_multipass(p, w, c);
  }
}

int hcir_topk_merge(const float* vals, const int64_t* idx, int32_t nlists, int64_t nq, int32_t k_in,
                    int32_t k_out, float* out_val, int64_t* out_idx, void* stream) {
  HCIR_ENTER();
  if (!vals || !idx || !out_val || !out_idx) return HCIR_ERR_INVALID;
  if (nlists <= 0 || nq <= 0 || k_in <= 0 || k_out <= 0) return HCIR_ERR_INVALID;
  if (nlists > 64 * kMergeLPL) return HCIR_ERR_UNSUPPORTED;
  const Merge64Args m{vals, idx, out_val, out_idx, nq, nlists, k_in, k_out};
  hipLaunchKernelGGL(topk_merge_kernel, dim3((int)hcir_cdiv(nq, 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), m);
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

}  // extern "C"
