// attn.hip — fused multi-head self-attention forward for ViT token counts (T <= 288).
//
// Replaces Attention.forward (HP/src/models_vit.py:69-78) and the
// nn.MultiheadAttention inside torchvision's EncoderBlock (HP/src/main_backbone.py:554):
//   out = softmax((q * scale) k^T) v   per (batch, head).
//
// The arithmetic of one 32-row query tile is written ONCE (the attn_* helpers below) and is shared by the three
// kernels, so that their results agree by construction:
//   S^T = K . Q^T   : MFMA 32x32x16 f16, keys on the MFMA row, queries on the column
//                     -> a lane owns ONE query and holds its scores in registers:
//                     row max / exp2 / row sum need one cross-half shuffle only.
//   O^T = V^T . P   : the fp32 score accumulators, converted pairwise to fp16, ARE the
//                     B operand of the second MFMA (cdna_hip_programming.md §3, "An
//                     accumulator tile as the next MFMA's operand"); the A operand V^T is
//                     read from the row-major V image with ds_read_b64_tr_b16 (T10).
// The kernels keep what differs between them: how K, V and Q reach LDS and registers, which tiles a wave walks, the
// barriers and the waits.
//   attn_fwd_kernel<NKT>              head_dim 64: one 4-wave workgroup per (b, head), wave w owns query tiles w,
//                                     w+4, ...; K and V of the head are staged ONCE into LDS by LDS-DMA and shared by
//                                     all waves.  Four waves (not one per query tile) keep two workgroups resident
//                                     per CU, so one workgroup's K/V staging latency hides under the other's MFMAs.
//   attn_fwd2_kernel                  head_dim 64, T in (192, 224], all query rows: persistent, double-buffered.
//   attn_fwd_generic_kernel<HD, NKT>  any other head_dim: register-staged, plain images.  With head_dim 32 it also
//                                     serves training (the MAE decoder): it writes the per-row log2-sum-exp in the
//                                     layout and domain of the head_dim-64 kernels, behind the same row stores.
// LDS images (KVImage): with head_dim 64, K rows are 128 B, 16-B slots XOR-swizzled with (key>>1)&7 (ds_read_b128
// conflict-free); V rows are 128 B with the two 64-B halves swapped when key bit 1 is set (the 4-row x 32-col
// transposed reads of a half-wave then cover all 64 banks).  The generic kernel's images are plain.
#include <type_traits>

#include "common.h"

namespace {

struct AttnArgs {
  const _Float16* qkv;  // [B][T][3][H][HD]
  _Float16* out;        // [B][NQ][H*HD]
  int t, h;
  int nq;               // query rows computed per (b, head): T, or fewer (CLS-only last layer: 1)
  float scale_log2e;
  float* lse;           // optional [B][H][T]: log2 of the softmax denominator incl. the row maximum (training)
};

// Where the K and V images of one head keep their data: the fill asks for the place of a 16-B chunk, the tile code
// for the place it reads.  Both swizzles are XORs, so the same function answers "where does chunk c of this row go"
// and "which chunk does slot c of this row hold" (LDS-DMA lands linearly and swizzles its source instead).
template <int HD, bool Swizzled>
struct KVImage {
  static_assert(HD % 16 == 0 && HD <= 128 && (!Swizzled || HD == 64), "head_dim");
  static constexpr int HDP = (HD + 31) / 32 * 32;      // V / output dims padded to whole 32-row MFMA tiles
  static constexpr int NS = HD / 16, NDT = HDP / 32;   // 16-dim steps of S^T, 32-dim tiles of O^T
  static constexpr int KPB = HD * 2, VPB = HDP * 2;    // row pitches in bytes
  // byte offset inside key's K row of 16-B chunk c16; inside key's V row of column col
  static __device__ __forceinline__ int k_in_row(int key, int c16) {
    return (Swizzled ? c16 ^ ((key >> 1) & 7) : c16) << 4;
  }
  static __device__ __forceinline__ int v_in_row(int key, int col) {
    return (Swizzled ? col ^ (((key >> 1) & 1) << 5) : col) * 2;
  }
  static __device__ __forceinline__ int k_off(int key, int c16) { return key * KPB + k_in_row(key, c16); }
  static __device__ __forceinline__ int v_off(int key, int col) { return key * VPB + v_in_row(key, col); }
};

// ---- the query tile: a lane is (r = lane & 31, h = lane >> 5), and (grp = lane >> 4, li = lane & 15) for the
//      transposed reads.  sc[], sum and oacc[] live in the kernel and the indices come by value: one helper for the
//      whole tile that derives them from `lane` and declares sc[] itself compiled to 25-50 instructions more per tile.

// S^T = K . Q^T: lane (q = r, half h) holds Q[q][16s + 8h .. +7] in qf[s]
template <int NKT, class Img>
__device__ __forceinline__ void attn_scores(const char* ks, const f16x8 (&qf)[Img::NS], int r, int h,
                                            f32x16 (&sc)[NKT]) {
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
    const int key = kt * 32 + r;
#pragma unroll
    for (int s = 0; s < Img::NS; ++s) {
      const f16x8 kf = *reinterpret_cast<const f16x8*>(ks + Img::k_off(key, 2 * s + h));
      sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sc[kt], 0, 0, 0);
    }
  }
}

// row maximum over the keys < t (registers + one cross-half exchange); only the LAST key tile can hold keys >= T
// (32 NKT - T < 32), so only it is masked.  Keys past T are staged as the last real key: finite data whose scores
// become -inf here, so that their probabilities are exactly 0.
template <int NKT>
__device__ __forceinline__ float attn_masked_max(f32x16 (&sc)[NKT], int t, int h) {
  const float ninf = -__builtin_huge_valf();
  float mx = ninf;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int key = (NKT - 1) * 32 + acc_row(i, h);
    sc[NKT - 1][i] = key < t ? sc[NKT - 1][i] : ninf;
  }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sc[kt][i]);
  return fmaxf(mx, __shfl_xor(mx, 32));
}

// P = exp2(S scale log2e - max) and its row sum for one key tile
__device__ __forceinline__ void attn_exp_tile(f32x16& sc, float scale_log2e, float mxs, float& sum) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[i], scale_log2e, -mxs));
    sc[i] = p;
    sum += p;
  }
}

// P, its row sum (this lane's half of it) and O^T = V^T . P, software-pipelined over the key tiles: the exponentials
// of key tile kt + 1 stand between the transposed V reads and the MFMAs of key tile kt IN ONE BASIC BLOCK (the lse
// store, a branch, stays behind the loop), so the 16 x (fma, v_exp_f32, add) chains issue in the shadow of the matrix
// pipe.  As one block of 112 v_exp_f32 in front of the PV MFMAs (what hipcc emitted for the plain loop nest) the
// wave's matrix pipe idled for ~1800 cycles per query tile.
template <int NKT, class Img>
__device__ __forceinline__ void attn_exp_pv(const char* vs, f32x16 (&sc)[NKT], float scale_log2e, float mxs, int grp,
                                            int li, float& sum, f32x16 (&oacc)[Img::NDT]) {
  constexpr int NDT = Img::NDT;
#pragma unroll
  for (int t2 = 0; t2 < NDT; ++t2)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[t2][i] = 0.f;
  attn_exp_tile(sc[0], scale_log2e, mxs, sum);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f16x8 pf[2], vf[2][NDT];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[s][j] = (_Float16)sc[kt][8 * s + j];
#pragma unroll
      for (int hdt = 0; hdt < NDT; ++hdt) {
        // transposed read: this lane supplies row (kb + li>>2), columns c0 + 4*(li&3) .. +3
        const int c0 = 32 * hdt + 16 * (grp & 1) + 4 * (li & 3);
        const int kb = 32 * kt + 16 * s + 4 * (grp >> 1) + (li >> 2);
#pragma unroll
        for (int half = 0; half < 2; ++half) tr_read_half(vf[s][hdt], half, vs + Img::v_off(kb + 8 * half, c0));
      }
    }
    if (kt + 1 < NKT) attn_exp_tile(sc[kt + 1], scale_log2e, mxs, sum);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int hdt = 0; hdt < NDT; ++hdt)
        oacc[hdt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[s][hdt], pf[s], oacc[hdt], 0, 0, 0);
  }
}

// the lane's four normalised outputs g4 of one O^T tile: query r, dims 8 g4 + 4 h .. + 3 of the tile's 32
__device__ __forceinline__ f16x4 attn_out4(const f32x16& oacc, int g4, float inv) {
  f16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (_Float16)(oacc[4 * g4 + e] * inv);
  return o;
}

// Where the rows of the query tile at q0 go: row q0's place in `out`, the elements between rows, and how many of the
// tile's 32 rows are to be stored.  Wave-uniform, so that a row's address is one multiply-add away.
struct AttnOutTile {
  _Float16* row0;
  int64_t pitch;
  int rows;
};
template <int HD>
__device__ __forceinline__ AttnOutTile attn_out_tile(const AttnArgs& a, int64_t b, int head, int q0) {
  const int64_t pitch = (int64_t)a.h * HD;
  return AttnOutTile{a.out + (b * a.nq + q0) * pitch + head * HD, pitch, a.nq - q0};
}

// Row store, head_dim 64: the lane owns query row q0 + r and 4-dim pieces of it; a direct store would write 16 B of
// 32 different rows per instruction (partial lines).  The wave transposes its 32 x 64 tile through 4 KB of LDS `ot`
// (16-B chunks XOR-swizzled with row & 7) and stores whole 128-B rows: 8 lanes x 16 B.
__device__ __forceinline__ void attn_store_rows_lds(const AttnOutTile& o, char* ot, const f32x16 (&oacc)[2], float inv,
                                                    int lane, int r, int h) {
#pragma unroll
  for (int hdt = 0; hdt < 2; ++hdt) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int chunk = 4 * hdt + g4;  // 16-B chunk = 8 head dims; h picks its 8-B half
      *reinterpret_cast<f16x4*>(ot + r * 128 + ((chunk ^ (r & 7)) << 4) + 8 * h) = attn_out4(oacc[hdt], g4, inv);
    }
  }
  const int rr = lane >> 3, cc = lane & 7;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = it * 8 + rr;
    const u32x4 v = *reinterpret_cast<const u32x4*>(ot + row * 128 + ((cc ^ (row & 7)) << 4));
    if (row < o.rows) *reinterpret_cast<u32x4*>(o.row0 + row * o.pitch + cc * 8) = v;
  }
}

// Row store without the LDS tile: 8 bytes per lane and piece; the dims a padded last O^T tile computed past HD stay
// unstored
template <int HD, int NDT>
__device__ __forceinline__ void attn_store_rows_direct(const AttnOutTile& o, const f32x16 (&oacc)[NDT], float inv,
                                                       int r, int h) {
  if (r < o.rows) {
    _Float16* orow = o.row0 + r * o.pitch;
#pragma unroll
    for (int hdt = 0; hdt < NDT; ++hdt) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int dim = 32 * hdt + 8 * g4 + 4 * h;
        if (HD % 32 == 0 || dim < HD) *reinterpret_cast<f16x4*>(orow + dim) = attn_out4(oacc[hdt], g4, inv);
      }
    }
  }
}

// p = exp2(s * scale_log2e - lse): what hcir_attn_bwd recomputes P from.  `sum` is the whole row's.
__device__ __forceinline__ void attn_store_lse(const AttnArgs& a, int64_t b, int head, int q0, int r, int h, float mxs,
                                               float sum) {
  if (a.lse && h == 0 && q0 + r < a.nq)
    a.lse[(b * a.h + head) * (int64_t)a.t + q0 + r] = mxs + __builtin_amdgcn_logf(sum);
}

template <int NKT>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnArgs a) {
  using Img = KVImage<64, true>;
  constexpr int TP = 32 * NKT;
  // K and V images, then a 4 KB output-transposition tile per wave
  constexpr bool kTrans = NKT <= 7;  // with 8-9 key tiles the extra 16 KB would cost the second workgroup per CU
  __shared__ __attribute__((aligned(16))) char lds[2 * TP * 128 + (kTrans ? 4 * 4096 : 0)];
  char* ks = lds;
  char* vs = lds + TP * 128;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthreads = blockDim.x;
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.x % a.h;
  const int64_t b = blockIdx.x / a.h;
  const int64_t row_stride = (int64_t)3 * a.h * 64;  // elements between tokens
  const _Float16* base = a.qkv + b * a.t * row_stride + head * 64;
  const _Float16* qg = base;
  const _Float16* kg = base + (int64_t)a.h * 64;
  const _Float16* vg = base + (int64_t)2 * a.h * 64;

  // ---- stage K and V by LDS-DMA: every piece of the head in flight at once, no VGPR round trip.
  // The LDS destination of a wave instruction is linear (base + lane*16), so both swizzles are
  // applied to the per-lane SOURCE chunk (k_in_row / v_in_row are bytes, the pointers fp16).  Keys past T are
  // clamped to the last real key.
  for (int slot0 = (tid & ~63); slot0 < TP * 8; slot0 += nthreads) {
    const int slot = slot0 + lane;
    const int key = slot >> 3, pc = slot & 7;
    const int src_key = key < a.t ? key : a.t - 1;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(kg + src_key * row_stride + Img::k_in_row(key, pc) / 2),
        (__attribute__((address_space(3))) void*)(ks + slot0 * 16), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(vg + src_key * row_stride + Img::v_in_row(key, 8 * pc) / 2),
        (__attribute__((address_space(3))) void*)(vs + slot0 * 16), 16, 0, 0);
  }
  // Q fragments come straight from global.  The first tile's fragments are requested together with the K/V DMA,
  // the next tile's at the top of the current tile, so their latency is never exposed.
  auto load_q = [&](int qt, f16x8 (&dst)[4]) {
    int qrow = qt * 32 + r;
    qrow = qrow < a.t ? qrow : a.t - 1;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      dst[s] = *reinterpret_cast<const f16x8*>(qg + qrow * row_stride + 16 * s + 8 * h);
  };
  f16x8 qf[4], qn[4];
  load_q(wave, qf);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // explicit: see sim_glds_retire_and_sync()
  __syncthreads();
  const int nqt = (a.nq + 31) >> 5;
  const int grp = lane >> 4, li = lane & 15;

  for (int qt = wave; qt < nqt; qt += 4) {
    // opaque per-iteration offset: stops hipcc from hoisting the ~80 loop-invariant LDS addresses
    // out of the loop (that cost 256 VGPRs + scratch spills); they are re-derived from `lane` here
    int opaque = 0;
    asm volatile("" : "+v"(opaque));
    const int q0 = qt * 32;
    if (qt + 4 < nqt) load_q(qt + 4, qn);

    f32x16 sc[NKT], oacc[2];
    attn_scores<NKT, Img>(ks + opaque, qf, r, h, sc);
    const float mxs = attn_masked_max(sc, a.t, h) * a.scale_log2e;
    float sum = 0.f;
    attn_exp_pv<NKT, Img>(vs + opaque, sc, a.scale_log2e, mxs, grp, li, sum, oacc);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    attn_store_lse(a, b, head, q0, r, h, mxs, sum);
    const AttnOutTile o = attn_out_tile<64>(a, b, head, q0);
    if constexpr (kTrans)
      attn_store_rows_lds(o, lds + 2 * TP * 128 + wave * 4096 + opaque, oacc, inv, lane, r, h);
    else
      attn_store_rows_direct<64>(o, oacc, inv, r, h);
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = qn[s];
  }
}

// --------------------------------------------------------------------------
// T in (192, 224] (ViT-B/16: 197 tokens), all query rows: PERSISTENT workgroup of seven waves, wave w owns query tile
// w of every (b, head) item the workgroup walks over; two K / V image pairs in LDS, the next item's pair filled by
// LDS-DMA (lds_dma16: invisible to hipcc, see common.h) and the next item's Q fragments requested while the current
// item computes; one barrier per item.  The 4-wave kernel above loads, computes and stores in sequence and relies on
// its second co-resident workgroup for overlap: with one key tile of compute it takes 197 us per launch at 880 images
// (all bytes moved), with all seven 286 us - 89 us of compute standing outside the memory time.  (Round 2's persistent
// attempt gained 2.5 %: its pending transfers were retired by the compiler in front of every transposed V read.)
// The tile arithmetic and the LDS images are those of attn_fwd_kernel<7>, the same code.
// --------------------------------------------------------------------------
constexpr int kF2NKT = 7, kF2Rows = 32 * kF2NKT, kF2Img = kF2Rows * 128;

__global__ __launch_bounds__(64 * kF2NKT, 1) void attn_fwd2_kernel(AttnArgs a, int items) {
  using Img = KVImage<64, true>;
  constexpr int NKT = kF2NKT;
  __shared__ __attribute__((aligned(16))) char lds[4 * kF2Img + kF2NKT * 4096];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int grp = lane >> 4, li = lane & 15;
  const int row_stride = 3 * a.h * 64;   // elements between tokens
  const uint32_t lds0 = lds_addr(lds);
  const int q0 = wave * 32;
  const bool active = q0 < a.nq;                 // this wave's query tile exists
  auto item_base = [&](int item) { return ((int64_t)(item / a.h) * a.t) * row_stride + (item % a.h) * 64; };

  // K / V images of `item` into buffer `buf`: 2 x 28 wave instructions of 8 rows, four of each per wave
  auto dma_kv = [&](int item, int buf) {
    const _Float16* kg = a.qkv + item_base(item) + (int64_t)a.h * 64;
    const _Float16* vg = kg + (int64_t)a.h * 64;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ii = wave + u * NKT;
      const int key = ii * 8 + (lane >> 3), pc = lane & 7;
      const int src = key < a.t ? key : a.t - 1;   // past T: the last real key (finite; masked / P = 0)
      const uint32_t rowoff = (uint32_t)(src * row_stride * 2);
      lds_dma16(kg, rowoff + Img::k_in_row(key, pc), lds0 + buf * 2 * kF2Img + ii * 1024);
      lds_dma16(vg, rowoff + Img::v_in_row(key, 8 * pc), lds0 + buf * 2 * kF2Img + kF2Img + ii * 1024);
    }
  };
  f16x8 qf[4], qn[4];
  auto load_q = [&](int item, f16x8 (&dst)[4]) {
    int qrow = q0 + r;
    qrow = qrow < a.t ? qrow : a.t - 1;
    const char* qg = reinterpret_cast<const char*>(a.qkv + item_base(item));
    const uint32_t off = (uint32_t)(qrow * row_stride * 2 + 16 * h);
#pragma unroll
    for (int s = 0; s < 4; ++s) dst[s] = *reinterpret_cast<const f16x8*>(qg + (off + 32 * s));
  };

  int item = blockIdx.x, buf = 0;
  if (item < items) {
    dma_kv(item, 0);
    load_q(item, qf);
  }
  while (item < items) {
    // this item's images and Q fragments have landed (issued an item ago).  (A counted wait that leaves the previous
    // item's row stores in flight is of no use here: the stores sit under per-lane predicates, so the compiler's own
    // wait for the Q registers below counts none of them and drains everything anyway.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(qf[s]));
    __syncthreads();   // ... and every wave is done with the other buffer (the previous item's)
    const int next = item + gridDim.x;
    if (next < items) {
      dma_kv(next, buf ^ 1);
      load_q(next, qn);
    }
    if (active) {
      int opaque = 0;
      asm volatile("" : "+v"(opaque));
      const char* ksl = lds + buf * 2 * kF2Img + opaque;
      const int head = item % a.h;
      const int64_t b = item / a.h;
      f32x16 sc[NKT], oacc[2];
      attn_scores<NKT, Img>(ksl, qf, r, h, sc);
      const float mxs = attn_masked_max(sc, a.t, h) * a.scale_log2e;
      float sum = 0.f;
      attn_exp_pv<NKT, Img>(ksl + kF2Img, sc, a.scale_log2e, mxs, grp, li, sum, oacc);
      sum += __shfl_xor(sum, 32);
      attn_store_rows_lds(attn_out_tile<64>(a, b, head, q0), lds + 4 * kF2Img + wave * 4096 + opaque, oacc,
                          1.0f / sum, lane, r, h);
      attn_store_lse(a, b, head, q0, r, h, mxs, sum);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = qn[s];
    item = next;
    buf ^= 1;
  }
}

// --------------------------------------------------------------------------
// Any head_dim that is a multiple of 16 up to 128 (vit_huge_patch14: 1280 / 16 = 80, HP/src/models_vit.py:266-270).
// The same tile code as attn_fwd_kernel; correctness-first staging: K and V go through registers into plain
// (unswizzled) LDS images, K rows HD * 2 bytes, V rows padded with zeros to a multiple of 32 dims so that the
// O^T = V^T . P tiles of 32 dims need no edge case (the padded output rows are computed and not stored).
// The tuned head_dim-64 kernel above is what every BASELINE config runs.
// --------------------------------------------------------------------------
template <int HD, int NKT>
__global__ __launch_bounds__(256, 1) void attn_fwd_generic_kernel(AttnArgs a) {
  using Img = KVImage<HD, false>;
  constexpr int TP = 32 * NKT, HDP = Img::HDP, NS = Img::NS, NDT = Img::NDT;
  __shared__ __attribute__((aligned(16))) char lds[TP * (Img::KPB + Img::VPB)];
  char* ks = lds;
  char* vs = lds + TP * Img::KPB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.x % a.h;
  const int64_t b = blockIdx.x / a.h;
  const int64_t row_stride = (int64_t)3 * a.h * HD;
  const _Float16* base = a.qkv + b * a.t * row_stride + head * HD;
  const _Float16* qg = base;
  const _Float16* kg = base + (int64_t)a.h * HD;
  const _Float16* vg = base + (int64_t)2 * a.h * HD;
  for (int slot = tid; slot < TP * (HDP / 8); slot += 256) {
    const int key = slot / (HDP / 8), c = slot % (HDP / 8);
    const int src_key = key < a.t ? key : a.t - 1;
    u32x4 kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
    if (c * 8 < HD) {
      kv = *reinterpret_cast<const u32x4*>(kg + src_key * row_stride + c * 8);
      vv = *reinterpret_cast<const u32x4*>(vg + src_key * row_stride + c * 8);
      *reinterpret_cast<u32x4*>(ks + Img::k_off(key, c)) = kv;
    }
    *reinterpret_cast<u32x4*>(vs + Img::v_off(key, 8 * c)) = vv;
  }
  __syncthreads();
  const int nqt = (a.nq + 31) >> 5;
  const int grp = lane >> 4, li = lane & 15;
  for (int qt = wave; qt < nqt; qt += 4) {
    const int q0 = qt * 32;
    int qrow = q0 + r;
    qrow = qrow < a.t ? qrow : a.t - 1;
    f16x8 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = *reinterpret_cast<const f16x8*>(qg + qrow * row_stride + 16 * s + 8 * h);
    f32x16 sc[NKT], oacc[NDT];
    attn_scores<NKT, Img>(ks, qf, r, h, sc);
    const float mxs = attn_masked_max(sc, a.t, h) * a.scale_log2e;
    float sum = 0.f;
    attn_exp_pv<NKT, Img>(vs, sc, a.scale_log2e, mxs, grp, li, sum, oacc);
    sum += __shfl_xor(sum, 32);
    attn_store_rows_direct<HD>(attn_out_tile<HD>(a, b, head, q0), oacc, 1.0f / sum, r, h);
    attn_store_lse(a, b, head, q0, r, h, mxs, sum);   // training (head_dim 32: the MAE decoder); a.lse is null otherwise
  }
}

// f(std::integral_constant<int, N>) for the kernel instantiation that covers nkt key tiles, N = 1..9 (T <= 288)
template <int N = 1, class F>
static void attn_with_key_tiles(int nkt, F&& f) {
  if constexpr (N == 9) {
    f(std::integral_constant<int, 9>{});
  } else {
    if (nkt == N) f(std::integral_constant<int, N>{});
    else attn_with_key_tiles<N + 1>(nkt, f);
  }
}

template <int HD>
static void attn_generic_launch(const AttnArgs& a, int nkt, dim3 grid, hipStream_t st) {
  attn_with_key_tiles(nkt, [&](auto n) {
    hipLaunchKernelGGL((attn_fwd_generic_kernel<HD, decltype(n)::value>), grid, dim3(256), 0, st, a);
  });
}

}  // namespace

static int attn_fwd_launch(const void* qkv, int64_t b, int32_t t, int32_t h, int32_t hd, float scale, int32_t nq,
                           void* out, float* lse, void* stream) {
  HCIR_ENTER();
  if (!qkv || !out || b <= 0 || t <= 0 || h <= 0 || nq <= 0 || nq > t) return HCIR_ERR_INVALID;
  if (t > 288) return HCIR_ERR_UNSUPPORTED;
  // the log-sum-exp output exists where hcir_attn_bwd does: head_dim 64 and 32
  if (hd != 64 && ((lse && hd != 32) || (hd != 32 && hd != 48 && hd != 80 && hd != 96 && hd != 128)))
    return HCIR_ERR_UNSUPPORTED;
  if (b * h > 0x7fffffff) return HCIR_ERR_INVALID;
  AttnArgs a{static_cast<const _Float16*>(qkv), static_cast<_Float16*>(out), t, h, nq,
             scale * 1.44269504088896340736f, lse};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nkt = (t + 31) / 32;   // the kernels are built for a number of key tiles
  const dim3 grid((unsigned)(b * h));
  if (hd != 64) {   // generic (unswizzled, register-staged) kernel
    if (hd == 32) attn_generic_launch<32>(a, nkt, grid, st);
    else if (hd == 48) attn_generic_launch<48>(a, nkt, grid, st);
    else if (hd == 80) attn_generic_launch<80>(a, nkt, grid, st);
    else if (hd == 96) attn_generic_launch<96>(a, nkt, grid, st);
    else attn_generic_launch<128>(a, nkt, grid, st);
    HCIR_LAUNCH_CHECK();
    return HCIR_OK;
  }
  if (nkt == kF2NKT && nq == t && b * h >= 512) {
    const int items = (int)(b * h);
    hipLaunchKernelGGL(attn_fwd2_kernel, dim3(256), dim3(64 * kF2NKT), 0, st, a, items);
    HCIR_LAUNCH_CHECK();
    return HCIR_OK;
  }
  // 4 waves walk the query tiles
  attn_with_key_tiles(nkt, [&](auto n) {
    hipLaunchKernelGGL(attn_fwd_kernel<decltype(n)::value>, grid, dim3(256), 0, st, a);
  });
  HCIR_LAUNCH_CHECK();
  return HCIR_OK;
}

extern "C" int hcir_attn_fwd(const void* qkv, int64_t b, int32_t t, int32_t h, int32_t hd, float scale, int32_t nq,
                             void* out, void* stream) {
  return attn_fwd_launch(qkv, b, t, h, hd, scale, nq, out, nullptr, stream);
}

// training forward: all T query rows, and the per-row log2-sum-exp for hcir_attn_bwd
extern "C" int hcir_attn_fwd_lse(const void* qkv, int64_t b, int32_t t, int32_t h, int32_t hd, float scale,
                                 void* out, float* lse, void* stream) {
  if (!lse) return HCIR_ERR_INVALID;
  return attn_fwd_launch(qkv, b, t, h, hd, scale, t, out, lse, stream);
}
