/*
 * hcir.h — C ABI of libhcir.so, the MI355X (gfx950) retrieval hot path.
 *
 * The reference (atunnd/Hair-centric-Image-Retrieval) has no FFI: its hot path is
 * Python calling torch / torchvision / lightly / scikit-learn.  Each entry point
 * below replaces one of those library calls; the reference call site it stands in
 * for is cited as  <file>:<line>  relative to the reference root
 * (HP/ = HairPretraining/).  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add at each site.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller (PyTorch tensor
 *     .data_ptr()); the library allocates nothing and keeps no global state.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream()
 *     .cuda_stream); every call is asynchronous on that stream.
 *   - Return value: HCIR_OK (0) or a negative hcir_status.  Nothing throws
 *     across the ABI.  hcir_status_string() maps a code to text.
 *   - Row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 *   - Tie-break of every top-k: score descending, then index ascending.
 */
#ifndef HCIR_H
#define HCIR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  HCIR_OK = 0,
  HCIR_ERR_INVALID = -1,      /* bad argument (null pointer, k > n, d % 8 != 0 ...) */
  HCIR_ERR_UNSUPPORTED = -2,  /* valid request this build has no kernel for       */
  HCIR_ERR_LAUNCH = -3,       /* HIP reported a launch error                      */
  HCIR_ERR_WORKSPACE = -4     /* workspace too small                              */
} hcir_status;

typedef enum {
  HCIR_F32 = 0, /* fp32 storage, exact-fp32 MFMA (k-ordered fmaf chain)    */
  HCIR_F16 = 1, /* fp16 storage, fp16 MFMA, fp32 accumulate               */
  HCIR_BF16 = 2 /* bf16 storage, bf16 MFMA, fp32 accumulate               */
} hcir_dtype;

int hcir_version(void);
const char* hcir_status_string(int status);
/* "<16 hex digits: sha256 of the kernel sources this binary was compiled from>[ -D build flags]".  bench.py reports a
 * recorded PMC summary only when it was taken on a binary with this id. */
const char* hcir_build_id(void);

/* ------------------------------------------------------------------ *
 * Row norms.  out[i] = 1 / max(||x_i||_2, eps)   (fp32)
 * Replaces the normalisation half of
 *   sklearn cosine_similarity / cosine_distances   (HP/src/classification_engine.py:80-82,
 *                                                    src/models/hair_encoder.py:193)
 *   embeddings / norm.clamp(min=1e-8)               (HP/src/neg_sampling.py:35)
 * ------------------------------------------------------------------ */
int hcir_row_invnorm(const void* x, int64_t n, int32_t d, int64_t ldx, int dtype,
                     float eps, float* out, void* stream);

/* In-place-capable L2 normalise of fp32 rows, optional second output in fp16:
 *   y = x / max(||x||, eps)            torch.nn.functional.normalize(x, dim=1)
 * (HP/src/classification_engine.py:50,62).  y_f32 and/or y_f16 may be NULL. */
int hcir_l2_normalize(const float* x, int64_t n, int32_t d, float eps, float* y_f32,
                      void* y_f16, void* stream);

/* ------------------------------------------------------------------ *
 * Brute-force cosine / inner-product top-k:  query x gallery.
 *   score[i][j] = <q_i, g_j> * (q_inv_norm ? q_inv_norm[i] : 1)
 *                            * (g_inv_norm ? g_inv_norm[j] : 1)
 *   out_val[i][0..k) = the k largest scores of row i, descending
 *   out_idx[i][0..k) = idx_base + j of those scores (ties: smaller j first)
 * Replaces
 *   KNeighborsClassifier(metric="cosine").kneighbors   HP/src/classification_engine.py:80-82
 *   cosine_similarity + np.argsort[::-1][:top_k]       src/models/hair_encoder.py:193-194
 *   torch.mm + torch.sort (rank-k pick)                HP/src/neg_sampling.py:37,45-51
 * The Q x N score matrix is never materialised.  dtype is the storage type of
 * BOTH q and g.  HCIR_F32 scores are bit-reproducible: each score is one fp32
 * fmaf chain over k in the order documented in DESIGN.md ("sim_topk k-order"),
 * which oracle/knn_oracle.c follows.
 * Requirements: d % 8 == 0, 1 <= k <= min(ng, HCIR_TOPK_MAX), ng < 2^31.
 * ------------------------------------------------------------------ */
#define HCIR_TOPK_MAX 1024
size_t hcir_sim_topk_workspace_bytes(int64_t nq, int64_t ng, int32_t d, int32_t k,
                                     int dtype);
int hcir_sim_topk(const void* q, int64_t nq, const void* g, int64_t ng, int32_t d,
                  int32_t k, int dtype, const float* q_inv_norm,
                  const float* g_inv_norm, int64_t idx_base, float* out_val,
                  int64_t* out_idx, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Exact re-scoring + certification of a candidate list ("exact by verification" search,
 * DESIGN.md §3 "filtered search"; no reference equivalent).  cand_idx/cand_val [nq][kc] come from
 * hcir_sim_topk on a reduced-precision MIRROR of the gallery (kc <= 64, sorted).  Every candidate is
 * re-scored against the fp32 gallery `g` with the HCIR_F32 fmaf chain (bit-identical to
 * hcir_sim_topk(HCIR_F32)), ranked (score desc, index asc) into out_val/out_idx [nq][k], and
 * certified[i] = 1 iff  cand_val[i][kc-1] + err_bound[i] < exact k-th score, i.e. no row outside
 * the candidate set can belong to the exact top-k, given |exact - mirror score| <= err_bound[i].
 * err_bound is a device array [nq], or NULL: then E_i is computed in the kernel from the HOST array
 * mirror_consts = {max_j ||g_j - g~_j||, max_j ||g~_j||, max_j ||g_j||, gamma_d} of an fp16 mirror
 * (derivation: hcir/gallery.py).  The mirror is fp16 and nothing else: the kernel takes ||q - q~||
 * from an fp16 rounding of q, so with a bf16 mirror E_i would not be a bound.  The caller re-runs
 * uncertified queries through hcir_sim_topk(HCIR_F32).
 * Pinned by tests/test_refine_gpu.py against oracle/refine.py, bit for bit:
 *   - candidate indices are TRUSTED: an index >= 0 must satisfy idx_base <= index < idx_base + ng
 *     (ng itself is not used, no range check is made); an index < 0 is an empty slot;
 *   - g_inv_norm is indexed by index - idx_base, q_inv_norm by the query;
 *   - a candidate whose score is NaN never ranks: it is dropped like an empty slot;
 *   - equal scores rank by index ascending;
 *   - with v valid candidates, v < k, slots [v, k) hold -inf / -1;
 *   - certified[i] = 1 when cand_idx[i][kc-1] < 0 (the filter returned every row it has);
 *     otherwise k valid candidates must exist and fl32(cand_val[i][kc-1] + E_i) < the k-th score,
 *     strictly: equality is not certified, and a NaN or infinite E_i certifies nothing.
 * Returns HCIR_ERR_INVALID, before any launch, for d % 8 != 0, kc > 64, k > kc, nq <= 0, or
 * err_bound and mirror_consts both NULL. */
int hcir_topk_refine_f32(const float* q, int64_t nq, const float* g, int64_t ng, int32_t d,
                         const int64_t* cand_idx, const float* cand_val, int32_t kc, int32_t k,
                         int64_t idx_base, const float* q_inv_norm, const float* g_inv_norm,
                         const float* err_bound, const float* mirror_consts, float* out_val,
                         int64_t* out_idx, int32_t* certified, void* stream);

/* Merge `nlists` sorted top-k lists per query into one top-k_out list.
 * vals/idx layout: [nlists][nq][k_in].  Used for the per-shard merge after the
 * RCCL all-gather (no reference equivalent: the reference is single-GPU,
 * SURVEY.md §2.3) and internally by hcir_sim_topk.  Entries with idx < 0 are
 * empty slots. */
int hcir_topk_merge(const float* vals, const int64_t* idx, int32_t nlists, int64_t nq,
                    int32_t k_in, int32_t k_out, float* out_val, int64_t* out_idx,
                    void* stream);

/* ------------------------------------------------------------------ *
 * NT-Xent forward (lightly.loss.NTXentLoss semantics; call site
 * HP/src/pretrain_engine.py:93,725; in-tree restatement
 * experiments/DualViewHair/src/losses/ntxent_loss.py:30-57).
 *   z = [normalize(z0); normalize(z1)]  (2B x D),  logits = z z^T * inv_t,
 *   diagonal removed, positive of row i is (i + B) mod 2B,
 *   loss = mean_i ( logsumexp_{j != i} logits[i][j] - logits[i][pos(i)] ).
 * Outputs: loss (1 float), row_lse[2B] (saved for a backward pass, may be NULL).
 * The 2B x 2B logits are never materialised.  d % 8 == 0.
 * Status: HCIR_ERR_INVALID for a null z0/z1/loss, b <= 0, d <= 0, d % 8 != 0, inv_t == 0 or NaN;
 * HCIR_ERR_UNSUPPORTED for a dtype other than HCIR_F32/F16/BF16; HCIR_ERR_WORKSPACE for a null or short
 * workspace.  Nothing is written on an error.
 * ------------------------------------------------------------------ */
size_t hcir_ntxent_workspace_bytes(int64_t b, int32_t d, int dtype);
int hcir_ntxent_fwd(const void* z0, const void* z1, int64_t b, int32_t d, int dtype,
                    float inv_t, float* loss, float* row_lse, void* workspace,
                    size_t workspace_bytes, void* stream);

/* NT-Xent backward: dL/dz0, dL/dz1 (same dtype as the inputs) for the loss of hcir_ntxent_fwd.
 *   G = (P - Y)/2B,  dU = (1/T)(G + G^T) U,  dz_i = grad_out * (dU_i - (dU_i.u_i) u_i) / ||z_i||
 * W = P + P^T - 2Y is written once as fp16 [2B][2B] into the workspace and dU = W.U runs on
 * hcir_gemm_f16 (fp16 MFMA: gradients carry fp16-level relative error for every input dtype).
 * row_lse: the [2B] vector saved by hcir_ntxent_fwd.  Requirements: d % 8 == 0, b % 4 == 0.
 * Statuses as hcir_ntxent_fwd (a null row_lse/dz0/dz1 and b % 4 != 0 are HCIR_ERR_INVALID too). */
size_t hcir_ntxent_bwd_workspace_bytes(int64_t b, int32_t d, int dtype);
int hcir_ntxent_bwd(const void* z0, const void* z1, int64_t b, int32_t d, int dtype, float inv_t,
                    const float* row_lse, float grad_out, void* dz0, void* dz1, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * Supervised contrastive loss (SupConLoss, HairPretraining/utils/losses.py:8-101, contrast_mode 'all';
 * the simclr_supcon step, HairPretraining/src/pretrain_engine.py:76,390).
 *   feat [B][V][D];  row r = v*B + i is view v of sample i,  N = V*B;  y_r = labels[r mod B]
 *   (labels NULL: y_r = r mod B, the SimCLR case);  x_r = the row, or row / max(||row||, 1e-12) with normalize;
 *   s_ij = x_i.x_j * inv_t;  lse_i = log sum_{j != i} exp(s_ij);  m_ij = [y_i == y_j, j != i],  n_i = sum_j m_ij;
 *   loss = mean_i t_over_base [n_i > 0] (lse_i - sum_j m_ij s_ij / max(n_i, 1)),  t_over_base = T / T_base.
 * A row without positives contributes 0 and still counts in the mean.  V = 2, labels NULL, normalize and
 * t_over_base = 1 is hcir_ntxent_fwd's loss.  Outputs: loss (1 float), row_lse[N] and row_npos[N] (saved for the
 * backward, either may be NULL).  Labels are compared as 64-bit integers.  The N x N logits are never materialised;
 * no atomics, results are bit-identical from run to run.
 * Backward: p_ij = exp(s_ij - lse_i), G_ij = [n_i > 0](p_ij - m_ij / n_i), W = G + G^T written once as fp16 [N][N]
 * into the workspace, g = W.x on hcir_gemm_f16, dfeat = grad_out * inv_base / N * g (inv_base = 1 / T_base), through
 * the projection rn_i (g_i - (g_i.u_i) u_i) with normalize; dfeat is [B][V][D] in the input dtype.
 * hcir_supcon_workspace_bytes(..., backward): bytes for the forward (0) or the backward (1).
 * Status: HCIR_ERR_INVALID for a null feat/loss (backward: feat/row_lse/row_npos/dfeat), b, v, d <= 0, N < 2,
 * d % 8 != 0, inv_t == 0 or NaN, and for a backward with N % 8 != 0 (hcir_gemm_f16's rule); HCIR_ERR_UNSUPPORTED for a
 * dtype other than HCIR_F32/F16/BF16; HCIR_ERR_WORKSPACE for a null or short workspace.  Nothing is written on an error.
 * ------------------------------------------------------------------ */
size_t hcir_supcon_workspace_bytes(int64_t b, int32_t v, int32_t d, int dtype, int backward);
int hcir_supcon_fwd(const void* feat, const int64_t* labels, int64_t b, int32_t v, int32_t d, int dtype,
                    float inv_t, float t_over_base, int normalize, float* loss, float* row_lse,
                    int32_t* row_npos, void* workspace, size_t workspace_bytes, void* stream);
int hcir_supcon_bwd(const void* feat, const int64_t* labels, int64_t b, int32_t v, int32_t d, int dtype,
                    float inv_t, float inv_base, int normalize, const float* row_lse, const int32_t* row_npos,
                    float grad_out, void* dfeat, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * NT-Xent against a memory bank (lightly.loss.NTXentLoss(memory_bank_size=(K, D)); the two criteria of the DenseCL
 * step, HairPretraining/src/pretrain_engine.py:85-87,309-312).
 *   q_i = z0_i / max(||z0_i||, 1e-12),  k_i = z1_i / max(||z1_i||, 1e-12)                   i < N
 *   logits_i = [ q_i.k_i , q_i.bank_0 , ... , q_i.bank_{K-1} ] * inv_t      bank rows as stored, not renormalised
 *   loss = mean_i ( logsumexp(logits_i) - logits_i[0] )
 * z0, z1 [N][D] in dtype; bank fp32 [K][D].  Outputs: loss (1 float); row_lse[N] and row_pos[N] (the positive logit),
 * saved for the backward, either may be NULL; k_unit fp32 [N][D] (may be NULL): the normalised key rows, which are
 * what a caller enqueues into the bank.  The N x (K + 1) logits are never materialised; no atomics, results are
 * bit-identical from run to run.
 * Backward: p_ij = exp(logit_ij - lse_i) (j = 0 the positive),
 *   dq_i = grad_out * inv_t / N * (sum_j p_ij bank_j + (p_i0 - 1) k_i),  dk_i = grad_out * inv_t / N * (p_i0 - 1) q_i,
 * through the normalisation's projection rn_i (g_i - (g_i.u_i) u_i); P is written once as fp16 [N][K] into the
 * workspace and P.bank runs on hcir_gemm_f16.  dz1 may be NULL (a key without gradient): its work is skipped and dz0
 * is the same bits.  The bank receives no gradient.
 * hcir_ntxent_bank_workspace_bytes(..., backward): bytes for the forward (0) or the backward (1).
 * Status: HCIR_ERR_INVALID for a null z0/z1/bank/loss (backward: z0/z1/bank/row_lse/row_pos/dz0), n, k, d <= 0,
 * d % 8 != 0, n > 65535 * 128, inv_t == 0 or NaN, and for a backward with k % 8 != 0 (hcir_gemm_f16's rule for its
 * inner dimension, which is the bank here; n is the GEMM's row count and is free); HCIR_ERR_UNSUPPORTED for a dtype other than HCIR_F32/F16/BF16; HCIR_ERR_WORKSPACE for a null or short
 * workspace.  Nothing is written on an error.
 * ------------------------------------------------------------------ */
size_t hcir_ntxent_bank_workspace_bytes(int64_t n, int64_t k, int32_t d, int dtype, int backward);
int hcir_ntxent_bank_fwd(const void* z0, const void* z1, const float* bank, int64_t n, int64_t k, int32_t d, int dtype,
                         float inv_t, float* loss, float* row_lse, float* row_pos, float* k_unit, void* workspace,
                         size_t workspace_bytes, void* stream);
int hcir_ntxent_bank_bwd(const void* z0, const void* z1, const float* bank, int64_t n, int64_t k, int32_t d, int dtype,
                         float inv_t, const float* row_lse, const float* row_pos, float grad_out, void* dz0, void* dz1,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * MSN criterion (lightly.loss.MSNLoss; the MSN step, HairPretraining/src/pretrain_engine.py:242-275).  Row i of the
 * anchors pairs with target i mod B; N % B == 0.
 *   a_i = anchors_i / max(||anchors_i||, 1e-12), t_j and c_k (prototypes) likewise
 *   p_ik = softmax_k(a_i.c_k * inv_t)
 *   q_jk = softmax_k(t_j.c_k * inv_t_sharp)        inv_t_sharp = 1 / (T * Ts): softmax(./T) ** (1/Ts), renormalised
 *   Sinkhorn (iterations > 0): v = 1; repeat u_k = 1 / (K sum_j q_jk v_j), v_j = 1 / (B sum_k u_k q_jk);
 *                              q_jk <- u_k q_jk / sum_k u_k q_jk
 *   loss = mean_i sum_k -q_(i mod B)k log p_ik + reg_weight * (sum_k pbar_k log pbar_k + log K),  pbar_k = mean_i p_ik
 * hcir_msn_targets: targets [B][D] in dtype, prototypes fp32 [K][D] (normalised here, not by the caller) -> q fp32
 * [B][K]; iterations == 0 leaves the sharpened softmax.
 * hcir_msn_fwd: anchors [N][D] in dtype -> loss (1 float); loss_parts[2] = {cross-entropy, regulariser without its
 * weight}, row_lse[N], pbar[K]: each may be NULL; the backward needs row_lse and pbar.  No [N][K] matrix is stored.
 * hcir_msn_bwd: G_ik = p_ik (sum_k q_ik + reg_weight (log pbar_k - e_i)) - q_ik, e_i = sum_k p_ik log pbar_k, written
 * once as fp16 [N][K] into the workspace (1 / N and grad_out stay out of that image); g = G.c on hcir_gemm_f16;
 * danchors_i = grad_out * inv_t / N * rn_i (g_i - (g_i.a_i) a_i), [N][D] in dtype.  The targets and the prototypes
 * receive no gradient.
 * No atomics, every sum in a fixed order: results are bit-identical from run to run.
 * hcir_msn_workspace_bytes(n, k, d, dtype, stage): stage 0 = targets (n is B), 1 = forward, 2 = backward.
 * Status: HCIR_ERR_INVALID for a null required pointer, n, b, k, d <= 0, d % 8 != 0, n % b != 0, n > 65535 * 128,
 * a temperature factor that is 0 or NaN, iterations < 0, and for a backward with k % 8 != 0 (hcir_gemm_f16's rule for
 * its inner dimension); HCIR_ERR_UNSUPPORTED for a dtype other than HCIR_F32/F16/BF16; HCIR_ERR_WORKSPACE for a null
 * or short workspace.  Nothing is written on an error.
 * ------------------------------------------------------------------ */
size_t hcir_msn_workspace_bytes(int64_t n, int64_t k, int32_t d, int dtype, int stage);
int hcir_msn_targets(const void* targets, const float* prototypes, int64_t b, int64_t k, int32_t d, int dtype,
                     float inv_t_sharp, int32_t iterations, float* q, void* workspace, size_t workspace_bytes,
                     void* stream);
int hcir_msn_fwd(const void* anchors, const float* prototypes, const float* q, int64_t n, int64_t b, int64_t k,
                 int32_t d, int dtype, float inv_t, float reg_weight, float* loss, float* loss_parts, float* row_lse,
                 float* pbar, void* workspace, size_t workspace_bytes, void* stream);
int hcir_msn_bwd(const void* anchors, const float* prototypes, const float* q, int64_t n, int64_t b, int64_t k,
                 int32_t d, int dtype, float inv_t, float reg_weight, const float* row_lse, const float* pbar,
                 float grad_out, void* danchors, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * Dense matching (lightly.models.utils.select_most_similar; the DenseCL step,
 * HairPretraining/src/pretrain_engine.py:304-306).  For image b and query position n:
 *   j*(b, n) = argmax_m (x_bn . y_bm) / max(||y_bm||, 1e-12),   out[b][n] = y_values[b][j*(b, n)]
 * x's own norm is a positive row constant and is not computed; a zero x row takes index 0.  On exact ties of the fp32
 * scores the lowest m wins (torch.argmax).  x [B][N][C] and y [B][M][C] fp16 (a trunk's NHWC maps as they stand);
 * y_values [B][M][Dv] in values_dtype (HCIR_F16 | HCIR_F32), may be NULL; idx int32 [B][N] is always written, out
 * [B][N][Dv] in values_dtype when y_values is given.  Workspace: hcir_dense_match_workspace_bytes(b, m).
 * Status: HCIR_ERR_INVALID for a null x/y/idx (or out with y_values), a size below 1, b > 65535;
 * HCIR_ERR_UNSUPPORTED for n or m > 256, c % 8 != 0, dv % 8 != 0 or another values_dtype; HCIR_ERR_WORKSPACE for a
 * null or short workspace.  Nothing is written on an error.
 * ------------------------------------------------------------------ */
size_t hcir_dense_match_workspace_bytes(int64_t b, int32_t m);
int hcir_dense_match_f16(const void* x, const void* y, const void* y_values, int values_dtype, int64_t b, int32_t n,
                         int32_t m, int32_t c, int32_t dv, int32_t* idx, void* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * ViT building blocks (fp16 MFMA, fp32 accumulate, fp32 residual stream).
 * ------------------------------------------------------------------ */

/* LayerNorm over the last dim of fp32 rows -> fp16 rows.
 * nn.LayerNorm(D, eps=1e-6)   torchvision EncoderBlock.ln_1/ln_2 (HP/src/main_backbone.py:554)
 *                             models_vit.LayerNorm (HP/src/models_vit.py:23-27) */
int hcir_layernorm_f16(const void* x, int x_dtype /* HCIR_F32 | HCIR_F16 residual stream */,
                       int64_t rows, int32_t d, int64_t ldx, const float* gamma, const float* beta,
                       float eps, void* y_f16, int64_t ldy, void* stream);

/* Epilogues of hcir_gemm_f16:  acc = A[M,K] . W[N,K]^T  (fp32 accumulate) */
typedef enum {
  HCIR_EPI_BIAS_F16 = 0,      /* out_f16 = acc + bias                      (qkv / in_proj)      */
  HCIR_EPI_BIAS_GELU_F16 = 1, /* out_f16 = gelu_erf(acc + bias)            (mlp fc1)            */
  HCIR_EPI_BIAS_RESID_F32 = 2,/* out_f32 += scale[n] * (acc + bias)        (attn proj, mlp fc2; */
                              /*   scale = LayerScale gamma or NULL)                            */
  HCIR_EPI_BIAS_F32 = 3,      /* out_f32 = acc + bias                                           */
  HCIR_EPI_AFFINE_RELU_F16 = 4,/* out_f16 = relu(acc * scale[n] + bias[n])  (proj-head Linear+BN+ReLU, eval) */
  HCIR_EPI_AFFINE_F32 = 5,    /* out_f32 = acc * scale[n] + bias[n]        (proj-head Linear+BN, eval)      */
  HCIR_EPI_BIAS_RESID_F16 = 6 /* out_f16 += scale[n] * (acc + bias)        (fp16 residual stream; the     */
                              /*   product term is formed in fp32 and rounded to fp16, the sum of the  */
                              /*   two fp16 numbers is rounded once)                                   */
} hcir_epilogue;

/* out[M,N] = epilogue(A[M,K] . W[N,K]^T).  A, W fp16 row-major (W is the
 * nn.Linear weight as stored).  Replaces nn.Linear / MultiheadAttention
 * in_proj / out_proj / MLPBlock / timm Mlp  (HP/src/models_vit.py:63,66,70,79;
 * HP/src/main_backbone.py:554 -> torchvision EncoderBlock).
 * Requirements: K % 8 == 0, N % 8 == 0; ldo >= N and a multiple of 4, of 8 for an fp16 output on the persistent
 * kernels (M >= 1024, N % 256 == 0, K % 64 == 0: rows are stored in 16-byte pieces); bias may be NULL.  lda / ldw are row pitches in
 * elements (>= K, multiples of 8); pitches other than K are carried by the persistent
 * 256 x 256 kernel only (M >= 1024, N % 256 == 0, K % 64 == 0), else HCIR_ERR_UNSUPPORTED. */
int hcir_gemm_f16(const void* a, int64_t lda, const void* w, int64_t ldw,
                  const float* bias, const float* scale, int64_t m, int32_t n,
                  int32_t k, int epilogue, void* out, int64_t ldo, void* stream);
/* The *_RESID_* epilogues out of place: out = resid + scale[n] * (acc + bias), resid [M, N] of out's type and row
 * pitch (the residual add of a Block, x = x + attn(...) / x + mlp(...), HP/src/models_vit.py:147-149, when the
 * block's input must survive - the training forward keeps it for the backward).  resid NULL or == out: in place,
 * i.e. hcir_gemm_f16.  Any other epilogue with resid != NULL: HCIR_ERR_INVALID. */
int hcir_gemm_f16_resid(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                        const float* scale, int64_t m, int32_t n, int32_t k, int epilogue, const void* resid,
                        void* out, int64_t ldo, void* stream);

/* fc1 of the TRAINING forward: out_pre = fp16(acc + bias) (the pre-activation the GELU backward needs) and
 * out_act = fp16(gelu(acc + bias)) (the next GEMM's operand) from one pass over the accumulators - the value is
 * formed once in fp32 and rounded twice - instead of a GEMM plus an hcir_gelu_fwd_f16 pass over M x N.
 * (MLPBlock / timm Mlp fc1 + act, HP/src/main_backbone.py:554; HP/src/models_vit.py:19.)  Both outputs fp16 with row
 * pitch ldo.  Persistent kernel only: HCIR_ERR_UNSUPPORTED unless hcir_gemm_fused_supported(m, n, k). */
int hcir_gemm_f16_gelu_dual(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m,
                            int32_t n, int32_t k, void* out_pre, void* out_act, int64_t ldo, void* stream);

/* LayerNorm fused into the GEMMs on either side of it (persistent 256 x 256 kernel only:
 * hcir_gemm_fused_supported(m, n, k) != 0, i.e. M >= 1024, N % 256 == 0, K % 64 == 0).
 * Replaces the  x -> norm1/ln_1 -> qkv   and   x -> norm2/ln_2 -> fc1   pairs of a Block
 * (HP/src/models_vit.py:147-149; torchvision EncoderBlock via HP/src/main_backbone.py:554)
 * without ever writing the normalised tokens:
 *  (1) producer: epilogue HCIR_EPI_BIAS_RESID_F16 with stats_part != NULL also writes, per
 *      stored fp16 row, one (mean, sum of squared deviations from it) pair per 64-feature slice:
 *          stats_part[slice][row][2],  slice < hcir_gemm_stats_slices(n) = n / 64;
 *  (2) hcir_ln_stats_finalize combines the slices (Chan's parallel-variance formula, index order:
 *      deterministic, no E[x^2] - mean^2 cancellation) and writes
 *          ln_stats[row] = (mean, 1 / sqrt(var + eps)),  var biased (/ n_features = 64 * slices);
 *  (3) consumer: epilogue HCIR_EPI_BIAS_F16 / HCIR_EPI_BIAS_GELU_F16 with ln_stats, ln_c1:
 *      A = the RAW residual rows x (fp16), W' = fp16(gamma o W),
 *          out = act( rstd[m] * (A . W'^T - mean[m] * ln_c1[n]) + bias[n] )
 *      where the caller prepares  ln_c1[n] = sum_k W'[n][k]  (of the ROUNDED fp16 values) and
 *      bias[n] = sum_k beta[k] * W[n][k] + b[n]:  algebraically LayerNorm(x) . W^T + b.
 * Exactly one of {ln_stats + ln_c1, stats_part} must be given.  scale as in hcir_gemm_f16. */
int hcir_gemm_fused_supported(int64_t m, int32_t n, int32_t k);
int32_t hcir_gemm_stats_slices(int32_t n);
/* Which kernel hcir_gemm_f16 / _resid / _fused (epilogue: an hcir_epilogue value) or hcir_gemm_f16_gelu_dual
 * (epilogue: HCIR_GEMM_ROUTE_EPI_DUAL) takes for an M x N x K problem; host arithmetic only, nothing is launched:
 *   SMALL  the 128 x 128 kernel (also every shape the fused and dual calls refuse);
 *   MID    the whole launch on the persistent 128 x 192 kernel;
 *   BIG    the whole launch on the persistent 256 x 256 kernel (256 workgroups; more tiles: several per workgroup);
 *   SPLIT  rows [0, *rows_on_big) on the 256 x 256 kernel, the rest as a second launch on the 128 x 192 kernel.
 * *rows_on_big (may be NULL) receives the rows the 256 x 256 kernel computes: M on BIG, 0 on SMALL and MID.
 * Returns the route, or HCIR_ERR_INVALID (m, n, k < 1, n or k no multiple of 8, unknown epilogue). */
typedef enum {
  HCIR_GEMM_ROUTE_SMALL = 0,
  HCIR_GEMM_ROUTE_MID = 1,
  HCIR_GEMM_ROUTE_BIG = 2,
  HCIR_GEMM_ROUTE_SPLIT = 3
} hcir_gemm_route_kind;
#define HCIR_GEMM_ROUTE_EPI_DUAL 10
int hcir_gemm_route(int64_t m, int32_t n, int32_t k, int epilogue, int64_t* rows_on_big);
int hcir_gemm_f16_fused(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                        const float* scale, int64_t m, int32_t n, int32_t k, int epilogue,
                        void* out, int64_t ldo, const float* ln_stats, const float* ln_c1,
                        float* stats_part, void* stream);
/* The LayerNorm-folded HCIR_EPI_BIAS_F16 form of hcir_gemm_f16_fused for ANY number of rows m >= 1 (a few rows picked
 * out of a larger matrix by their pitch lda - the class-token rows of the last ViT block), always on the persistent
 * 128 x 192 kernel: the same k order and epilogue arithmetic as the 256 x 256 kernel, so row r of this call holds the
 * bits that row would have in a hcir_gemm_f16_fused launch over the whole matrix.  ln_stats [m][2] belongs to the m
 * rows of THIS call.  K % 64 == 0 and N % 128 == 0, else HCIR_ERR_UNSUPPORTED. */
int hcir_gemm_f16_ln_rows(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t m,
                          int32_t n, int32_t k, void* out, int64_t ldo, const float* ln_stats,
                          const float* ln_c1, void* stream);
int hcir_ln_stats_finalize(const float* stats_part, int32_t slices, int64_t m, int32_t n_features,
                           float eps, float* ln_stats, void* stream);

/* Patch embedding = Conv2d(C, D, kernel=P, stride=P) as an im2col-free MFMA GEMM
 * over the fp32 NCHW image, fused with bias, class token and positional add:
 *   tok[b][0]     = cls + pos_mult * pos[0]
 *   tok[b][1 + p] = W . patch(b,p) + bias + pos_mult * pos[1 + p]
 * (HP/src/main_backbone.py:543-551 with pos_mult = 2, see DESIGN.md "double
 *  positional add"; HP/src/models_vit.py:42,48,229-233 with pos_mult = 1).
 * img fp32 [B][C][H][W]; w fp16 [D][ldw], row = the C*P*P weights of one output feature in
 * (c, ky, kx) order, zero-padded to ldw (a multiple of 64); tok [B][1 + (H/P)(W/P)][D] in
 * tok_dtype (HCIR_F32 or HCIR_F16: the residual-stream storage type).  Any patch size P <= 32
 * (P == 16 takes a vectorised path). */
int hcir_patch_embed(const float* img, int64_t b, int32_t c, int32_t h, int32_t w_px,
                     int32_t p, const void* w_f16, int64_t ldw, const float* bias,
                     const float* cls, const float* pos, float pos_mult, int32_t d, void* tok,
                     int tok_dtype, void* stream);
/* The same patch embedding on the persistent 256 x 256 tile engine of hcir_gemm_f16 (weights by LDS-DMA, the image
 * gathered and converted once per 256-feature n-tile), for P == 16, tok_dtype == HCIR_F16, d % 256 == 0 and
 * ldw == c * 256; every other shape returns HCIR_ERR_UNSUPPORTED with tok untouched (use hcir_patch_embed).
 * tok: same contract as hcir_patch_embed (fp32 sum, one rounding to fp16).  stats_part (may be NULL): for EVERY
 * token row, class-token rows included, the (mean, sum of squared deviations from it) of each 64-feature slice of
 * the fp16 values as stored, [d / 64][b * T][2] - the producer side of the LayerNorm fold, read by
 * hcir_ln_stats_finalize with m = b * T.
 * hcir_patch_embed_route: which of the two a shape takes; host arithmetic only, nothing is launched.  Returns the
 * route, or HCIR_ERR_INVALID (a size < 1, image sides no multiple of p). */
typedef enum {
  HCIR_PATCH_ROUTE_TILE128 = 0, /* hcir_patch_embed: 128 x 128 tiles, both operands staged through registers */
  HCIR_PATCH_ROUTE_BIG = 1      /* hcir_patch_embed_fused: persistent 256 x 256 tiles */
} hcir_patch_route_kind;
int hcir_patch_embed_route(int64_t b, int32_t c, int32_t h, int32_t w_px, int32_t p, int32_t d, int64_t ldw,
                           int tok_dtype);
int hcir_patch_embed_fused(const float* img, int64_t b, int32_t c, int32_t h, int32_t w_px,
                           int32_t p, const void* w_f16, int64_t ldw, const float* bias,
                           const float* cls, const float* pos, float pos_mult, int32_t d, void* tok,
                           int tok_dtype, float* stats_part, void* stream);

/* Fused multi-head self-attention forward over packed qkv:
 *   qkv fp16 [B][T][3][H][hd]  (rows of the in_proj / qkv GEMM),
 *   out fp16 [B][nq][H*hd] = softmax((q * scale) k^T) v   per (b, head), for the FIRST nq query
 *   rows of every image (nq = T: all tokens; nq = 1: the class token only, which is all the last
 *   block of an embedding forward needs).
 * K and V of one (b, head) are LDS-resident; QK^T and PV are MFMA 32x32x16
 * tiles; softmax stays in registers.  (HP/src/models_vit.py:69-78;
 * nn.MultiheadAttention inside torchvision EncoderBlock, HP/src/main_backbone.py:554.)
 * Requirements: T <= 288; hd == 64 runs the tuned kernel, hd in {32, 48, 80, 96, 128} (vit_huge_patch14: 80,
 * HP/src/models_vit.py:266-270) a generic one with unswizzled, register-staged LDS images. */
int hcir_attn_fwd(const void* qkv, int64_t b, int32_t t, int32_t h, int32_t hd,
                  float scale, int32_t nq, void* out, void* stream);

/* Final step of extract_features for the CLS token:
 *   e = ln ? LayerNorm(tok[b][0]) : tok[b][0];  optionally L2-normalised.
 * (torchvision Encoder.ln + x[:,0]  HP/src/main_backbone.py:554,557;
 *  F.normalize  HP/src/classification_engine.py:50.)
 * emb_f32 [B][D]; emb_f16 optional. */
int hcir_cls_head(const void* tok, int tok_dtype, int64_t b, int32_t t, int32_t d,
                  const float* gamma, const float* beta, float eps, int l2_normalize,
                  float* emb_f32, void* emb_f16, void* stream);

/* Mean over patch tokens 1..T-1 after the optional final LayerNorm
 * (pooled_patches of ViTWrapper.forward, HP/src/main_backbone.py:558-561). */
int hcir_patch_mean(const void* tok, int tok_dtype, int64_t b, int32_t t, int32_t d,
                    const float* gamma, const float* beta, float eps, float* out_f32,
                    void* stream);

/* knn_transform on the device (HP/utils/transform.py:10-14): CenterCrop(size) -> ToTensor ->
 * Normalize(mean, std) of a batch of decoded RGB8 images of one size, img [B][H][W][3] uint8 (device)
 * -> out [B][3][size][size] fp32.  Bit-exact with torchvision's arithmetic (u8 / 255, (x - mean) / std,
 * IEEE fp32); images smaller than the window are zero-padded as CenterCrop does.  mean3 / std3 are
 * HOST pointers to 3 floats. */
int hcir_knn_transform_u8(const uint8_t* img, int64_t b, int32_t h, int32_t w, int32_t size,
                          const float* mean3, const float* std3, float* out, void* stream);

/* EMA update of the momentum encoder, every parameter tensor in ONE launch:
 *     ema = ema * m + p * one_minus_m        (fp32, two rounded multiplies + one rounded add: bit-exact with
 *                                             lightly's update_momentum, HP/src/pretrain_engine.py:618-619)
 * dst_ptrs / src_ptrs / counts are DEVICE arrays of n_chunks entries: chunk c covers counts[c] consecutive
 * floats at address dst_ptrs[c] (ema) and src_ptrs[c] (online parameters).  The caller builds the table once
 * per model pair (hcir.momentum) and splits big tensors into chunks of its choice. */
int hcir_ema_update(const uint64_t* dst_ptrs, const uint64_t* src_ptrs, const int64_t* counts,
                    int64_t n_chunks, float m, float one_minus_m, void* stream);

/* ------------------------------------------------------------------ *
 * The optimizer tail of the training step on the device, with no host read:
 *     scaler.unscale_(opt); clip_grad_norm_(params, max_norm); scaler.step(opt); scaler.update()
 *                                                              (HP/src/pretrain_engine.py:746-749)
 * for torch.optim.Adam with coupled L2 weight decay and per-group weight_decay / lr, as built by get_optimizer
 * (HP/utils/utils.py:59-71, called at HP/src/pretrain_engine.py:108).  Three launches over a chunk table in DEVICE
 * memory (hcir.optim builds and caches it): chunk c covers counts[c] (1 .. 65 536) consecutive floats of ONE
 * parameter at p_ptrs[c] / g_ptrs[c] / m_ptrs[c] (exp_avg) / v_ptrs[c] (exp_avg_sq); param_idx[c] is that
 * parameter's index into steps / step_size / bc2_sqrt and weight_decay[c] its group's weight decay.  16-byte
 * accesses where a chunk's pointers are 16-byte aligned, 4-byte accesses otherwise.  No atomics; two calls on the
 * same inputs give the same bits.  fp contraction is off: every product and sum is rounded on its own.
 * The GRADIENT BUFFERS ARE NEVER WRITTEN: after the step they still hold what backward() left, scaled and unclipped.
 *
 * ctl is 4 device floats written by hcir_optim_finalize and read by hcir_adam_step:
 *     ctl[0] total_norm   ctl[1] c = inv_scale * clip_coef   ctl[2] found_inf (0 / 1)   ctl[3] clip_coef
 * ------------------------------------------------------------------ */

/* scaler.unscale_ + the norm half of clip_grad_norm_ (:746-747): partial[c] = sum over chunk c of
 * (g * inv_scale)^2 in fp32, flags[c] = 1 if some g * inv_scale of the chunk is inf or NaN, else 0; plain stores,
 * one slot per chunk.  inv_scale = float(1 / double(scale[0])) read from DEVICE memory (GradScaler._scale);
 * scale == NULL means 1. */
int hcir_grad_sumsq(const uint64_t* g_ptrs, const int64_t* counts, int64_t n_chunks, const float* scale,
                    float* partial, int32_t* flags, void* stream);

/* One workgroup: sum = partial[0 .. n_chunks) added in fp64 in a fixed order; total_norm = sqrt(sum);
 * clip_coef = use_clip ? min(1, max_norm / (total_norm + 1e-6)) : 1 (clip_grad_norm_, :747; a NaN stays a NaN);
 * found_inf = scale != NULL and some flag is set (without a scaler the step is unconditional, as in the reference's
 * else branch :750-751).  With a scaler, GradScaler.update (:749): on found_inf scale *= backoff_factor and the
 * tracker is reset; otherwise the tracker is incremented and, when it reaches growth_interval, scale *= growth_factor
 * (kept if that overflows) and the tracker is reset.  If not found_inf, for each of the n_part participating
 * parameters i = part_idx[j]: steps[i] += 1, step_size[i] = lr / (1 - beta1^step), bc2_sqrt[i] =
 * sqrt(1 - beta2^step), both computed in double and rounded to fp32.  Participating parameters [group_end[g-1],
 * group_end[g]) take group_lr[g]; group_end / group_lr are HOST arrays of n_groups (<= 16) entries, group_end
 * ascending and ending at n_part.  n_chunks may be 0 (a plain step: no norm, no scaler); partial / flags may then
 * be NULL.  scale and growth_tracker are both NULL or both set. */
int hcir_optim_finalize(const float* partial, const int32_t* flags, int64_t n_chunks, float* scale,
                        int32_t* growth_tracker, float growth_factor, float backoff_factor,
                        int32_t growth_interval, int use_clip, double max_norm, const int32_t* group_end,
                        const double* group_lr, int32_t n_groups, double beta1, double beta2,
                        const int32_t* part_idx, int32_t n_part, float* steps, float* step_size,
                        float* bc2_sqrt, float* ctl, void* stream);

/* scaler.step(opt) (:748) = torch.optim.Adam.step on the unscaled, clipped gradient.  Per chunk, nothing is written
 * if ctl[2] (found_inf) is set; otherwise per element, in fp32, each operation rounded on its own:
 *     g = grad * c + wd * p;   m = m + (g - m) * one_minus_beta1;   v = v * beta2 + one_minus_beta2 * (g * g)
 *     p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps))
 * p, m and v are written; grad is only read. */
int hcir_adam_step(const uint64_t* p_ptrs, const uint64_t* g_ptrs, const uint64_t* m_ptrs,
                   const uint64_t* v_ptrs, const int64_t* counts, const int32_t* param_idx,
                   const float* weight_decay, int64_t n_chunks, const float* step_size,
                   const float* bc2_sqrt, const float* ctl, float beta2, float one_minus_beta1,
                   float one_minus_beta2, float eps, void* stream);

/* PositiveMaskingTransform on the device (HP/utils/transform.py:84-150; the masked positive view of the
 * pretrain step, HP/src/pretrain_engine.py:692-694).  images/out fp32 [B][C][H][W] (may not alias).  A patch
 * (patch x patch, non-overlapping grid) is a "hair" patch when its mean over (C, patch, patch) > threshold;
 * per image int(n_hair * u[b]) hair patches — those with the smallest keys[b][patch] (ties: smaller patch
 * index) — are zeroed.  u [B] and keys [B][(H/patch)*(W/patch)] are DEVICE arrays of the caller's random
 * numbers (u ~ U(mask_ratio_range), keys ~ U(0,1): the reference's uniform_ + randperm as data).
 * n_masked [B] (optional) receives the number of zeroed patches. */
int hcir_positive_masking(const float* images, int64_t b, int32_t c, int32_t h, int32_t w, int32_t patch,
                          float threshold, const float* u, const float* keys, float* out,
                          int32_t* n_masked, void* stream);

/* ------------------------------------------------------------------ *
 * What the reference does with the top-k list, on the device.
 * `ks` is a HOST array of nk <= 16 strictly ascending values, each in [1, kmax].
 * ------------------------------------------------------------------ */

/* KNeighborsClassifier(n_neighbors=k, metric="cosine").predict for EVERY k of the sweep from ONE
 * top-kmax neighbour list (HP/src/classification_engine.py:71,79-82 re-fits and re-scans per k):
 * uniform-weight mode of the first k neighbour labels, smallest label on ties (scipy.stats.mode as sklearn
 * uses it).  nbr_idx [nq][kmax] as written by hcir_sim_topk (idx_base is subtracted), labels [nlabels] in
 * [0, nclass), nclass <= 16384; pred [nk][nq].  *bad (device int, zeroed by the caller) is set when a
 * neighbour slot is empty or a label is out of range. */
int hcir_knn_vote(const int64_t* nbr_idx, int64_t nq, int32_t kmax, int64_t idx_base, const int64_t* labels,
                  int64_t nlabels, int32_t nclass, const int32_t* ks, int32_t nk, int64_t* pred, int32_t* bad,
                  void* stream);

/* sklearn confusion_matrix counts (HP/src/classification_engine.py:85): cm[t][p] += 1 over n samples;
 * cm [nclass][nclass] int32 zeroed by the caller; accuracy_score (:83) is its trace / n. */
int hcir_confusion_matrix(const int64_t* y_true, const int64_t* y_pred, int64_t n, int32_t nclass, int32_t* cm,
                          int32_t* bad, void* stream);

/* Linear probe: LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial").fit
 * (HP/src/classification_engine.py:107-110).  One evaluation of the objective the solver minimises, without its
 * penalty term (the caller adds 0.5 * ||w||^2 and + w):
 *   z = x w^T + b,   *loss = sum_i ( logsumexp_c z_ic - z_i,labels[i] )   (fp64),
 *   gw [c][d] = (P - Y)^T x,   gb [c] = colsum(P - Y),   P = softmax(z) (never written to memory).
 * x [n][ldx] fp32 (16-byte aligned, ldx % 4 == 0), labels [n] in [0, c), w [c][d], b [c]; d % 8 == 0,
 * 2 <= c <= 1024 (larger: HCIR_ERR_UNSUPPORTED).  A class without rows is legal.  *bad (device int, zeroed by the
 * caller) is set when a label is out of range; such a row is left out.  Operands stay fp32
 * (v_mfma_f32_32x32x2_f32); per-workgroup partials are added in a fixed order, so two calls with the same inputs
 * return the same bits.  workspace: hcir_softmax_xent_workspace_bytes (HOST; 0 for a shape the kernel rejects). */
size_t hcir_softmax_xent_workspace_bytes(int64_t n, int32_t d, int32_t c);
int hcir_softmax_xent_fwd_bwd(const float* x, int64_t n, int32_t d, int64_t ldx, const int64_t* labels,
                              const float* w, const float* b, int32_t c, double* loss, float* gw, float* gb,
                              int32_t* bad, void* workspace, size_t workspace_bytes, void* stream);

/* LogisticRegression.predict / decision_function (HP/src/classification_engine.py:111): pred[i] = arg-max over c of
 * z_ic = <x_i, w_c> + b_c, the FIRST maximum on exact ties (np.argmax); logits [n][c] fp32 is optional (NULL).
 * Same shape limits as hcir_softmax_xent_fwd_bwd. */
int hcir_linear_argmax(const float* x, int64_t n, int32_t d, int64_t ldx, const float* w, const float* b, int32_t c,
                       int64_t* pred, float* logits, void* stream);

/* Intra/inter-class variance (HP/src/classification_engine.py:241-262), two passes with fp64 accumulators.
 * Pass 1, hcir_class_sums_f64: counts [c] = rows of each class, sums [c][d] = their column sums; the class means
 * (:251) and the global mean (:244) follow from them.  Pass 2, hcir_class_scatter_f64: scatter [c] =
 * sum over the rows of class c of ||x_i - means[c]||^2 (:254) with means [c][d] read in fp64.  (The one-pass form
 * sum ||x||^2 / n - ||m||^2 cancels on unit-norm rows.)  Every sum runs in a fixed order.  labels [n] in [0, c);
 * *bad (device int, zeroed by the caller) is set otherwise and the row is left out.  One workspace size serves both
 * passes: hcir_class_moments_workspace_bytes (HOST). */
size_t hcir_class_moments_workspace_bytes(int64_t n, int32_t d, int32_t c);
int hcir_class_sums_f64(const float* x, int64_t n, int32_t d, int64_t ldx, const int64_t* labels, int32_t c,
                        int64_t* counts, double* sums, int32_t* bad, void* workspace, size_t workspace_bytes,
                        void* stream);
int hcir_class_scatter_f64(const float* x, int64_t n, int32_t d, int64_t ldx, const int64_t* labels, int32_t c,
                           const double* means, double* scatter, int32_t* bad, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Recall@K and AP@K of a retrieved list against per-query ground-truth ids
 * (experiments/DualViewHair/scripts/quantitative_eval.py:194-209):
 *   hit[s][q] = any ground-truth id among the first ks[s] retrieved ids
 *   ap[s][q]  = ( sum over hit ranks i < ks[s] of hits_so_far / (i + 1) ) / min(|gt_q|, ks[s]),  0 if |gt_q| = 0
 * (fp64, summed in rank order like the reference's Python floats).  retrieved [nq][kmax] (ids < 0 = empty),
 * gt [nq][gmax] padded with -1.  recall_mean / map_mean [nk] (optional, both or neither): the means over the
 * queries in index order (:228-234). */
int hcir_retrieval_metrics(const int64_t* retrieved, int64_t nq, int32_t kmax, const int64_t* gt, int32_t gmax,
                           const int32_t* ks, int32_t nk, int32_t* hit, double* ap, double* recall_mean,
                           double* map_mean, void* stream);

/* ------------------------------------------------------------------ *
 * Training side of the HSimCLR step (HP/src/pretrain_engine.py:681-751):
 * the backward of the ViT blocks and the two small losses.  Gradients flow as fp32 along the residual stream
 * and as fp16 GEMM operands; any loss scale (torch GradScaler, :745) passes through linearly.
 * ------------------------------------------------------------------ */

/* nn.GELU() forward / backward on fp16 buffers (n % 8 == 0): h = gelu(u);  du = dh * gelu'(u)
 * (MLPBlock / timm Mlp activation, HP/src/main_backbone.py:554; HP/src/models_vit.py:19). */
int hcir_gelu_fwd_f16(const void* u, int64_t n, void* h, void* stream);
int hcir_gelu_bwd_f16(const void* u, const void* dh, int64_t n, void* du, void* stream);
/* The same backward over an [m, n] matrix (row pitch ld) that also leaves colsum[n] (+)= sum_m du[m][n] - the bias
 * gradient of fc1 - in the same pass; bit-identical to hcir_gelu_bwd_f16 followed by hcir_colsum_f16.
 * workspace: hcir_colsum_chunks(m) * n floats. */
int hcir_gelu_bwd_colsum_f16(const void* u, const void* dh, int64_t m, int32_t n, int64_t ld, void* du, float* colsum,
                             int accumulate, float* workspace, size_t workspace_bytes, void* stream);

/* y_f16 = fp16(a + b)  (b may be NULL): the fp32 residual gradient as the next GEMM's fp16 operand. n % 4 == 0 */
int hcir_add_f32_f16(const float* a, const float* b, int64_t n, void* y, void* stream);

/* nn.LayerNorm(d, eps) backward over `rows` rows (ln_1 / ln_2 / encoder.ln; models_vit norm1 / norm2):
 *   xhat = (x - mean) rstd,  g = dy o gamma,  dx = rstd (g - mean(g) - xhat mean(g o xhat))
 *   dres_out[row] = (dres_in ? dres_in[row] : 0) + dx            fp32, row pitch ldr (dres_out may alias dres_in)
 *   dgamma (+)= sum_rows dy o xhat,  dbeta (+)= sum_rows dy       (accumulate != 0: added to the existing values)
 * x is the layer's INPUT (residual stream, HCIR_F32 or HCIR_F16; statistics are recomputed), dy fp16.
 * Requirements: d % 4 == 0, d <= 4096; ldx, lddy, ldr >= d and each a multiple of 4 (rows are read and written
 * four elements at a time), else HCIR_ERR_INVALID.
 * workspace: 2 * hcir_layernorm_bwd_blocks(rows) * d floats (two-stage, fixed-order column sums). */
int32_t hcir_layernorm_bwd_blocks(int64_t rows);
int hcir_layernorm_bwd(const void* x, int x_dtype, int64_t rows, int32_t d, int64_t ldx, const void* dy_f16,
                       int64_t lddy, const float* gamma, float eps, const float* dres_in, float* dres_out,
                       int64_t ldr, float* dgamma, float* dbeta, int accumulate, float* workspace,
                       size_t workspace_bytes, void* stream);
/* hcir_layernorm_bwd that also writes dres_f16[row] = fp16(dres_out[row]) (row pitch ldh) - the operand of the next
 * dgrad / wgrad GEMM, otherwise one hcir_add_f32_f16 pass - and, if dres_colsum != NULL, dres_colsum[c] = sum_rows of
 * that fp16 copy - the bias gradient of the Linear layer whose output gradient it is, otherwise one hcir_colsum_f16
 * pass.  dres_f16 NULL: exactly hcir_layernorm_bwd.  ldh >= d, ldh % 4 == 0; dres_colsum needs dres_f16 and is
 * assigned whatever `accumulate` says.  workspace: 3 * hcir_layernorm_bwd_blocks(rows) * d floats. */
int hcir_layernorm_bwd_fused(const void* x, int x_dtype, int64_t rows, int32_t d, int64_t ldx, const void* dy_f16,
                             int64_t lddy, const float* gamma, float eps, const float* dres_in, float* dres_out,
                             int64_t ldr, float* dgamma, float* dbeta, int accumulate, void* dres_f16, int64_t ldh,
                             float* dres_colsum, float* workspace, size_t workspace_bytes, void* stream);

/* out[n] (+)= sum_m x[m][n] of an fp16 matrix: the bias gradient of a Linear layer.
 * workspace: hcir_colsum_chunks(m) * n floats. */
int32_t hcir_colsum_chunks(int64_t m);
int hcir_colsum_f16(const void* x, int64_t m, int32_t n, int64_t ldx, float* out, int accumulate, float* workspace,
                    size_t workspace_bytes, void* stream);

/* Weight gradient of a Linear layer:  dw[N][K] (+)= A[M][N]^T . B[M][K]   (A = dY, B = the layer's input), fp16
 * operands, fp32 accumulate, fp32 output.  Both operands are read as stored (row-major, M the slow index): tiles go
 * to LDS by LDS-DMA and the MFMA fragments are read TRANSPOSED (ds_read_b64_tr_b16).  M is split over workgroups;
 * the partial tiles meet in `workspace` (hcir_gemm_f16_tn_workspace_bytes) and are summed in split order
 * (deterministic, no atomics).  Requirements: N % 256 == 0 or N % 128 == 0, K % 128 == 0, lda/ldb % 8 == 0. */
size_t hcir_gemm_f16_tn_workspace_bytes(int64_t m, int32_t n, int32_t k);
int hcir_gemm_f16_tn(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t m, int32_t n, int32_t k,
                     float* dw, int64_t lddw, int accumulate, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Training forward of the attention: hcir_attn_fwd for all T query rows that also writes, per (b, head, query),
 * lse[b][h][q] = log2 sum_k exp2((s_qk - max) scale log2e) + max scale log2e  (log2 domain), from which the
 * backward recomputes P = exp2(s scale log2e - lse).  hd == 64, or hd == 32 (the MAE decoder, 512 / 16 heads:
 * HairPretraining/src/backbone.py:472-482) on the generic kernel, whose `out` is bit-equal to hcir_attn_fwd's; any
 * other head_dim: HCIR_ERR_UNSUPPORTED. */
int hcir_attn_fwd_lse(const void* qkv, int64_t b, int32_t t, int32_t h, int32_t hd, float scale, void* out,
                      float* lse, void* stream);

/* Backward of hcir_attn_fwd over packed qkv [B][T][3][H][hd] (fp16): given the forward output `out` [B][T][H*hd],
 * its gradient d_out (fp16) and lse, writes d_qkv [B][T][3][H][hd] (fp16):
 *   P = softmax(scale q k^T);  dV = P^T dO;  dP = dO V^T;  dS = P o (dP - rowsum(dO o O));
 *   dQ = scale dS K;  dK = scale dS^T Q.
 * Requirements: hd == 64 or hd == 32, T <= 256.  (HP/src/models_vit.py:69-78; nn.MultiheadAttention; hd 32: the timm
 * blocks of lightly's MAEDecoderTIMM, HairPretraining/src/backbone.py:472-482, a separate kernel - attn_bwd32.hip.)
 * No atomics, fixed summation orders: two runs give the same bits. */
int hcir_attn_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, int64_t b, int32_t t,
                  int32_t h, int32_t hd, float scale, void* d_qkv, void* stream);

/* The same pair for the CLASS-TOKEN query only (token 0 of every image): the last block of a training pass whose loss
 * reads cls_token = x[:, 0] alone (HP/src/main_backbone.py:625-627).  out / d_out fp16 [B][H*64] (compact), lse fp32
 * [B][H]; d_qkv [B][T][3][H][64] receives dK, dV of every token, dQ of token 0 and ZERO for the other tokens' dQ.
 * hd == 64, T <= 256 (else HCIR_ERR_UNSUPPORTED); b * h <= 2^31 - 1 (else HCIR_ERR_INVALID, as hcir_attn_fwd and
 * hcir_attn_bwd). */
int hcir_attn_cls_fwd_lse(const void* qkv, int64_t b, int32_t t, int32_t h, int32_t hd, float scale, void* out,
                          float* lse, void* stream);
int hcir_attn_cls_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, int64_t b, int32_t t,
                      int32_t h, int32_t hd, float scale, void* d_qkv, void* stream);

/* nn.TripletMarginLoss(margin, p=2, eps, reduction='mean') (HP/src/pretrain_engine.py:96-97,717-721), fp32 [B][D]:
 *   d(x, y) = || x - y + eps ||_2,  loss = mean_i max(d(a_i, p_i) - d(a_i, n_i) + margin, 0).
 * row_loss [B] and dist [2][B] are kept for the backward; grad_out is a DEVICE scalar. */
int hcir_triplet_margin_fwd(const float* anchor, const float* positive, const float* negative, int64_t b, int32_t d,
                            float margin, float eps, float* loss, float* row_loss, float* dist, void* stream);
int hcir_triplet_margin_bwd(const float* anchor, const float* positive, const float* negative, int64_t b, int32_t d,
                            float eps, const float* row_loss, const float* dist, const float* grad_out,
                            float* d_anchor, float* d_positive, float* d_negative, void* stream);

/* F.mse_loss(x, y, reduction='mean') (HP/src/pretrain_engine.py:730) and its backward; workspace: 256 floats. */
int hcir_mse_fwd(const float* x, const float* y, int64_t n, float* loss, float* workspace, void* stream);
int hcir_mse_bwd(const float* x, const float* y, int64_t n, const float* grad_out, float* dx, float* dy,
                 void* stream);

/* fp32 -> fp16 / bf16 conversion of a contiguous buffer (gallery upload). */
int hcir_convert_f32(const float* x, int64_t n, int dtype, void* y, void* stream);

/* positive_transform of the pretrain step (HP/utils/transform.py:21-24, applied to the device batch at
 * HP/src/pretrain_engine.py:686): T.RandomRotation((-15, 15)) (nearest neighbour, zero fill) followed by
 * T.GaussianBlur(kernel_size=3) (reflect padding), in one kernel.  torchvision draws ONE angle and ONE sigma per call
 * for a batch tensor; the caller draws them and passes, as HOST arrays, theta4 = {a, b, c, d} of torchvision's inverse
 * affine matrix [[a, b, 0], [c, d, 0]] (= {cos r, sin r, -sin r, cos r}, r = radians(-angle)... computed as
 * torchvision's _get_inverse_affine_matrix does) and taps2 = {k(+-1), k(0)} of the normalised 3-tap Gaussian.
 * images / out fp32 [B][C][H][W], must not alias. */
int hcir_positive_transform(const float* images, int64_t b, int32_t c, int32_t h, int32_t w, const float* theta4,
                            const float* taps2, float* out, void* stream);

/* BatchNorm1d in TRAINING mode over x fp32 [rows][f] (lightly SimCLRProjectionHead, HP/src/main_backbone.py:589):
 * batch mean / biased variance, y = (x - mean) rstd gamma + beta (+ ReLU), running statistics updated with `momentum`
 * and the unbiased variance as torch does (running_* may be NULL).  Outputs y_f32 and / or y_f16 (one may be NULL);
 * save_mean / save_rstd [f] are kept for the backward.  ldx, ldy32, ldy16: row pitches in elements; a pitch of a
 * non-NULL operand below f is HCIR_ERR_INVALID (checked on the host, before the launch). */
int hcir_bn1d_fwd(const float* x, int64_t ldx, int64_t rows, int32_t f, const float* gamma, const float* beta,
                  float eps, float momentum, int relu, float* running_mean, float* running_var, float* save_mean,
                  float* save_rstd, float* y_f32, int64_t ldy32, void* y_f16, int64_t ldy16, void* stream);
/* Its backward: dx (fp16 [rows][f], the operand of the dgrad / wgrad GEMMs in front), dgamma, dbeta [f].
 * relu_out_f16 (optional): the forward's fp16 ReLU output; the incoming gradient is zero where it is <= 0.
 * dy_scale (optional DEVICE scalar): dy is multiplied by it first (the caller's power-of-two renormalisation);
 * dgamma and dbeta are sums of the scaled, masked gradient.  lddy, ldx, lddx and, with relu_out_f16, ldr below f:
 * HCIR_ERR_INVALID before the launch. */
int hcir_bn1d_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t rows, int32_t f,
                  const float* gamma, const float* save_mean, const float* save_rstd, const void* relu_out_f16,
                  int64_t ldr, const float* dy_scale, void* dx_f16, int64_t lddx, float* dgamma, float* dbeta,
                  void* stream);

/* ------------------------------------------------------------------ *
 * Baseline-JPEG decode on the device.  Replaces
 *   read_file + torchvision.io.decode_image(img_bytes, mode=RGB)      HP/utils/dataloader.py:28-31
 *   PIL.Image.open(path).convert('RGB')                               src/models/hair_encoder.py:108,169
 * in front of knn_transform's CenterCrop (HP/utils/transform.py:11): only the window is reconstructed.
 * Output bytes equal libjpeg-turbo's default decompressor (islow IDCT, fancy upsampling, its YCbCr
 * tables) — what both reference decoders link.
 *
 * Scope: baseline / extended sequential Huffman, 8-bit, one interleaved scan, grey or YCbCr with luma
 * sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and 1x1 chroma, with or without restart intervals.
 * Everything else (progressive, arithmetic, 12-bit, CMYK, 4:4:0, 4:1:1, multi-scan) is
 * HCIR_ERR_UNSUPPORTED from hcir_jpeg_stage and the loader keeps its host decoder for that file.
 *
 * Two steps.  (1) HOST: hcir_jpeg_stage parses the markers of one file into a header (frame geometry,
 * quantisation tables in natural order, derived Huffman tables) and copies the entropy-coded bytes into the
 * caller's (pinned) staging blob with byte stuffing (FF 00) and RSTn markers removed: the copy a loader
 * makes into pinned memory anyway.  The blob for a batch is
 *     [ hcir_jpeg_header x b ][ image 0: stream words | segment table ][ image 1 ... ]
 * with header.stage_offset = byte offset of the image's stream inside the blob.  (2) DEVICE: after ONE
 * H2D copy of the blob, hcir_jpeg_decode_window_u8 runs, per image, a workgroup that Huffman-decodes the
 * stream with one thread per fixed-size subsequence (speculative decode, then the self-synchronisation
 * hand-over of Weissenberger & Schmidt until every subsequence's start state is verified against its
 * predecessor's chain), prefix-sums the DC differences, and two small kernels for IDCT and
 * upsampling + colour conversion of the MCUs the window touches.
 * ------------------------------------------------------------------ */
#define HCIR_JPEG_LOOK_BITS 11
#define HCIR_JPEG_LOOK2 256
/* One decoded symbol, packed: bits 0-4 = bits consumed (code + magnitude bits, 1..31); bits 5-9 = zigzag advance
 * (run + 1 for a coefficient, 16 for ZRL, 1 for a DC symbol; 0 = end of block); bits 10-14 = code length.  0 = no
 * code of at most the indexed length starts with these bits. */
typedef struct hcir_jpeg_lut { /* the part of a table the device keeps in LDS */
  uint16_t look[1 << HCIR_JPEG_LOOK_BITS]; /* indexed by the next LOOK_BITS stream bits                           */
  uint16_t look2[HCIR_JPEG_LOOK2]; /* longer codes, indexed by the low bits of the 16-bit prefix: canonical codes */
  uint32_t base2;                  /* put the long ones at the top of the prefix space, from base2 on             */
  uint32_t use2;                   /* base2 >= 65536 - HCIR_JPEG_LOOK2; else long codes take the range search     */
} hcir_jpeg_lut;
typedef struct hcir_jpeg_hufftab {
  hcir_jpeg_lut lut;
  uint32_t limit[18]; /* limit[l]: first 16-bit left-aligned prefix that is NOT a code of length <= l       */
  int32_t valoff[17]; /* symbol index = (prefix >> (16 - l)) + valoff[l]                                    */
  uint8_t vals[256];
  uint32_t is_ac;
} hcir_jpeg_hufftab;

typedef struct hcir_jpeg_header {
  int32_t width, height, ncomp;
  int32_t hmax, vmax;
  int32_t hs[3], vs[3];         /* sampling factors as decoded (a grey image is 1x1)   */
  int32_t mcus_x, mcus_y, blocks_per_mcu;
  int32_t restart_interval;     /* MCUs per restart segment, 0 = none                   */
  int32_t nsegments;            /* entropy-coded segments (restart intervals), >= 1     */
  uint32_t stream_bits;         /* bits of the staged stream (segments concatenated)    */
  uint32_t stream_words;        /* 32-bit words staged, incl. 3 words of 1-bit padding  */
  uint64_t stage_offset;        /* byte offset of the stream inside the staging blob    */
  uint8_t blk_comp[12];         /* component of block i of an MCU                       */
  uint8_t dc_tab[4], ac_tab[4]; /* per component: index into huff[] (DC 0-1, AC 2-3)    */
  uint16_t quant[3][64];        /* per component, natural (row-major) order             */
  hcir_jpeg_hufftab huff[4];
} hcir_jpeg_header;

/* HOST.  Bytes of staging blob needed for this file's stream + segment table (0 if not a JPEG). */
size_t hcir_jpeg_stage_bytes(const uint8_t* file, size_t nbytes);
/* HOST.  Parse `file`, fill *hdr, write the unstuffed stream (big-endian 32-bit words) and the segment
 * table (uint32 start bit of each segment, nsegments + 1 entries) at blob + blob_offset (multiple of 16);
 * *used = bytes written (multiple of 16).  HCIR_ERR_UNSUPPORTED / HCIR_ERR_INVALID (corrupt) /
 * HCIR_ERR_WORKSPACE (cap too small). */
int hcir_jpeg_stage(const uint8_t* file, size_t nbytes, hcir_jpeg_header* hdr, uint8_t* blob,
                    size_t blob_offset, size_t blob_cap, size_t* used);
/* HOST.  The same for b files into one blob (headers at blob[0 .. b * sizeof(hcir_jpeg_header)), streams behind),
 * `nthreads` worker threads.  status[i] = per-file result; a rejected file gets a zeroed header (width 0), which
 * hcir_jpeg_decode_window_u8 skips (its window stays zero; the loader decodes that file on the host).
 * blob == NULL: only *blob_used (bytes to allocate: an upper bound from the file sizes, the entropy-coded bytes are
 * not read) and status[] are produced.  A blob that is too small: HCIR_ERR_WORKSPACE with *blob_used set - a loader
 * that recycles its (pinned) blobs calls once per batch and re-allocates only then. */
int hcir_jpeg_stage_batch(const uint8_t* const* files, const size_t* nbytes, int64_t b, uint8_t* blob,
                          size_t blob_cap, size_t* blob_used, int32_t* status, int32_t nthreads);
/* HOST.  Workspace bytes for a batch (per-image strides are the maxima over the batch). */
size_t hcir_jpeg_workspace_bytes(const hcir_jpeg_header* hdrs_host, int64_t b, int32_t win_h, int32_t win_w);
/* HOST.  Which kernels hcir_jpeg_decode_window_u8 would launch for this batch and window (the same plan, no launch):
 * *huff_threads = 1024 or 512 threads of the Huffman workgroup, *fast = 1 when every table in use resolves its long
 * codes in the second lookup level (the branch-free decode loop), else 0 (the generic loop), *color_pix = 4 or 1
 * output pixels per thread of the colour kernel. */
int hcir_jpeg_plan(const hcir_jpeg_header* hdrs_host, int64_t b, int32_t win_h, int32_t win_w, int32_t* huff_threads,
                   int32_t* fast, int32_t* color_pix);
/* blob_dev: DEVICE copy of the staging blob (headers first); hdrs_host: the same headers on the host (grid
 * sizing only).  out [b][win_h][win_w][3] uint8 = the CenterCrop((win_h, win_w)) window of every decoded
 * image, zero where the window leaves the image (torchvision pads before cropping).  status_dev [b]
 * int32 (may be NULL): 0, or a negative hcir_status when a stream did not decode to the frame's block count. */
int hcir_jpeg_decode_window_u8(const void* blob_dev, const hcir_jpeg_header* hdrs_host, int64_t b, int32_t win_h,
                               int32_t win_w, uint8_t* out, int32_t* status_dev, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * PNG decode on the device: the format of every hair-region crop the reference lists —
 *   HairPretraining/data/data_train.csv:2-3 ("133101_hair.png", ...: 103 945 of 103 945 rows),
 *   HairPretraining/data/data_{train,test}_combination3.csv, the four PNGs of assets/hair_region_only.
 * Replaces, as the JPEG entry points above do,
 *   read_file + torchvision.io.decode_image(img_bytes, mode=RGB)      HP/utils/dataloader.py:28-31
 *   PIL.Image.open(path).convert('RGB')                               src/models/hair_encoder.py:108,169
 * in front of knn_transform's CenterCrop (HP/utils/transform.py:11).  Output bytes equal libpng's / Pillow's:
 * inflate and the scanline filters are exact integer algorithms (RFC 1950/1951, PNG spec §9).
 *
 * Scope: 8-bit samples, non-interlaced, colour types 0 (grey), 2 (RGB), 3 (palette), 4 (grey + alpha),
 * 6 (RGBA); the RGB conversion is the one `convert('RGB')` / `mode=RGB` make: grey replicated, alpha dropped,
 * palette indices through PLTE.  Everything else (16-bit, 1/2/4-bit, Adam7) is HCIR_ERR_UNSUPPORTED from
 * hcir_png_stage and the loader keeps its host decoder for that file.
 *
 * Two steps, as for JPEG.  (1) HOST: hcir_png_stage walks the chunks (IHDR, PLTE, IDAT ..., optionally verifying
 * every chunk's CRC-32 as Pillow does), fills a header and concatenates the IDAT payloads — the zlib stream —
 * into the caller's (pinned) staging blob:
 *     [ hcir_png_header x b ][ image 0: zlib stream, zero padded to 16 B + 16 B ][ image 1 ... ]
 * (2) DEVICE: hcir_png_decode_window_u8 runs one wavefront per image that inflates the stream up to the last
 * scanline the window needs (stored, fixed and dynamic Huffman blocks; the 32 KB history is an LDS ring; match
 * copies are lane-parallel), then one wavefront per image that undoes the filters of rows 0..last along the
 * anti-diagonals of (row, pixel) — lane = row, so Paeth's left / up / upper-left are a register and two
 * neighbour-lane reads — and writes the window's RGB8 pixels.
 * ------------------------------------------------------------------ */
typedef struct hcir_png_header {
  int32_t width, height;
  int32_t color_type;    /* 0, 2, 3, 4, 6                                                */
  int32_t bpp;           /* bytes per pixel of the filtered scanlines: 1, 3, 1, 2, 4      */
  uint32_t stream_bytes; /* bytes of the zlib stream (IDAT payloads concatenated)         */
  uint32_t reserved;
  uint64_t stage_offset; /* byte offset of the stream inside the staging blob (16-aligned) */
  uint8_t palette[768];  /* PLTE, RGB triples (colour type 3)                             */
} hcir_png_header;

/* Longest zlib stream (IDAT payloads joined) the device decodes: 2^29 - 256 bytes, so that the inflate's 32-bit bit
 * positions cannot wrap.  hcir_png_stage reports a longer stream as HCIR_ERR_UNSUPPORTED (the loader keeps its host
 * decoder for it); hcir_png_workspace_bytes / hcir_png_decode_window_u8 reject a header with stream_bytes at or
 * above it. */
#define HCIR_PNG_MAX_STREAM_BYTES ((1u << 29) - 256u)
#define HCIR_PNG_VERIFY_CRC 1 /* flags: verify the CRC-32 of every chunk while staging (Pillow's default)   */

/* HOST.  Bytes of staging blob needed for this file's stream (0 if it is not a PNG of the subset above). */
size_t hcir_png_stage_bytes(const uint8_t* file, size_t nbytes);
/* HOST.  Parse `file`, fill *hdr, copy the zlib stream to blob + blob_offset (multiple of 16); *used = bytes
 * written (multiple of 16).  HCIR_ERR_UNSUPPORTED / HCIR_ERR_INVALID (not a PNG, corrupt chunk structure or CRC) /
 * HCIR_ERR_WORKSPACE. */
int hcir_png_stage(const uint8_t* file, size_t nbytes, int32_t flags, hcir_png_header* hdr, uint8_t* blob,
                   size_t blob_offset, size_t blob_cap, size_t* used);
/* HOST.  The same for b files into one blob (headers first), `nthreads` worker threads; status[i] per file, a
 * rejected file gets a zeroed header (width 0) that the device skips.  blob == NULL: only *blob_used and status[]. */
int hcir_png_stage_batch(const uint8_t* const* files, const size_t* nbytes, int64_t b, int32_t flags, uint8_t* blob,
                         size_t blob_cap, size_t* blob_used, int32_t* status, int32_t nthreads);
/* HOST.  Workspace bytes for a batch: the inflated scanlines 0..last needed row of every image. */
size_t hcir_png_workspace_bytes(const hcir_png_header* hdrs_host, int64_t b, int32_t win_h, int32_t win_w);
/* blob_dev: DEVICE copy of the staging blob; hdrs_host: the same headers on the host (sizing only).
 * out [b][win_h][win_w][3] uint8 = the CenterCrop((win_h, win_w)) window of every decoded image, zero where the
 * window leaves the image.  status_dev [b] int32 (may be NULL): 0, or HCIR_ERR_INVALID when the stream is corrupt
 * (bad block type / code set / distance, a filter type > 4, or it ends before the last needed scanline). */
int hcir_png_decode_window_u8(const void* blob_dev, const hcir_png_header* hdrs_host, int64_t b, int32_t win_h,
                              int32_t win_w, uint8_t* out, int32_t* status_dev, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * Resize(224, bicubic) + CenterCrop(224) on the device: the input transform of the hair_retrieval path,
 *   transforms.Resize(224, interpolation=3) -> CenterCrop(224)        src/models/hair_encoder.py:44-48
 * applied in extract_dataset_features (:116-117) and encode_single_image (:175).  torchvision hands a PIL image to
 * Image.resize(size, BICUBIC): Pillow's two-pass separable resampler (third-party, not under /root/reference;
 * Pillow 12.2 src/libImaging/Resample.c): per output pixel a window of the bicubic kernel (a = -0.5) widened by the
 * scale (antialias), coefficients normalised in double and rounded to 22-bit fixed point, horizontal pass first,
 * an 8-bit clipped intermediate, then the vertical pass.  The coefficient tables are computed on the HOST with the
 * same double arithmetic; the two passes run on the device in the same integer arithmetic: bytes equal Pillow's.
 * Only the pixels the crop window needs are computed.
 * ------------------------------------------------------------------ */
/* HOST.  Taps per output pixel (Pillow's ksize) of one axis resampled from in_size to out_size; 0 on bad sizes. */
int32_t hcir_resize_bicubic_ksize(int32_t in_size, int32_t out_size);
/* HOST.  bounds [2 * out_size] = (first source index, tap count) per output index; kk [out_size * ksize] = the
 * 22-bit fixed-point coefficients (precompute_coeffs + normalize_coeffs_8bpc). */
int hcir_resize_bicubic_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* kk);

typedef struct hcir_resize_job { /* one image of a batch */
  uint64_t src_offset;          /* bytes from `src`: RGB8 rows of the source image                              */
  int64_t src_pitch;            /* bytes between its rows                                                        */
  int32_t src_h, src_w;
  int32_t out_h, out_w;         /* size after the resize (before the crop)                                       */
  int32_t crop_top, crop_left;  /* origin of the window inside the resized image (negative: zero padding)       */
  int32_t coef_h, coef_v;       /* int32 offsets into `coef`: [bounds (2 * out) | kk (out * ksize)] of each axis; */
  int32_t ksize_h, ksize_v;     /* -1 offset: that axis is not resampled (out == in)                             */
} hcir_resize_job;

/* HOST.  Workspace bytes: the horizontal pass's 8-bit intermediate of every image. */
size_t hcir_resize_crop_workspace_bytes(const hcir_resize_job* jobs_host, int64_t b, int32_t win_h, int32_t win_w);
/* src, coef, jobs_dev: DEVICE; jobs_host: the same records on the host (sizing).  out [b][win_h][win_w][3] uint8. */
int hcir_resize_crop_bicubic_u8(const uint8_t* src, const int32_t* coef, const hcir_resize_job* jobs_dev,
                                const hcir_resize_job* jobs_host, int64_t b, int32_t win_h, int32_t win_w,
                                uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* HOST.  The same tables for a named Pillow filter (Image.Resampling numbering).  HCIR_FILTER_BICUBIC returns exactly
 * what hcir_resize_bicubic_ksize / _coeffs return; HCIR_FILTER_BILINEAR is the triangle filter (support 1.0) of
 * Image.resize(size, BILINEAR).  Any other filter: 0 / HCIR_ERR_UNSUPPORTED.  The device resampler above takes its
 * tables, tap counts, source offset and pitch per job, so it runs either filter, and a crop box followed by a resize
 * (img.crop(box).resize(size)) is a job whose source is the box. */
#define HCIR_FILTER_BILINEAR 2
#define HCIR_FILTER_BICUBIC 3
int32_t hcir_resize_ksize(int32_t filter, int32_t in_size, int32_t out_size);
int hcir_resize_coeffs(int32_t filter, int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* kk);

/* ------------------------------------------------------------------ *
 * SimCLR training views on the device: the input of the pretrain step (batch["anchor"], batch["pos1"]).
 *   transform = SimCLRTransform(input_size=224)                        HP/mainpretrain.py:130
 *   images = self.transform(image); {"anchor": images[0], "pos1": images[1]}   HP/utils/dataloader.py:36-38
 * lightly's SimCLRTransform is, on a PIL image: RandomResizedCrop(224, scale=(0.08, 1)) (bilinear) ->
 * RandomHorizontalFlip -> RandomApply(ColorJitter(0.8, 0.8, 0.8, 0.2), p=0.8) -> RandomGrayscale(0.2) ->
 * GaussianBlur(sigmas=(0.1, 2), prob=0.5) -> ToTensor -> Normalize(ImageNet); every op is executed by Pillow
 * (third-party; Pillow 12.2 libImaging Blend.c, Convert.c, BoxBlur.c, Resample.c).
 * The crop + resize is a job of hcir_resize_crop_bicubic_u8 with bilinear tables; everything after it is
 * hcir_simclr_view_f32: one workgroup per view, the 224 x 224 RGB8 image resident in LDS (3 planes of 224 rows with
 * a 228-byte pitch = 153 216 of the CU's 163 840 bytes) from the load to the fp32 store.  Bytes equal Pillow's after
 * every op, and the fp32 output equals ToTensor + Normalize of them bit for bit.  All random draws are the caller's.
 * ------------------------------------------------------------------ */
#define HCIR_VIEW_SIZE 224
#define HCIR_VIEW_BRIGHTNESS 0 /* entries of hcir_view_params.order */
#define HCIR_VIEW_CONTRAST 1
#define HCIR_VIEW_SATURATION 2
#define HCIR_VIEW_HUE 3

typedef struct hcir_view_params { /* one view */
  int32_t flip;                   /* 0 / 1: horizontal flip                                                     */
  int32_t jitter;                 /* 0 / 1: apply the four colour ops below                                     */
  int32_t order[4];               /* a permutation of HCIR_VIEW_BRIGHTNESS .. HCIR_VIEW_HUE: the order they run */
  float brightness, contrast, saturation; /* enhancement factors, finite and >= 0                               */
  float hue;                      /* in [-0.5, 0.5]                                                             */
  int32_t gray;                   /* 0 / 1: every channel <- L                                                  */
  int32_t blur;                   /* 0 / 1: Gaussian blur by three box passes per axis with ...                 */
  int32_t blur_r;                 /* ... whole pixels each side (0 or 1: sigma <= 2.3),                         */
  uint32_t blur_ww, blur_fw;      /* ... and these 24-bit weights (hcir_view_blur_weights)                      */
  float sigma;                    /* the sigma they derive from (kept for the caller; not read by the kernel)   */
} hcir_view_params;

/* HOST.  Pillow's box-blur weights for ImageFilter.GaussianBlur(radius = sigma).  sigma must be finite and > 0;
 * HCIR_ERR_UNSUPPORTED when it needs more than one whole pixel each side (sigma > 2.3). */
int hcir_view_blur_weights(float sigma, int32_t* r, uint32_t* ww, uint32_t* fw);
/* crops: DEVICE uint8 [n][224][224][3]; params_dev: DEVICE, params_host: the same records on the host (checked here:
 * HCIR_ERR_INVALID for a flag that is not 0 / 1, an order that is no permutation, a factor out of range, blur weights
 * that do not sum to at most 2^24).  mean3 / std3: HOST.  out: DEVICE fp32 [n][3][224][224]. */
int hcir_simclr_view_f32(const uint8_t* crops, const hcir_view_params* params_dev, const hcir_view_params* params_host,
                         int64_t n, const float* mean3, const float* std3, float* out, void* stream);

/* ------------------------------------------------------------------ *
 * ResNet-18 / ResNet-50 trunk, eval mode (running statistics): the inference engine.  hcir_conv2d_f16 with the
 * identity epilogue is also the train-mode forward and the data gradient of the body convolutions (next section).
 * Replaces the nn.Sequential(children()[:-1]) trunk behind SHAM2.extract_features / extract_features_ema
 * (HP/src/main_backbone.py:572-578,624-629) and SimCLR.extract_features (HP/src/backbone.py:660-661):
 * torchvision Conv2d / BatchNorm2d / ReLU / MaxPool2d / AdaptiveAvgPool2d.
 * Activations are NHWC fp16; accumulation and every epilogue are fp32; each stored value is rounded to fp16 once.
 * ------------------------------------------------------------------ */

/* Implicit-GEMM convolution (no im2col buffer) fused with the folded BatchNorm, the block's residual add and ReLU:
 *   out[b][ho][wo][n] = fp16( relu?( acc * scale[n] + bias[n] (+ resid[b][ho][wo][n]) ) ),
 *   acc = sum_{r,s,c} x[b][ho*stride + r - pad][wo*stride + s - pad][c] * w[n][r][s][c]   (padding taps are zeros).
 * x fp16 [B][H][W][Cin]; w fp16 [Cout][R][S][Cin]; scale, bias fp32 [Cout] (scale = gamma / sqrt(var + eps) stays
 * out of the fp16 weights: a small running_var would overflow them); resid fp16 of out's shape or NULL, added in
 * fp32; out fp16 [B][Ho][Wo][Cout], Ho = (H + 2 pad - R) / stride + 1.
 * Kernels exist for (R, S, pad) in {(1,1,0), (3,3,1)}, stride in {1, 2}, Cin % 64 == 0, Cout % 64 == 0, any
 * B, H, W >= 1; anything else is HCIR_ERR_UNSUPPORTED (decided from the shape alone, before any pointer is looked at
 * or the device is touched). */
int hcir_conv2d_f16(const void* x, int64_t b, int32_t h, int32_t w, int32_t cin, const void* wgt, int32_t cout,
                    int32_t r, int32_t s, int32_t stride, int32_t pad, const float* scale, const float* bias,
                    const void* resid, int relu, void* out, void* stream);
/* HOST.  Width of the output-channel tile hcir_conv2d_f16 runs this shape with: 128 when Cout % 128 == 0 and the
 * launch still has at least 512 workgroups of 128 pixels x 128 channels, else 64 (two instantiations of one kernel; a
 * test uses this to know which one a case exercised).  Negative: the status hcir_conv2d_f16 returns for the shape. */
int32_t hcir_conv2d_tile_n(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r, int32_t s,
                           int32_t stride, int32_t pad);

/* The stem: Conv2d(3, 64, 7, stride 2, pad 3) + folded BatchNorm + ReLU + MaxPool2d(3, stride 2, pad 1) in one
 * kernel; the Hc x Wc x 64 pre-pool map never goes to memory.  img fp32 NCHW [B][3][H][W], H, W >= 7 (smaller:
 * HCIR_ERR_UNSUPPORTED); out fp16 NHWC [B][Hp][Wp][64] with Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1.
 * The image is rounded to fp16 for the MFMA (as the weights are); conv * scale + bias and ReLU are fp32, the max is
 * taken over the fp32 values of the window's positions INSIDE the conv map (padding is excluded, not zero) and
 * rounded once.  w_packed fp16 [10][2][64][8]: element j of lane l of MFMA step kk, n tile nt is
 * W[nt * 32 + (l & 31)][k = 16 kk + 8 (l >> 5) + j] with k = (c * 7 + ky) * 7 + kx, zero for k >= 147
 * (hcir.resnet_engine.pack_stem_weight). */
int hcir_resnet_stem(const float* img, int64_t b, int32_t h, int32_t w, const void* w_packed, const float* scale,
                     const float* bias, void* out, void* stream);

/* AdaptiveAvgPool2d((1, 1)) + flatten: out[b][c] = mean over H*W of x fp16 [B][H][W][C], fp32 out [B][C].
 * fp32 compensated summation in index order, no atomics: the result does not depend on the launch.  l2_normalize != 0:
 * each row is divided by max(||row||_2, eps) (F.normalize, HP/src/classification_engine.py:50, eps 1e-12). */
int hcir_avgpool_nhwc_f16(const void* x, int64_t b, int32_t h, int32_t w, int32_t c, int l2_normalize, float eps,
                          float* out, void* stream);

/* ------------------------------------------------------------------ *
 * ResNet-18 / ResNet-50 body convolutions, backward (training; hcir/conv_train.py, the model's `hip_train` switch).
 * Serves the backward of the torchvision Conv2d modules behind HP/src/main_backbone.py:576-579, reached from
 * scaler.scale(total_loss).backward() at HP/src/pretrain_engine.py:747 (the step runs under torch.autocast(fp16),
 * HP/src/pretrain_engine.py:681,715: fp16 operands with fp32 accumulation are the reference's own arithmetic).
 * The data gradient needs no kernel of its own: it is hcir_conv2d_f16 over dy with the flipped, transposed weight
 * (stride 1), followed (1x1 stride 2) or preceded (3x3 stride 2) by hcir_spread2_nhwc_f16.
 * ------------------------------------------------------------------ */

/* Weight gradient of hcir_conv2d_f16's convolution:
 *   dw[n][r][s][c] = sum_{b,ho,wo} dy[b][ho][wo][n] * x[b][ho*stride + r - pad][wo*stride + s - pad][c]
 * (padding taps are zeros).  x fp16 [B][H][W][Cin]; dy fp16 [B][Ho][Wo][Cout]; dw fp32 [Cout][R][S][Cin], overwritten.
 * fp32 accumulation; the B*Ho*Wo pixels are split over workgroups whose partial tiles go to `workspace` and are added
 * in split order: no float atomics, two calls give the same bits.  Shapes and statuses as the forward: (R, S, pad) in
 * {(1,1,0), (3,3,1)}, stride in {1, 2}, Cin % 64 == 0, Cout % 64 == 0, any B, H, W >= 1; anything else is
 * HCIR_ERR_UNSUPPORTED, decided from the shape alone before a pointer is looked at.  HCIR_ERR_WORKSPACE when
 * `workspace_bytes` is below the size the shape needs (0 when one split covers M; `workspace` may then be NULL). */
int hcir_conv2d_wgrad_f16(const void* x, const void* dy, int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout,
                          int32_t r, int32_t s, int32_t stride, int32_t pad, float* dw, void* workspace,
                          size_t workspace_bytes, void* stream);
/* HOST.  Workspace of the weight gradient for a shape: splits * Cout * R * S * Cin * 4 bytes, 0 when one split covers
 * M or the shape has no kernel. */
size_t hcir_conv2d_wgrad_workspace_bytes(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r,
                                         int32_t s, int32_t stride, int32_t pad);
/* HOST.  Number of M splits the weight gradient runs this shape with (a test uses it to know which path a case
 * exercised).  Negative: the status the weight gradient returns for the shape. */
int32_t hcir_conv2d_wgrad_splits(int64_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t r, int32_t s,
                                 int32_t stride, int32_t pad);

/* dst[b][2i][2j][:] = src[b][i][j][:], zero elsewhere: src fp16 [B][hs][ws][C], dst fp16 [B][h][w][C], every element
 * of dst written (plain vector stores, no memset needed).  HCIR_ERR_INVALID unless 2 (hs - 1) <= h - 1 and
 * 2 (ws - 1) <= w - 1; HCIR_ERR_UNSUPPORTED unless C % 8 == 0. */
int hcir_spread2_nhwc_f16(const void* src, int64_t b, int32_t hs, int32_t ws, int32_t c, int32_t h, int32_t w,
                          void* dst, void* stream);

/* ------------------------------------------------------------------ *
 * ResNet-18 / ResNet-50 body normalisation in training: batch-statistics BatchNorm2d, optionally with the block's
 * residual add and ReLU, forward and backward (csrc/bn2d.hip; hcir/conv_train.py, the model's `hip_train_norm`
 * switch).  Serves the torchvision BatchNorm2d / ReLU / `out += identity` behind HP/src/main_backbone.py:576-579 in
 * the step of HP/src/pretrain_engine.py:682-747.
 * Maps are fp16 NHWC viewed as [m = B*H*W][c]; parameters, statistics and their gradients fp32 [c].  fp32 arithmetic,
 * each stored activation rounded to fp16 once; the m rows are cut into hcir_bn2d_chunks(m, c) contiguous ranges whose
 * partial results go to `workspace` ([chunk][c][2] fp32) and are merged in a fixed order: no atomics, two calls give
 * the same bits.  Statuses, decided from the shape alone before a pointer is looked at: HCIR_ERR_UNSUPPORTED unless
 * c % 64 == 0 and 64 <= c <= 65536 (and m < 2^31), HCIR_ERR_INVALID for m < 2 (one value per channel has no variance)
 * or a required pointer that is NULL, HCIR_ERR_WORKSPACE when `workspace_bytes` is below
 * hcir_bn2d_workspace_bytes(m, c).  The entry points allocate nothing and do not synchronise.
 * ------------------------------------------------------------------ */

/* y = fp16(relu?((x - mean) * rstd * gamma + beta (+ resid))) with mean and the biased variance of this batch
 * (F.batch_norm(training=True)).  Three launches: per-chunk (mean, M2) from shifted sums, a merge by Chan's formula
 * that writes save_mean [c] and save_rstd [c] = 1 / sqrt(var_biased + eps) and, where running_mean / running_var are
 * not NULL, running = (1 - momentum) * running + momentum * (mean | M2 / (m - 1)), then the elementwise pass.
 * resid: fp16 [m][c] or NULL; relu: 0 / 1. */
int hcir_bn2d_fwd_nhwc_f16(const void* x, int64_t m, int32_t c, const float* gamma, const float* beta, float eps,
                           float momentum, const void* resid, int relu, float* running_mean, float* running_var,
                           float* save_mean, float* save_rstd, void* y, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Backward of the above.  g = dy, or dy where y_relu > 0 and 0 elsewhere when y_relu (the forward's output y of a call
 * with relu = 1) is not NULL; xhat = (x - mean) * rstd.  dbeta = sum g, dgamma = sum g * xhat (fp32 [c]),
 * dx = fp16(gamma * rstd * (g - dbeta / m - xhat * dgamma / m)), and, where dresid is not NULL, dresid = fp16(g): the
 * gradient of the residual branch, exactly dy or 0.  Three launches: per-chunk sums, their merge, the elementwise
 * pass. */
int hcir_bn2d_bwd_nhwc_f16(const void* dy, const void* x, const void* y_relu, int64_t m, int32_t c,
                           const float* gamma, const float* save_mean, const float* save_rstd, void* dx, void* dresid,
                           float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* HOST.  Workspace of either call for a shape: chunks * c * 2 * 4 bytes; 0 when the shape has no kernel. */
size_t hcir_bn2d_workspace_bytes(int64_t m, int32_t c);
/* HOST.  Number of row chunks the reductions run the shape with (a test uses it to know which path a case
 * exercised).  Negative: the status the entry points return for the shape. */
int32_t hcir_bn2d_chunks(int64_t m, int32_t c);
/* The statistics half of hcir_bn2d_fwd_nhwc_f16 alone - its first two launches, the same kernels, the same bits:
 * save_mean, save_rstd and the running-statistic update, no elementwise pass.  Same shape rules, statuses and
 * workspace.  The stem normalises inside its pooling kernel (below). */
int hcir_bn2d_stats_nhwc_f16(const void* x, int64_t m, int32_t c, float eps, float momentum, float* running_mean,
                             float* running_var, float* save_mean, float* save_rstd, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * The ResNet stem in training: Conv2d(3, 64, 7, stride 2, pad 3), batch-statistics BatchNorm2d, ReLU and
 * MaxPool2d(3, stride 2, pad 1), forward and backward (csrc/stem_train.hip; hcir/conv_train.py stem_train, the
 * model's `hip_train_stem` switch).  Serves the first four torchvision modules of the trunk behind
 * HP/src/main_backbone.py:576-579 in the step of HP/src/pretrain_engine.py:682-747.
 *   forward    c = hcir_stem_conv_f16(img);  hcir_bn2d_stats_nhwc_f16(c);  p = hcir_stem_bn_relu_pool_f16(c)
 *   backward   g = hcir_stem_pool_relu_bwd_f16(dp, c);  dc, dgamma, dbeta = hcir_bn2d_bwd_nhwc_f16(dy = g, x = c,
 *              y_relu = NULL);  dw = hcir_stem_wgrad_f16(img, dc).  The image needs no gradient: no data gradient.
 * Sizes as hcir_resnet_stem: Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1.  img fp32 NCHW [B][3][H][W]; the conv-level
 * maps c, g, dc fp16 NHWC [B][Hc][Wc][64]; the pooled maps p, dp fp16 NHWC [B][Hp][Wp][64].  Statuses are decided
 * from the shape alone before a pointer is looked at: HCIR_ERR_INVALID for a size below 1, HCIR_ERR_UNSUPPORTED for
 * H < 7 or W < 7 (Hc < 4 or Wc < 4 where the entry point takes the conv map's size), then HCIR_ERR_INVALID for a NULL
 * pointer.  No atomics; the caller's stream; no allocation or synchronisation inside; two calls give the same bits.
 * ------------------------------------------------------------------ */

/* c = fp16(conv7x7/2/pad3(fp16(img), fp16(W))), fp32 accumulation, no epilogue.  w_packed: hcir_resnet_stem's
 * (hcir.resnet_engine.pack_stem_weight).  Non-overlapping 16 x 16 tiles of conv pixels; 16-byte stores. */
int hcir_stem_conv_f16(const float* img, int64_t b, int32_t h, int32_t w, const void* w_packed, void* out,
                       void* stream);
/* p = fp16(max over the window's positions INSIDE the conv map of relu((c - mean) * (rstd * gamma) + beta)): fp32
 * arithmetic, one rounding; padding is excluded from the max, not zero (as in hcir_resnet_stem). */
int hcir_stem_bn_relu_pool_f16(const void* c, int64_t b, int32_t hc, int32_t wc, const float* gamma,
                               const float* beta, const float* save_mean, const float* save_rstd, void* out,
                               void* stream);
/* Backward of the above down to the conv map, the gradient with respect to y = (c - mean) * (rstd * gamma) + beta:
 *   g[i][j] = fp16(sum over the 1, 2 or 4 windows containing (i, j) of
 *                  dp[window] * [(i, j) is the window's selected position] * [y(i, j) > 0]),
 * fp32 sum in a fixed order, every element of g written by a plain store.  The selected position is torch's: the first,
 * in row-major order of the window, among the positions inside the map at which y is maximal; y is monotone in c per
 * channel, so it is found on the fp16 values of c (first maximum where rstd * gamma > 0, first minimum where < 0,
 * first position where == 0). */
int hcir_stem_pool_relu_bwd_f16(const void* dp, const void* c, int64_t b, int32_t hc, int32_t wc, const float* gamma,
                                const float* beta, const float* save_mean, const float* save_rstd, void* g,
                                void* stream);
/* dw[n][(ch * 7 + ky) * 7 + kx] = sum_{b,i,j} dc[b][i][j][n] * fp16(img[b][ch][2i - 3 + ky][2j - 3 + kx]) (zero
 * outside the image): dw fp32 [64][3][7][7], torch's layout, overwritten.  hcir_stem_wgrad_parts(b, h, w) persistent
 * workgroups each add a contiguous run of 16 x 16 conv tiles in registers and write one partial to `workspace`; a second
 * launch adds the partials in part order.  With one part dw is stored directly and `workspace` may be NULL.
 * HCIR_ERR_WORKSPACE when `workspace_bytes` is below hcir_stem_wgrad_workspace_bytes(b, h, w). */
int hcir_stem_wgrad_f16(const float* img, const void* dc, int64_t b, int32_t h, int32_t w, float* dw, void* workspace,
                        size_t workspace_bytes, void* stream);
/* HOST.  parts * 64 * 147 * 4 bytes; 0 with one part or for a shape without a kernel. */
size_t hcir_stem_wgrad_workspace_bytes(int64_t b, int32_t h, int32_t w);
/* HOST.  Number of parts: conv tiles / max(4, ceil(conv tiles / 512)), rounded up.  Negative: the status the weight
 * gradient returns for the shape. */
int32_t hcir_stem_wgrad_parts(int64_t b, int32_t h, int32_t w);

/* ------------------------------------------------------------------ *
 * SimMIM pre-training around the ViT walk (csrc/mim.hip; hcir/backbone.py SimMIM, hcir/vit_train.py).  Serves
 * HairPretraining/src/backbone.py:549-601 and src/pretrain_engine.py:514-532: lightly's mask_at_index in front of the
 * encoder, patchify + the gather of the masked patches, nn.L1Loss.  Four memory-bound passes; the network between
 * them is the existing walk.  b images, t = 1 + patches tokens per image, d features, P = C ps ps elements per patch.
 * No float atomics: partial sums go to `workspace` and are added in a fixed order, two calls give the same bits.
 * 16-byte accesses throughout: HCIR_ERR_UNSUPPORTED unless d % 8 == 0 resp. P % 8 == 0 (and P <= 12288, one patch
 * in LDS); HCIR_ERR_INVALID for a size below 1, an image side that is no multiple of ps, or a NULL pointer;
 * HCIR_ERR_WORKSPACE for a NULL or short workspace.  Statuses are decided before anything is launched.
 * Token indices `idx` (int64, lightly's idx_mask: 0 = class token, 1 + p = patch p) are read on the device and
 * range-checked there: a row whose index is outside [1, t) reads no image, is written as zero and adds nothing to a
 * sum.  The byte mask of the other two calls is a table [b][t] indexed by position: it cannot address anything.
 * ------------------------------------------------------------------ */

/* tok[b][k][:] = round(mask_token + pos_mult * pos[k]) for every (b, k) with mask[b][k] != 0 (k = 0, the class token,
 * included); every other row is left as it is.  tok [b][t][d] in tok_dtype (HCIR_F32 | HCIR_F16) as hcir_patch_embed
 * wrote it; mask_token fp32 [d], pos fp32 [t][d].  One fp32 fma (one rounding), one rounding to tok_dtype. */
int hcir_mim_mask_tokens(void* tok, int tok_dtype, int64_t b, int32_t t, int32_t d, const uint8_t* mask,
                         const float* mask_token, const float* pos, float pos_mult, void* stream);
/* Backward of the above, one pass over the stream gradient dtok fp32 [b][t][d]:
 *   g_mask_token[d]          = sum over the rows with mask != 0 of dtok[b][k][:]          (fp32, overwritten)
 *   dpatch[b (t-1) + p][:]   = mask[b][1 + p] ? +0 : fp16(dtok[b][1 + p][:])              (fp16 [b (t-1)][d])
 * Rows of dpatch behind b (t-1) are not touched.  The b t rows are cut into chunks = clamp(ceil(b t / 64), 1, 256)
 * shares of ceil(b t / chunks) consecutive rows; inside a share 8 row lanes (row % 8 within the share) add their rows
 * in order, the lanes are added in order, then the shares in order. */
int hcir_mim_mask_bwd(const float* dtok, int64_t b, int32_t t, int32_t d, const uint8_t* mask, float* g_mask_token,
                      void* dpatch, void* workspace, size_t workspace_bytes, void* stream);
/* HOST.  chunks * d * 4 bytes; 0 for a shape without a kernel. */
size_t hcir_mim_mask_bwd_workspace_bytes(int64_t b, int32_t t, int32_t d);
/* out[b n + j][(py ps + px) C + ch] = img[b][ch][gy ps + py][gx ps + px] with patch idx[b][j] - 1 = gy (W / ps) + gx:
 * the rows patchify(img)[idx - 1] in lightly's element order, channel fastest.  img fp32 [b][C][H][W], idx int64
 * [b][n], out fp32 [b n][P].  Data movement only: bit-exact. */
int hcir_mim_patch_targets(const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps,
                           const int64_t* idx, int32_t n, float* out, void* stream);
/* loss = mean over all b n P elements of |pred - target| (fp32 device scalar) and sgn = sign(pred - target) in
 * {-1, 0, +1} (fp16 [b n][P]), target = the rows hcir_mim_patch_targets would write, read from the image and never
 * stored.  pred fp16 [b n][P].  Differences and sums are fp32.  Workgroup w of blocks = min(b n, 1024) takes the
 * ceil(b n / blocks) rows from w ceil(b n / blocks); a thread adds its elements in order, a workgroup its threads by
 * the xor butterfly and its four waves in order, a last launch the workgroups (thread i the parts i, i + 256, ...,
 * then the same workgroup sum) and multiplies by 1 / (b n P).  The gradient of the loss is grad_out / (b n P) * sgn:
 * there is no backward kernel. */
int hcir_mim_l1_fwd(const void* pred, const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps,
                    const int64_t* idx, int32_t n, float* loss, void* sgn, void* workspace, size_t workspace_bytes,
                    void* stream);
/* HOST.  blocks * 4 bytes for rows = b n. */
size_t hcir_mim_l1_workspace_bytes(int64_t rows);

/* ------------------------------------------------------------------------------------------------------------------
 * MAE pre-training (csrc/mae.hip; HairPretraining/src/backbone.py:462-525, src/pretrain_engine.py:323-338).  Token
 * indices are int64 [b][k], distinct per image, in [0, t); a compact buffer has row i k + j for (image i, idx[i][j]).
 * Shapes: d % 8 == 0, t <= 1024, 1 <= k <= t (else HCIR_ERR_UNSUPPORTED / HCIR_ERR_INVALID).  An index outside [0, t)
 * addresses nothing: its compact row is written as zero / ignored.
 * ------------------------------------------------------------------------------------------------------------------ */
/* out[i k + j][:] = tok[i][idx[i][j]][:] for fp16 tok [b t][d] -> fp16 out [pad64(b k)][d], pad rows written as zero.
 * A copy: bit-exact.  lightly's get_at_index: MaskedVisionTransformerTIMM.encode(images, idx_keep), which
 * backbone.py:484-486 calls, and get_at_index(x_decoded, idx_mask) at backbone.py:501. */
int hcir_mae_gather_rows(const void* tok, int64_t b, int32_t t, int32_t d, const int64_t* idx, int32_t k, void* out,
                         void* stream);
/* Its backward: dtok[i][tok][:] = comp[i k + j][:] where idx[i][j] == tok, 0 for every other token; fp32 comp
 * [>= b k][d] -> fp32 dtok [b t][d].  EVERY row of dtok is written (no fill in front).  Bit-exact.  (autograd through
 * the two get_at_index calls above, pretrain_engine.py:334.) */
int hcir_mae_scatter_rows(const float* comp, int64_t b, int32_t t, int32_t d, const int64_t* idx, int32_t k,
                          float* dtok, void* stream);
/* x[i][tok][:] = fp16((tok in idx_keep[i] at j ? fp32(embed[i k + j][:]) : mask_token[:]) + pos[tok][:]): the decoder's
 * input, built in one pass.  embed fp16 [>= b k][d] (decoder_embed of the encoder output), mask_token fp32 [d], pos fp32
 * [t][d] (decoder_pos_embed), x fp16 [b t][d].  One fp32 add and one rounding to fp16 per element.
 * (repeat_token / set_at_index at backbone.py:492-495 and MAEDecoderTIMM.decode's position add behind :498.) */
int hcir_mae_decoder_input(const void* embed, int64_t b, int32_t t, int32_t d, const int64_t* idx_keep, int32_t k,
                           const float* mask_token, const float* pos, void* x, void* stream);
/* Its backward, from the fp32 gradient dres [b t][d] of x: d_embed[i k + j][:] = fp16(dres[i][idx_keep[i][j]][:]) (rows
 * past b k are not touched) and g_mask_token[:] = the sum of the rows whose token is not in idx_keep, in a fixed order:
 * chunks = min(b, 256) shares of ceil(b / chunks) consecutive images; inside a share 8 row lanes (token % 8) add their
 * rows image by image in order, the lanes are added in order, then the shares in order.  decoder_pos_embed takes no
 * gradient (requires_grad=False in lightly).  workspace: hcir_mae_decoder_input_bwd_workspace_bytes. */
int hcir_mae_decoder_input_bwd(const float* dres, int64_t b, int32_t t, int32_t d, const int64_t* idx_keep, int32_t k,
                               void* d_embed, float* g_mask_token, void* workspace, size_t workspace_bytes,
                               void* stream);
/* HOST.  chunks * d * 4 bytes; 0 for a shape without a kernel. */
size_t hcir_mae_decoder_input_bwd_workspace_bytes(int64_t b, int32_t d);
/* loss = mean over all b n P elements of (pred - target)^2 (fp32 device scalar; nn.MSELoss, the criterion of
 * train_one_epoch_mae, pretrain_engine.py:331) and diff = fp16(pred - target) (fp16 [b n][P]), target =
 * patchify(img)[idx - 1] as hcir_mim_patch_targets writes it (backbone.py:518-520), read from the image and never
 * stored.  pred fp16 [b n][P].  The difference is one fp32 subtraction, the sum takes it by fma (the square is not
 * rounded); plan and summation order are hcir_mim_l1_fwd's.  The gradient of the loss is 2 grad_out / (b n P) * diff:
 * there is no backward kernel. */
int hcir_mae_mse_fwd(const void* pred, const float* img, int64_t b, int32_t c, int32_t h, int32_t w, int32_t ps,
                     const int64_t* idx, int32_t n, float* loss, void* diff, void* workspace, size_t workspace_bytes,
                     void* stream);
/* HOST.  blocks * 4 bytes for rows = b n. */
size_t hcir_mae_mse_workspace_bytes(int64_t rows);

#ifdef __cplusplus
}
#endif
#endif /* HCIR_H */
