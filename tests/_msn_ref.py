"""MSN restatements, error bounds, cases and mutations (TEST INFRASTRUCTURE ONLY), in the manner of
tests/_densecl_ref.py.

lightly is not installed and not in the reference tree: the semantics below restate lightly's public sources
(lightly.loss.MSNLoss: prototype_probabilities, sharpen, sinkhorn, forward) and are pinned by tests/test_msn_host.py to
torch's own ops (F.softmax, F.normalize, autograd) in float64.

  a_i, t_j, c_k  rows over max(norm, 1e-12)
  p_ik = softmax_k(a_i.c_k / T);  q_jk = softmax_k(t_j.c_k / (T Ts));  sinkhorn(q);  tgt = q repeated V times
  loss = mean_i sum_k -tgt_ik log p_ik + w (sum_k pbar_k log pbar_k + log K),  pbar = mean_i p_i
  G_ik = (p_ik (sum_k tgt_ik + w (log pbar_k - e_i)) - tgt_ik) / N,  e_i = sum_k p_ik log pbar_k
  danchors_i = (g_i - (g_i.a_i) a_i) / max(||anchors_i||, 1e-12),  g_i = sum_k G_ik c_k / T
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from oracle.ntxent import U_ROUND, err_over_bound  # noqa: F401  (re-exported for the tests)

U32 = 2.0 ** -24
T_DEFAULT, TS_DEFAULT = 0.1, 0.25

# (B, V, K, D): a ragged row block and a ragged column tile; 130 rows across a 128-row block at the workload's K and
# D; D off the LDS-DMA path (72: no multiple of 64 / 32); a target tile boundary (130 targets)
CASES = [(5, 3, 136, 8), (65, 2, 1024, 256), (3, 12, 264, 72), (130, 1, 1024, 64)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
FAMILIES = ("gauss", "scaled", "peaked", "tied", "zero_rows")
# (sinkhorn_iterations, regularization_weight) per family: every family at lightly's defaults, the Gaussian rows at
# the three other corners
CONFIGS = {f: [(3, 1.0)] for f in FAMILIES}
CONFIGS["gauss"] = [(3, 1.0), (0, 0.0), (0, 1.0), (3, 0.0)]


def table():
    """Every (case, family, iterations, weight) the device test runs and the host mutations must be seen on."""
    return [(c, f, it, w) for c in CASES for f in FAMILIES for (it, w) in CONFIGS[f]]


def make_inputs(case, family, dtype, seed: int = 0):
    """(anchors [N, D], targets [B, D]) in `dtype`, prototypes fp32 [K, D]; CPU tensors."""
    b, v, k, d = case
    n = b * v
    g = torch.Generator().manual_seed(1000003 * b + 7919 * k + 31 * d + 17 * FAMILIES.index(family) + seed)
    protos = F.normalize(torch.randn(k, d, generator=g), dim=-1)
    anchors = torch.randn(n, d, generator=g)
    targets = torch.randn(b, d, generator=g)
    if family == "scaled":            # non-unit prototypes: a kernel that forgets to normalise them is caught
        protos = protos * 3.0
    elif family == "peaked":          # anchors nearly collinear with one prototype
        idx = torch.randint(0, k, (n,), generator=g)
        anchors = protos[idx] * (0.5 + torch.rand(n, 1, generator=g)) + 0.01 * anchors
    elif family == "tied":            # two prototypes nearly tied for a target
        i0 = torch.randint(0, k, (b,), generator=g)
        i1 = (i0 + 1 + torch.randint(0, k - 1, (b,), generator=g)) % k
        targets = protos[i0] + protos[i1] + 1e-3 * targets
    elif family == "zero_rows":       # the 1e-12 clamp
        anchors[n // 2] = 0.0
        targets[b // 2] = 0.0
    return anchors.to(dtype), targets.to(dtype), protos.float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------
def _unit(z):
    return z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)


def sinkhorn_f64(q, iterations: int):
    """lightly.loss.msn_loss.sinkhorn on one process, float64."""
    if iterations <= 0:
        return q
    b, k = q.shape
    qq = q.t() / q.sum()
    for _ in range(iterations):
        qq = qq / qq.sum(dim=1, keepdim=True)
        qq = qq / k
        qq = qq / qq.sum(dim=0, keepdim=True)
        qq = qq / b
    return (qq * b).t()


class MsnRef(NamedTuple):
    loss: torch.Tensor
    ce: torch.Tensor
    reg: torch.Tensor      # without its weight
    a: torch.Tensor        # [N, D] unit anchors
    c: torch.Tensor        # [K, D] unit prototypes
    s: torch.Tensor        # [N, K] anchor logits / T
    st: torch.Tensor       # [B, K] target logits / (T Ts)
    lse: torch.Tensor      # [N]
    p: torch.Tensor        # [N, K]
    q0: torch.Tensor       # [B, K] sharpened softmax
    q: torch.Tensor        # [B, K] after Sinkhorn
    tgt: torch.Tensor      # [N, K]
    pbar: torch.Tensor     # [K]


def msn_f64(anchors, targets, protos, t=T_DEFAULT, ts=TS_DEFAULT, iterations=3, weight=1.0, mutation=None) -> MsnRef:
    """The restatement in float64; differentiable in `anchors`.  `mutation` names one deliberate mistake."""
    a, tt = _unit(anchors.double()), _unit(targets.double())
    c = protos.double() if mutation == "prototype_unnormalised" else _unit(protos.double())
    n, b, k = a.shape[0], tt.shape[0], c.shape[0]
    s = a @ c.t() / t
    st = tt @ c.t() / (t if mutation == "no_sharpen" else t * ts)
    lse = torch.logsumexp(s, dim=1)
    p = torch.exp(s - lse[:, None])
    q0 = torch.softmax(st.detach(), dim=1)
    if mutation == "sinkhorn_step_dropped" and iterations > 0:
        qq = q0.t() / q0.sum()
        for it in range(iterations):
            qq = qq / qq.sum(dim=1, keepdim=True) / k
            if it != iterations - 1:
                qq = qq / qq.sum(dim=0, keepdim=True)
            qq = qq / b
        q = (qq * b).t()
    else:
        q = sinkhorn_f64(q0, iterations)
    if mutation == "wrong_pairing":       # row i with target i // V, the other plausible layout
        tgt = q.repeat_interleave(n // b, dim=0)
    else:
        tgt = q.repeat(n // b, 1)
    ce = (-tgt * (s - lse[:, None])).sum(1).mean()
    pbar = p.mean(0)
    reg = (pbar * torch.log(pbar)).sum()
    if mutation != "no_log_k":
        reg = reg + math.log(k)
    if mutation == "regulariser_sign":
        reg = -reg
    return MsnRef(ce + weight * reg, ce, reg, a, c, s, st, lse, p, q0, q, tgt, pbar)


MUTATIONS = ("prototype_unnormalised", "no_log_k", "regulariser_sign", "sinkhorn_step_dropped", "wrong_pairing",
             "no_sharpen")


def msn_literal_f64(anchors, targets, protos, t=T_DEFAULT, ts=TS_DEFAULT, iterations=3, weight=1.0):
    """lightly's forward line by line on torch primitives (F.normalize, F.softmax, ** (1 / Ts), repeat, log of
    pbar ** -pbar), float64."""
    anchors, targets, protos = anchors.double(), targets.double(), protos.double()
    num_views = anchors.shape[0] // targets.shape[0]
    anchors = F.normalize(anchors, dim=1)
    targets = F.normalize(targets, dim=1)
    protos = F.normalize(protos, dim=1)
    anchor_probs = F.softmax(anchors @ protos.t() / t, dim=1)
    with torch.no_grad():
        target_probs = F.softmax(targets @ protos.t() / t, dim=1)
        target_probs = target_probs ** (1.0 / ts)
        target_probs = target_probs / target_probs.sum(dim=1, keepdim=True)
        if iterations > 0:
            target_probs = sinkhorn_f64(target_probs, iterations)
        target_probs = target_probs.repeat((num_views, 1))
    loss = torch.mean(torch.sum(torch.log(anchor_probs ** (-target_probs)), dim=1))
    if weight > 0:
        mean_anchor_probs = torch.mean(anchor_probs, dim=0)
        reg = -torch.sum(torch.log(mean_anchor_probs ** (-mean_anchor_probs)))
        reg = reg + math.log(float(len(mean_anchor_probs)))
        loss = loss + weight * reg
    return loss


def grads_f64(anchors, targets, protos, t=T_DEFAULT, ts=TS_DEFAULT, iterations=3, weight=1.0, grad_out=1.0,
              mutation=None):
    """dL/danchors * grad_out by float64 autograd through the restatement."""
    x = anchors.detach().double().requires_grad_(True)
    (msn_f64(x, targets, protos, t, ts, iterations, weight, mutation).loss * grad_out).backward()
    return x.grad


def closed_form_grad(ref: MsnRef, anchors, t=T_DEFAULT, weight=1.0, grad_out=1.0):
    """The backward the kernels implement, in float64."""
    n = ref.p.shape[0]
    lp = torch.log(ref.pbar)
    e = (ref.p * lp[None, :]).sum(1, keepdim=True)
    gm = (ref.p * (ref.tgt.sum(1, keepdim=True) + weight * (lp[None, :] - e)) - ref.tgt) / n
    g = gm @ ref.c / t
    rn = 1.0 / anchors.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    return grad_out * rn * (g - (g * ref.a).sum(1, keepdim=True) * ref.a)


# ---------------------------------------------------------------------------------------------------------------------
# Bounds of hcir_msn_targets / _fwd / _bwd against the float64 restatement taken on the inputs the kernels read
# (anchors and targets already rounded to the tested dtype, the prototypes fp32).  Every term counts roundings of the
# kernels' arithmetic; 2^-24 is the unit roundoff of fp32, u_c that of the compute dtype for the prototypes (0 in
# fp32).  The anchors and targets enter the MFMA as given (no rounding) and are scaled by their fp32 inverse norm after.
#
#   nrm(D)  = (ceil(D/64) + 6) / 2 + 3      fp32 roundings in an inverse norm / a normalised element (tests/_densecl_ref)
#   acc(D)  = D (fp32 MFMA: a k-ordered fmaf chain) or ceil(D/16) + 1 (16-bit MFMA: one rounding each)
#   cos     E_ik = [u_c + (2 nrm + acc + 4) 2^-24] (1 + 2^-6) sum_d |a_id| |c_kd|      the prototype rounded after its
#             normalisation, the row's inverse norm, the accumulation, 4 for inv_t, log2(e), their product and the multiply
#   logits  d_ik = E_ik / T (anchors), E_jk / (T Ts) (targets)
#   q0      |log q0~ - log q0|_jk <= b0_jk = d_jk + max_k d_jk + 4 2^-24 (|st_jk| + max_k |st_jk|) + (ceil(K/64) + 16) 2^-24
#             numerator and denominator of the softmax, the subtraction in exp2's argument, exp2 at 2 ulp, the lane
#             chain and wave sum, reciprocal, multiply
#   q       Sinkhorn on scaling vectors: a sum of positive terms moves (in log) by at most the largest move of a term,
#             so with eps = max_jk b0: u_1 moves by eps, v_1 by 2 eps, ..., u_m by (2m - 1) eps, and
#             q = u q0 / sum u q0 by 4 m eps; each of the 2 m sums adds (B/4 + K/64 + 12) 2^-24 of its own:
#             bq = 4 m eps + 2 m (ceil(B/4) + ceil(K/64) + 12) 2^-24          (m = 0: bq_jk = b0_jk)
#             |q~ - q| <= q expm1(bq) + 2^-126
#   lse     max_k d_ik + (64 + 3 (ceil(K/128) + 1)) 2^-24 + 6 2^-24 |lse_i|                    (tests/_densecl_ref)
#   p       |log p~ - log p|_ik <= pi_ik = d_ik + lse_i bound + 4 2^-24 (|s_ik| + |lse_i|) + 2^-22
#   pbar    |pbar~ - pbar|_k <= pbar_k (expm1(max_i pi_ik) + (ceil(N/128) + 48) 2^-24)
#   ce      mean_i [ sum_k dq_ik |lse_i - s_ik| + sum_k tgt_ik (d_ik + lse_i bound)
#                    + (ceil(K/128) + 44) 2^-24 (|lse_i| sum_k tgt_ik + sum_k tgt_ik |s_ik|) ]      the kernel forms
#             lse sum tgt - sum tgt s: 32 fmaf per lane, 4 partials, one add per tile, the multiply, the subtraction
#             + (ceil(N/1024) + 12) 2^-24 mean_i |ce_i|
#   reg     sum_k dpbar_k |1 + log pbar_k| + (ceil(K/1024) + 16) 2^-24 sum_k |pbar_k log pbar_k| + 4 2^-24 log K
#   loss    ce bound + |w| reg bound + 2 2^-24 (|ce| + |w reg|)
#   grad    dG_ik = dp_ik (tq_i + |w| |lp_k - e_i|) + p_ik (dtq_i + |w| (dlp_k + de_i)) + dq_ik
#                   + (2^-11 + 8 2^-24) |G_ik| + 2^-25                 its fp16 image
#             dp = p expm1(pi), dlp_k = dpbar_k / pbar_k + 2^-22, dtq_i = sum_k dq_ik + (ceil(K/128) + 36) 2^-24 tq_i,
#             de_i = sum_k (dp_ik |lp_k| + p_ik dlp_k) + (ceil(K/128) + 40) 2^-24 sum_k p_ik |lp_k|
#           g = G.c on hcir_gemm_f16: Eg = dG |c| + (2^-11 + (ceil(K/16) + 6) 2^-24) |G| |c| + 2^-25 sum_k |G_ik|
#           through the projection (tests/_densecl_ref._projected's, the row in fp32):
#             coef rn_i (Eg + |a| sum_d Eg |a| + 4 u_p |g.a| |a|) + (u_T + (nrm + 8) 2^-24) |ref| + qsub
# ---------------------------------------------------------------------------------------------------------------------
def nrm(d):
    return (math.ceil(d / 64) + 6) / 2 + 3


def acc(d, dtype):
    return d if dtype == torch.float32 else math.ceil(d / 16) + 1


def u_c_of(dtype):
    return 0.0 if dtype == torch.float32 else U_ROUND[dtype]


def cos_bound(rows_unit, c_unit, dtype):
    d = c_unit.shape[1]
    rel = (u_c_of(dtype) + (2 * nrm(d) + acc(d, dtype) + 4) * U32) * (1 + 2.0 ** -6)
    return rel * (rows_unit.abs() @ c_unit.abs().t())


class MsnBounds(NamedTuple):
    q: torch.Tensor       # [B, K] absolute
    lse: torch.Tensor     # [N]
    pbar: torch.Tensor    # [K]
    ce: torch.Tensor
    reg: torch.Tensor
    loss: torch.Tensor
    grad: torch.Tensor    # [N, D]


def bounds(ref: MsnRef, anchors, targets, dtype, t=T_DEFAULT, ts=TS_DEFAULT, iterations=3, weight=1.0,
           grad_out=1.0) -> MsnBounds:
    n, k = ref.p.shape
    b = ref.q.shape[0]
    d = ref.c.shape[1]
    w = abs(weight)
    nct = math.ceil(k / 128)
    tu = _unit(targets.double())
    # targets
    dt_ = cos_bound(tu, ref.c, dtype) / (t * ts)
    b0 = dt_ + dt_.max(1, keepdim=True).values + 4 * U32 * (ref.st.abs() + ref.st.abs().max(1, keepdim=True).values) \
        + (math.ceil(k / 64) + 16) * U32
    if iterations > 0:
        bq = 4 * iterations * b0.max() + 2 * iterations * (math.ceil(b / 4) + math.ceil(k / 64) + 12) * U32
        bq = torch.full_like(b0, float(bq))
    else:
        bq = b0
    dq = ref.q * torch.expm1(bq) + 2.0 ** -126
    dtgt = dq.repeat(n // b, 1)
    # anchors
    da = cos_bound(ref.a, ref.c, dtype) / t
    lse_b = da.max(1).values + (64 + 3 * (nct + 1)) * U32 + 6 * U32 * ref.lse.abs()
    pi = da + lse_b[:, None] + 4 * U32 * (ref.s.abs() + ref.lse.abs()[:, None]) + 2.0 ** -22
    dp = ref.p * torch.expm1(pi)
    dpbar = ref.pbar * (torch.expm1(pi.max(0).values) + (math.ceil(n / 128) + 48) * U32)
    tq = ref.tgt.sum(1)
    row_ce = (-ref.tgt * (ref.s - ref.lse[:, None])).sum(1)
    ce_rows = (dtgt * (ref.lse[:, None] - ref.s).abs()).sum(1) + (ref.tgt * (da + lse_b[:, None])).sum(1) \
        + (nct + 44) * U32 * (ref.lse.abs() * tq + (ref.tgt * ref.s.abs()).sum(1))
    ce_b = ce_rows.mean() + (math.ceil(n / 1024) + 12) * U32 * row_ce.abs().mean() + 2.0 ** -149
    lp = torch.log(ref.pbar)
    reg_b = (dpbar * (1 + lp).abs()).sum() + (math.ceil(k / 1024) + 16) * U32 * (ref.pbar * lp).abs().sum() \
        + 4 * U32 * math.log(k)
    loss_b = ce_b + w * reg_b + 2 * U32 * (ref.ce.abs() + w * ref.reg.abs())
    # gradient
    e = (ref.p * lp[None, :]).sum(1)
    gm = ref.p * (tq[:, None] + weight * (lp[None, :] - e[:, None])) - ref.tgt
    dlp = dpbar / ref.pbar + 2.0 ** -22
    dtq = dtgt.sum(1) + (nct + 36) * U32 * tq
    de = (dp * lp.abs()[None, :] + ref.p * dlp[None, :]).sum(1) + (nct + 40) * U32 * (ref.p * lp.abs()[None, :]).sum(1)
    dg = dp * (tq[:, None] + w * (lp[None, :] - e[:, None]).abs()) \
        + ref.p * (dtq[:, None] + w * (dlp[None, :] + de[:, None])) + dtgt \
        + (2.0 ** -11 + 8 * U32) * gm.abs() + 2.0 ** -25
    ac = ref.c.abs()
    eg = dg @ ac + (2.0 ** -11 + (math.ceil(k / 16) + 6) * U32) * (gm.abs() @ ac) \
        + 2.0 ** -25 * gm.abs().sum(1, keepdim=True)
    g = gm @ ref.c
    coef = abs(grad_out) / (t * n)
    rn = 1.0 / anchors.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    au = ref.a.abs()
    u_p = (2 * nrm(d) + math.ceil(d / 64) + 8) * U32
    gu = (g * ref.a).sum(1, keepdim=True)
    d_ref = coef * rn * (g - gu * ref.a)
    qsub = (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -30) * abs(grad_out)
    grad_b = coef * rn * (eg + au * (eg * au).sum(1, keepdim=True) + 4 * u_p * gu.abs() * au) \
        + (U_ROUND[dtype] + (nrm(d) + 8) * U32) * d_ref.abs() + qsub
    return MsnBounds(dq, lse_b, dpbar, ce_b, reg_b, loss_b, grad_b)


QUANTITIES = ("q", "row_lse", "pbar", "ce", "reg", "loss", "danchors")


def verdicts(out: dict, ref: MsnRef, bd: MsnBounds, grad_ref, dtype) -> dict:
    """err / bound (worst element) of each quantity in `out` (CPU tensors): q, row_lse, pbar, ce, reg, loss, danchors."""
    r = {
        "q": err_over_bound(out["q"], ref.q, bd.q),
        "row_lse": err_over_bound(out["row_lse"], ref.lse, bd.lse),
        "pbar": err_over_bound(out["pbar"], ref.pbar, bd.pbar),
        "ce": err_over_bound(out["ce"], ref.ce, bd.ce),
        "reg": err_over_bound(out["reg"], ref.reg, bd.reg),
        "loss": err_over_bound(out["loss"], ref.loss, bd.loss),
    }
    if "danchors" in out:
        r["danchors"] = err_over_bound(out["danchors"], grad_ref, bd.grad, dtype)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# The model: lightly's MaskedVisionTransformerTorchvision.forward(images, idx_keep) and MSNProjectionHead, restated
# from their public sources on a state dict (torchvision's layout), in whatever dtype it is handed.  PARITY UNPINNED,
# as tests/_mim_ref.py says of SimMIM: neither lightly nor torchvision is installed.
# ---------------------------------------------------------------------------------------------------------------------
def interpolate_pos_encoding(pos, npatch: int):
    """lightly's interpolate_pos_encoding: the class row as it is, the [1, d, g0, g0] patch grid through
    F.interpolate(scale_factor=sqrt(npatch / N0), mode="bicubic")."""
    n0 = pos.shape[1] - 1
    if npatch == n0:
        return pos
    d, g0 = pos.shape[-1], int(math.sqrt(n0))
    grid = F.interpolate(pos[:, 1:].reshape(1, g0, g0, d).permute(0, 3, 1, 2), scale_factor=math.sqrt(npatch / n0),
                         mode="bicubic")
    return torch.cat((pos[:, 0].unsqueeze(0), grid.permute(0, 2, 3, 1).reshape(1, -1, d)), dim=1)


def masked_vit_cls(sd, images, idx_keep=None, num_heads=12, p="anchor_backbone.vit."):
    """forward(images, idx_keep): patch embedding, class token, the position (interpolated for another grid) added
    once, get_at_index(idx_keep), the blocks, encoder.ln, the class token out."""
    import _mim_ref as mim
    from oracle import vit as ovit
    x = mim.images_to_tokens(sd, images, p)
    x = torch.cat((sd[p + "class_token"].expand(x.shape[0], -1, -1), x), 1)
    x = x + interpolate_pos_encoding(sd[p + "encoder.pos_embedding"], x.shape[1] - 1)
    if idx_keep is not None:
        x = mim.get_at_index(x, idx_keep)
    i = 0
    while f"{p}encoder.layers.encoder_layer_{i}.ln_1.weight" in sd:
        x = ovit._tv_encoder_block(sd, f"{p}encoder.layers.encoder_layer_{i}.", x, num_heads)
        i += 1
    x = F.layer_norm(x, (x.shape[-1],), sd[p + "encoder.ln.weight"], sd[p + "encoder.ln.bias"], 1e-6)
    return x[:, 0]


def projection_head(sd, x, p="anchor_projection_head.", eps=1e-5):
    """MSNProjectionHead in train mode: BatchNorm1d on the batch's own statistics (biased variance)."""
    for i in (0, 3):
        x = F.linear(x, sd[f"{p}layers.{i}.weight"])
        x = F.batch_norm(x, None, None, sd[f"{p}layers.{i + 1}.weight"], sd[f"{p}layers.{i + 1}.bias"], True, 0.0, eps)
        x = F.gelu(x)
    return F.linear(x, sd[f"{p}layers.6.weight"], sd[f"{p}layers.6.bias"])


def msn_step_loss(sd, views, keeps, num_heads, t=T_DEFAULT, ts=TS_DEFAULT, iterations=3, weight=1.0):
    """The loss of the reference's MSN step on given views and masks: views[0] through the target pair, views[1]
    through forward_masked, views[2:] concatenated through a second forward_masked call; keeps = (idx_keep of the
    anchors, idx_keep of the focal batch or None).  The restatement's dtype is the state dict's."""
    with torch.no_grad():
        tgt = projection_head(sd, masked_vit_cls(sd, views[0], None, num_heads, "backbone.vit."), "projection_head.")
    outs = [projection_head(sd, masked_vit_cls(sd, views[1], keeps[0], num_heads))]
    if len(views) > 2:
        outs.append(projection_head(sd, masked_vit_cls(sd, torch.cat(list(views[2:]), 0), keeps[1], num_heads)))
    anchors = torch.cat(outs, 0)
    ref = msn_f64(anchors, tgt, sd["prototypes"].detach(), t, ts, iterations, weight)
    return ref.loss, anchors, tgt


def msn_loss_torch(anchors, targets, protos, t=T_DEFAULT, ts=TS_DEFAULT, iterations=3, weight=1.0):
    """lightly's forward as plain torch in the tensors' own dtype and device (what runs under autocast in the
    reference: the e_ref side of the model tests and the torch side of tools/bench_msn.py)."""
    num_views = anchors.shape[0] // targets.shape[0]
    anchors, targets, protos = F.normalize(anchors, dim=1), F.normalize(targets, dim=1), F.normalize(protos, dim=1)
    anchor_probs = F.softmax(torch.matmul(anchors, protos.t()) / t, dim=1)
    with torch.no_grad():
        target_probs = F.softmax(torch.matmul(targets, protos.t()) / t, dim=1)
        target_probs = target_probs ** (1.0 / ts)
        target_probs = target_probs / target_probs.sum(dim=1, keepdim=True)
        if iterations > 0:
            b, k = target_probs.shape
            qq = target_probs.t() / target_probs.sum()
            for _ in range(iterations):
                qq = qq / qq.sum(dim=1, keepdim=True)
                qq = qq / k
                qq = qq / qq.sum(dim=0, keepdim=True)
                qq = qq / b
            target_probs = (qq * b).t()
        target_probs = target_probs.repeat((num_views, 1))
    loss = torch.mean(torch.sum(torch.log(anchor_probs ** (-target_probs)), dim=1))
    if weight > 0:
        mean_anchor_probs = torch.mean(anchor_probs, dim=0)
        reg = -torch.sum(torch.log(mean_anchor_probs ** (-mean_anchor_probs)))
        loss = loss + weight * (reg + math.log(float(len(mean_anchor_probs))))
    return loss
