"""DenseCL restatements, error bounds, kernel emulation and mutations (TEST INFRASTRUCTURE ONLY), in the manner of
tests/_supcon_ref.py.

lightly is not installed and not in the reference tree: the semantics below restate lightly's public sources
(lightly.loss.NTXentLoss with a memory bank, lightly.models.utils.select_most_similar) and are pinned by
tests/test_densecl_host.py to torch's own ops in float64.

  bank loss   q_i = z0_i / max(||z0_i||, 1e-12), k_i = z1_i / max(||z1_i||, 1e-12), i < N;  bank [K, D] as stored
              logits_i = [q_i.k_i, q_i.bank_0, .., q_i.bank_{K-1}] / T;  loss = mean_i (logsumexp(logits_i) - logits_i0)
              p_ij = exp(logit_ij - lse_i);  dq_i = (1 / (T N)) (sum_j p_ij bank_j + (p_i0 - 1) k_i),
              dk_i = (1 / (T N)) (p_i0 - 1) q_i, through rn_i (g_i - (g_i.u_i) u_i); no gradient to the bank
  match       j*(b, n) = argmax_m x_bn . y_bm / max(||y_bm||, 1e-12) (lowest m on a tie), out = y_values[b, j*]
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from oracle.ntxent import U_ROUND, err_over_bound, make_inputs  # noqa: F401  (re-exported for the tests)

_LOG2E = 1.44269504088896340736
_LN2 = 0.69314718055994530942
U32 = 2.0 ** -24

# (N, K, D): one row, below one tile, N off the tile, K one past a tile, both past a tile and D off the LDS-DMA
# path (72, 136: no multiple of 64 / 32), more than two tiles each way
CASES = [(1, 8, 8), (8, 120, 64), (74, 128, 72), (128, 136, 8), (136, 520, 136), (264, 264, 64)]
TEMPERATURES = (0.5, 0.07)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# "scaled_bank": the rows of "norms" against a bank whose rows are NOT unit rows (row j times a factor rising from 0.5
# to 2 over the bank): what separates "bank rows used as stored" from a kernel that renormalises them
MAIN_FAMILIES = ("exact", "norms", "exact_norms", "scaled_bank")
DEGENERATE_FAMILIES = ("collapsed", "same", "zero_row")   # zero_row: forward only (F.normalize's gradient at 0)


def has_backward(case):
    """hcir_gemm_f16's rule for its inner dimension, the bank; the row count is free."""
    return case[1] % 8 == 0


def u_in_of(family, dtype):
    """Rounding of the normalised rows into the compute dtype: none where they are exact in every dtype."""
    return U32 if family in ("exact", "exact_norms") else U_ROUND[dtype]


def u_bank_of(dtype):
    """Rounding of the fp32 bank into the compute dtype."""
    return 0.0 if dtype == torch.float32 else U_ROUND[dtype]


def make_bank(k: int, d: int, seed: int = 0, scaled: bool = False) -> torch.Tensor:
    """fp32 [K, D]: unit rows, as the module initialises its bank; scaled: row j times linspace(0.5, 2, K)[j]."""
    g = torch.Generator().manual_seed(7919 * k + 31 * d + seed)
    bank = F.normalize(torch.randn(k, d, generator=g), dim=-1)
    return bank * torch.linspace(0.5, 2.0, k)[:, None] if scaled else bank


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------
class BankRef(NamedTuple):
    loss: torch.Tensor      # scalar
    row_loss: torch.Tensor  # [N]
    lse: torch.Tensor       # [N]
    pos: torch.Tensor       # [N] positive logit
    q: torch.Tensor         # [N, D] normalised query rows
    k: torch.Tensor         # [N, D] normalised key rows
    p: torch.Tensor         # [N, K] softmax over the bank columns
    p0: torch.Tensor        # [N] softmax of the positive
    neg: torch.Tensor       # [N, K] bank logits
    bank: torch.Tensor      # [K, D] float64


def _unit(z):
    return z / z.norm(dim=1, keepdim=True).clamp_min(1e-12)


def bank_loss_f64(z0, z1, bank, t, full: bool = False):
    """float64 loss (full: a BankRef) of [N, D] rows against an fp32 / float64 [K, D] bank."""
    q, k = _unit(z0.double()), _unit(z1.double())
    bank = bank.double()
    pos = (q * k).sum(1) / t
    neg = q @ bank.t() / t
    lse = torch.logsumexp(torch.cat([pos[:, None], neg], 1), dim=1)
    row = lse - pos
    if not full:
        return row.mean()
    return BankRef(row.mean(), row, lse, pos, q, k, torch.exp(neg - lse[:, None]), torch.exp(pos - lse), neg, bank)


def bank_grads_f64(z0, z1, bank, t, grad_out: float = 1.0):
    """(dL/dz0, dL/dz1) * grad_out by float64 autograd."""
    a0 = z0.detach().double().requires_grad_(True)
    a1 = z1.detach().double().requires_grad_(True)
    (bank_loss_f64(a0, a1, bank, t) * grad_out).backward()
    return a0.grad, a1.grad


def closed_form_grads(ref: BankRef, z0, z1, t, grad_out: float = 1.0, p=None, p0=None, key_grad: bool = True):
    """The backward the kernels implement, in float64."""
    p = ref.p if p is None else p
    p0 = ref.p0 if p0 is None else p0
    n = ref.q.shape[0]
    c = grad_out / (t * n)
    gq = p @ ref.bank + (p0 - 1.0)[:, None] * ref.k
    gk = (p0 - 1.0)[:, None] * ref.q if key_grad else torch.zeros_like(ref.q)
    rn0 = 1.0 / z0.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    rn1 = 1.0 / z1.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    return (c * rn0 * (gq - (gq * ref.q).sum(1, keepdim=True) * ref.q),
            c * rn1 * (gk - (gk * ref.k).sum(1, keepdim=True) * ref.k))


def match_scores_f64(x, y):
    """[B, N, M] float64 scores x_bn . y_bm / max(||y_bm||, 1e-12)."""
    x, y = x.double(), y.double()
    return torch.bmm(x, (y / y.norm(dim=2, keepdim=True).clamp_min(1e-12)).transpose(1, 2))


def select_most_similar_f64(x, y, y_values, scores=None):
    """(idx int64 [B, N], out [B, N, Dv]): the lowest index on a tie."""
    s = match_scores_f64(x, y) if scores is None else scores
    best = s.max(dim=2, keepdim=True).values
    m = s.shape[2]
    idx = torch.where(s == best, torch.arange(m).expand_as(s), torch.full_like(s, m, dtype=torch.int64)).min(2).values
    return idx, torch.gather(y_values, 1, idx.unsqueeze(-1).expand(-1, -1, y_values.shape[2]))


def match_bound(x, y):
    """[B, N, M]: (C + 16) 2^-24 sum_c |x_c| |yhat_c|, yhat = y / ||y||.  C: one fp32 rounding per channel of the
    accumulation at most (the fp16 MFMA rounds once per 16 channels); 16: the key's sum of squares (a lane's chain and
    the six steps of the wave sum), square root, reciprocal and the one multiply."""
    c = x.shape[2]
    ax, ay = x.double().abs(), y.double().abs()
    return (c + 16) * U32 * torch.bmm(ax, (ay / y.double().norm(dim=2, keepdim=True).clamp_min(1e-12)).transpose(1, 2))


def match_verdict(idx, x, y):
    """The dense-match rule of a kernel's idx [B, N] on fp16 inputs.  -> (worst (max - chosen) / bound over every
    (b, n), number of rows whose float64 top-two gap exceeds 2 bound and whose index is NOT the float64 arg-max,
    fraction of rows left to the weaker condition)."""
    s = match_scores_f64(x, y)
    bound = match_bound(x, y)
    idx = idx.long()
    ref_idx, _ = select_most_similar_f64(x, y, y.double(), scores=s)
    chosen = torch.gather(s, 2, idx.unsqueeze(-1)).squeeze(-1)
    best = torch.gather(s, 2, ref_idx.unsqueeze(-1)).squeeze(-1)
    b_chosen = torch.gather(bound, 2, idx.unsqueeze(-1)).squeeze(-1)
    b_best = torch.gather(bound, 2, ref_idx.unsqueeze(-1)).squeeze(-1)
    lim = torch.maximum(b_chosen, b_best)
    ratio = ((best - chosen) / lim.clamp_min(2.0 ** -1000)).max()
    ratio = torch.where((best - chosen).max() <= 0, torch.zeros(()).double(), ratio)
    if s.shape[2] > 1:
        top2 = s.topk(2, dim=2)
        second = top2.indices[..., 1]
        gap = top2.values[..., 0] - top2.values[..., 1]
        b_second = torch.gather(bound, 2, second.unsqueeze(-1)).squeeze(-1)
        strict = gap > 2 * torch.maximum(b_best, b_second)
    else:
        strict = torch.ones_like(idx, dtype=torch.bool)
    wrong = int((strict & (idx != ref_idx)).sum())
    return float(ratio), wrong, float((~strict).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# Bounds of hcir_ntxent_bank_fwd / _bwd against the float64 reference taken on the inputs the kernel reads (z0, z1
# already rounded to the tested dtype, the bank fp32).  Every term counts roundings of the kernels' arithmetic; u_T is
# the unit roundoff of the tested dtype, 2^-24 that of fp32.
#
#   nrm(D)   = (ceil(D/64) + 6) / 2 + 3  fp32 roundings in a normalised element: the sum of squares (a lane's fmaf chain
#              of ceil(D/64) steps, six steps of the wave sum; halved by the square root), the square root, the
#              reciprocal, the multiply
#   acc(D)   = D (fp32: v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain) or ceil(D/16) + 1 (16-bit: one rounding per
#              MFMA) roundings of the accumulation, each relative to sum_k |a_k| |b_k| <= ||a|| ||b||
#   e_neg    = [u_in + u_bank + (nrm + acc + 4) 2^-24] (1 + 2^-6)      relative error of a bank logit in units of
#              ||q_i|| ||bank_j|| / |T|: q rounded into the compute dtype after its fp32 normalisation, the bank rounded
#              into it, the accumulation, and 4 for inv_t as an fp32 number, log2(e), their product and the multiply;
#              (1 + 2^-6) covers the products of these terms (u <= 2^-8)
#   e_pos    = [2 u_in + (2 nrm + ceil(D/64) + 7 + 4) 2^-24] (1 + 2^-6)  the positive: two normalised rounded rows, the
#              prep kernel's fp32 dot (lane chain, wave sum), the same 4
#   lse_i    : max(e_pos_i, max_j e_neg_ij)                      a log-sum-exp moves by at most the largest move of a term
#              + (64 + 3 (ceil(K/128) + 1)) 2^-24                relative error of the sum of exp2: 2 x 16 adds and two
#                rescales per lane, 4 partials met in LDS (multiply, multiply, add each), one merge per bank tile and one
#                for the positive, exp2 at 2 ulp and the subtraction in its argument weighted by p (<= 1/e each)
#              + 6 2^-24 |lse_i|                                 log2, the add to the max, times ln 2; the constants
#   pos_i    : e_pos_i + 2^-24 |pos_i| + 2^-149
#   k_unit   : nrm 2^-24 |k| + 2^-140
#   row_i    : lse_i bound + e_pos_i + 3 2^-24 (|lse_i| + |pos_i|)
#   loss     : mean_i row_i + (ceil(N/1024) + 12) 2^-24 mean_i |row loss_i| + 2^-149     the fixed tree, the divide
#   grad     g_i = sum_j p_ij bank_j + (p_i0 - 1) k_i.   Element error:
#              E_ik = [2^-11 + 2^-11 + (ceil(K/16) + 6) 2^-24] (p |bank|)_ik     P and the bank rounded to fp16, the fp32
#                                                                               accumulation of hcir_gemm_f16, exp2
#                   + sum_j p_ij (e_neg_ij + lam_i) |bank_jk|                    relative error of p_ij: logit and lse
#                     lam_i = lse_i bound + 4 2^-24 |lse_i|                      (the saved lse, back to the log2 domain)
#                   + 2^-25 sum_j |bank_jk| + 2^-25 sum_j p_ij                   fp16 subnormal spacing of P and the bank
#                   + dp0_i |k_ik| + |p_i0 - 1| (u_in + (nrm + 2) 2^-24) |k_ik|  the positive's term: dp0_i = p_i0 (pos_i
#                     bound + lam_i + 4 2^-24 (|pos_i| + |lse_i|)) + 2^-23, k_i as rounded, the fmaf
#            key: E_ik = dp0_i |q_ik| + |p_i0 - 1| (u_in + (nrm + 2) 2^-24) |q_ik|
#            through the projection (oracle.ntxent.grad_bound's, u the rounded unit row):
#              c rn_i (E_ik + |u_ik| sum_m E_im |u_im| + 4 u_p |g_i.u_i| |u_ik|),  u_p = u_in + (nrm + ceil(D/64) + 8) 2^-24
#              + (u_T + (nrm + 8) 2^-24) |ref| + q       the store in the output dtype, rn and the coefficient in fp32;
#              q the output dtype's subnormal spacing times |grad_out|
# ---------------------------------------------------------------------------------------------------------------------
def nrm(d):
    return (math.ceil(d / 64) + 6) / 2 + 3


def acc(d, dtype):
    return d if dtype == torch.float32 else math.ceil(d / 16) + 1


def e_neg(ref: BankRef, t, dtype, u_in):
    d = ref.q.shape[1]
    rel = (u_in + u_bank_of(dtype) + (nrm(d) + acc(d, dtype) + 4) * U32) * (1 + 2.0 ** -6)
    return rel * ref.q.norm(dim=1)[:, None] * ref.bank.norm(dim=1)[None, :] / abs(t)


def e_pos(ref: BankRef, t, u_in):
    d = ref.q.shape[1]
    rel = (2 * u_in + (2 * nrm(d) + math.ceil(d / 64) + 11) * U32) * (1 + 2.0 ** -6)
    return rel * ref.q.norm(dim=1) * ref.k.norm(dim=1) / abs(t)


def lse_bound(ref: BankRef, t, dtype, u_in):
    k = ref.bank.shape[0]
    worst = torch.maximum(e_pos(ref, t, u_in), e_neg(ref, t, dtype, u_in).max(1).values)
    return worst + (64 + 3 * (math.ceil(k / 128) + 1)) * U32 + 6 * U32 * ref.lse.abs()


def pos_bound(ref: BankRef, t, u_in):
    return e_pos(ref, t, u_in) + U32 * ref.pos.abs() + 2.0 ** -149


def k_unit_bound(ref: BankRef):
    return nrm(ref.q.shape[1]) * U32 * ref.k.abs() + 2.0 ** -140


def row_loss_bound(ref: BankRef, t, dtype, u_in):
    return lse_bound(ref, t, dtype, u_in) + e_pos(ref, t, u_in) + 3 * U32 * (ref.lse.abs() + ref.pos.abs())


def loss_bound(ref: BankRef, t, dtype, u_in):
    n = ref.q.shape[0]
    return row_loss_bound(ref, t, dtype, u_in).mean() + (math.ceil(n / 1024) + 12) * U32 * ref.row_loss.abs().mean() \
        + 2.0 ** -149


def _projected(e, u, g, c, rn, d_ref, dtype, u_in, grad_out):
    d = u.shape[1]
    u_t = U_ROUND[dtype]
    u_p = u_in + (nrm(d) + math.ceil(d / 64) + 8) * U32
    au = u.abs()
    gu = (g * u).sum(1, keepdim=True)
    q = (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -30) * abs(grad_out)
    return c * rn * (e + au * (e * au).sum(1, keepdim=True) + 4 * u_p * gu.abs() * au) \
        + (u_t + (nrm(d) + 8) * U32) * d_ref.abs() + q


def grad_bounds(ref: BankRef, z0, z1, dz0_ref, dz1_ref, t, grad_out, dtype, u_in):
    """([N, D], [N, D]) bounds on |dz0 - dz0_ref| and |dz1 - dz1_ref|."""
    n, d = ref.q.shape
    k = ref.bank.shape[0]
    ab = ref.bank.abs()
    lam = lse_bound(ref, t, dtype, u_in) + 4 * U32 * ref.lse.abs()
    dp0 = ref.p0 * (pos_bound(ref, t, u_in) + lam + 4 * U32 * (ref.pos.abs() + ref.lse.abs())) + 2.0 ** -23
    c0 = (ref.p0 - 1.0).abs()
    u_row = u_in + (nrm(d) + 2) * U32
    e = (2.0 ** -10 + (math.ceil(k / 16) + 6) * U32) * (ref.p @ ab) \
        + (ref.p * (e_neg(ref, t, dtype, u_in) + lam[:, None])) @ ab \
        + 2.0 ** -25 * ab.sum(0, keepdim=True) + 2.0 ** -25 * ref.p.sum(1, keepdim=True) \
        + dp0[:, None] * ref.k.abs() + (c0 * u_row)[:, None] * ref.k.abs()
    ek = dp0[:, None] * ref.q.abs() + (c0 * u_row)[:, None] * ref.q.abs()
    c = abs(grad_out) / (abs(t) * n)
    rn0 = 1.0 / z0.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    rn1 = 1.0 / z1.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    gq = ref.p @ ref.bank + (ref.p0 - 1.0)[:, None] * ref.k
    gk = (ref.p0 - 1.0)[:, None] * ref.q
    return (_projected(e, ref.q, gq, c, rn0, dz0_ref, dtype, u_in, grad_out),
            _projected(ek, ref.k, gk, c, rn1, dz1_ref, dtype, u_in, grad_out))


class BankProblem(NamedTuple):
    z0: torch.Tensor                 # CPU, tested dtype
    z1: torch.Tensor
    bank: torch.Tensor               # CPU fp32 [K, D]
    ref: BankRef
    dz0: Optional[torch.Tensor]      # float64 gradients at grad_out = 1 (None without a backward)
    dz1: Optional[torch.Tensor]
    u_in: float


@functools.lru_cache(maxsize=None)
def problem(family, case, t, dtype) -> BankProblem:
    """Inputs and float64 reference of one problem, computed once and shared; treat as read-only."""
    n, k, d = case
    z0, z1 = make_inputs("norms" if family == "scaled_bank" else family, n, d)
    z0, z1 = z0.to(dtype), z1.to(dtype)
    bank = make_bank(k, d, scaled=family == "scaled_bank")
    ref = bank_loss_f64(z0, z1, bank, t, full=True)
    dz0 = dz1 = None
    if has_backward(case) and family != "zero_row":
        dz0, dz1 = bank_grads_f64(z0, z1, bank, t)
    return BankProblem(z0, z1, bank, ref, dz0, dz1, u_in_of(family, dtype))


# ---------------------------------------------------------------------------------------------------------------------
# Plain-torch emulation of the kernels' arithmetic and reduction order (CPU): what the bounds must cover.
# ---------------------------------------------------------------------------------------------------------------------
def emulate(z0, z1, bank, t, grad_out=1.0, backward=True, want_dz1=True):
    """fp32 normalise -> round to T; bank rounded to T; fp32 logits in the log2 domain; per 128-column bank tile an
    (max, sum of exp2) pair, merged in tile order, then the positive; P and the bank rounded to fp16; fp32 product;
    fp32 finish -> round to T.  Returns (loss, lse, pos, k_unit, dz0, dz1)."""
    dtype = z0.dtype
    n, d = z0.shape
    k = bank.shape[0]
    f32 = torch.float32
    a, b = z0.float(), z1.float()
    inv0 = 1.0 / torch.sqrt((a * a).sum(1)).clamp_min(1e-12)
    inv1 = 1.0 / torch.sqrt((b * b).sum(1)).clamp_min(1e-12)
    k_unit = b * inv1[:, None]
    qn, kn = (a * inv0[:, None]).to(dtype).float(), k_unit.to(dtype).float()
    bc = bank.to(dtype).float()
    inv_t = torch.tensor(1.0 / t, dtype=f32)
    scale = inv_t * torch.tensor(_LOG2E, dtype=f32)
    dot = (qn * kn).sum(1)
    x = (qn @ bc.t()) * scale
    ninf = float("-inf")
    m = torch.full((n,), ninf, dtype=f32)
    l = torch.zeros(n, dtype=f32)
    for c0 in range(0, k, 128):
        xt = x[:, c0:c0 + 128]
        mp = xt.max(1).values
        lp = torch.exp2(xt - mp[:, None]).sum(1)
        mn = torch.maximum(m, mp)
        l = l * torch.exp2(m - mn) + lp * torch.exp2(mp - mn)
        m = mn
    pv = dot * scale
    mn = torch.maximum(m, pv)
    l = l * torch.exp2(m - mn) + torch.exp2(pv - mn)
    lse2 = mn + torch.log2(l)
    ln2 = torch.tensor(_LN2, dtype=f32)
    lse, pos = lse2 * ln2, dot * inv_t
    loss = ((lse2 - pv) * ln2).sum() / n
    if not backward:
        return loss, lse, pos, k_unit, None, None
    lrow = lse * torch.tensor(_LOG2E, dtype=f32)
    pm = torch.exp2(x - lrow[:, None]).half().float()
    g = pm @ bank.half().float()
    c0 = torch.exp2((pos - lse) * torch.tensor(_LOG2E, dtype=f32)) - 1.0
    coef = torch.tensor(grad_out, dtype=f32) * inv_t / torch.tensor(float(n), dtype=f32)
    gq = g + c0[:, None] * kn
    dz0 = ((coef * inv0)[:, None] * (gq - (gq * qn).sum(1, keepdim=True) * qn)).to(dtype)
    dz1 = None
    if want_dz1:
        qk = (qn * kn).sum(1, keepdim=True)
        dz1 = ((coef * inv1 * c0)[:, None] * (qn - qk * kn)).to(dtype)
    return loss, lse, pos, k_unit, dz0, dz1


def emulate_match(x, y):
    """fp16 inputs: fp32 scores dot * (1 / max(||y||, 1e-12)), torch.argmax's lowest index on a tie."""
    xf, yf = x.float(), y.float()
    inv = 1.0 / torch.sqrt((yf * yf).sum(2)).clamp_min(1e-12)
    return (torch.bmm(xf, yf.transpose(1, 2)) * inv[:, None, :]).argmax(dim=2)


def enqueue(bank: torch.Tensor, ptr: int, k_unit: torch.Tensor):
    """lightly's queue rule on a [K, D] bank, out of place: -> (bank, ptr)."""
    bank = bank.clone()
    size, n = bank.shape[0], k_unit.shape[0]
    if ptr + n >= size:
        bank[ptr:] = k_unit[:size - ptr]
        return bank, 0
    bank[ptr:ptr + n] = k_unit
    return bank, ptr + n


# ---------------------------------------------------------------------------------------------------------------------
# Mutations: the factor by which a kernel (or host) that makes a specific mistake misses the bound - the loss for the
# forward's mistakes, the worst gradient element for the backward's.  inf = the mistake cannot be made here.
#   last_col_dropped  bank column K - 1 excluded          extra_col     column K included (the clamped read of row K - 1
#                                                                       counted once more)
#   pos_twice         the positive counted twice in the log-sum-exp
#   bank_renormalised the bank rows renormalised (the "scaled_bank" family of the table shows it; on unit rows the
#                     mistake moves the loss by a rounding of the norms only)
#   stale_bank        the loss taken against the bank AFTER the enqueue of this call's keys
#   bank_grad_rows    (backward) the positive key treated as a bank row: no gradient to z1
#   no_pos_in_dq      (backward) the (p_i0 - 1) k_i term missing from dq
# Dense match (on an exact integer family, as index disagreements with the reference): tie_high, x_norm
# ---------------------------------------------------------------------------------------------------------------------
def mutation_factors(pr: BankProblem, case, t, dtype):
    ref = pr.ref
    n, k, d = case
    lb = loss_bound(ref, t, dtype, pr.u_in)
    inf = float("inf")

    def loss_factor(neg, pos=None, extra=None):
        pos = ref.pos if pos is None else pos
        cols = [pos[:, None], neg] + ([extra] if extra is not None else [])
        row = torch.logsumexp(torch.cat(cols, 1), dim=1) - pos
        return float((row.mean() - ref.loss).abs() / lb)

    out = {}
    out["last_col_dropped"] = loss_factor(ref.neg[:, :-1]) if k > 1 else inf
    out["extra_col"] = loss_factor(ref.neg, extra=ref.neg[:, -1:])
    out["pos_twice"] = loss_factor(ref.neg, extra=ref.pos[:, None])
    # the GPU test holds every row_lse element: the worst row, or the loss where that shows more
    renorm = ref.q @ _unit(ref.bank).t() / t
    lse_mut = torch.logsumexp(torch.cat([ref.pos[:, None], renorm], 1), dim=1)
    out["bank_renormalised"] = max(loss_factor(renorm),
                                   float(((lse_mut - ref.lse).abs() / lse_bound(ref, t, dtype, pr.u_in)).max()))
    after, _ = enqueue(ref.bank, 0, ref.k)
    out["stale_bank"] = loss_factor(ref.q @ after.t() / t)
    if pr.dz0 is not None:
        b0, b1 = grad_bounds(ref, pr.z0, pr.z1, pr.dz0, pr.dz1, t, 1.0, dtype, pr.u_in)
        m0, m1 = closed_form_grads(ref, pr.z0, pr.z1, t, key_grad=False)
        out["bank_grad_rows"] = float(((m1 - pr.dz1).abs() / b1).max())
        gq = ref.p @ ref.bank
        rn0 = 1.0 / pr.z0.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
        m0 = (1.0 / (t * n)) * rn0 * (gq - (gq * ref.q).sum(1, keepdim=True) * ref.q)
        out["no_pos_in_dq"] = float(((m0 - pr.dz0).abs() / b0).max())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Dense-match inputs
# ---------------------------------------------------------------------------------------------------------------------
MATCH_CASES = [(3, 49, 49, 8, 8), (3, 49, 49, 72, 16), (2, 64, 65, 136, 8), (1, 196, 196, 64, 8), (5, 7, 2, 40, 8),
               (2, 1, 1, 64, 8), (2, 49, 49, 2048, 512)]
MATCH_FAMILIES = ("relu", "signed")


@functools.lru_cache(maxsize=None)
def match_inputs(family, case, values_dtype=torch.float16):
    """fp16 CPU (x, y, y_values): ReLU'd Gaussians (a trunk's maps are ReLU outputs) or signed Gaussians."""
    b, n, m, c, dv = case
    g = torch.Generator().manual_seed(104729 * b + 1009 * n + 31 * m + c + len(family))
    x, y = torch.randn(b, n, c, generator=g), torch.randn(b, m, c, generator=g)
    if family == "relu":
        x, y = x.relu(), y.relu()
    elif family != "signed":
        raise ValueError(family)
    return x.half(), y.half(), torch.randn(b, m, dv, generator=g).to(values_dtype)


@functools.lru_cache(maxsize=None)
def match_exact_inputs(case):
    """An integer-valued family where every product, sum and score is exact in fp16 / fp32: every key row has exactly
    four entries +-1 (||y|| = 2, 1/||y|| = 0.5), the queries are integers in [-3, 3].  Scores are multiples of 0.5, so
    ties abound; key row 1 is planted again at M - 1 and at M // 2, query row 0 of every image is zero."""
    b, n, m, c, dv = case
    g = torch.Generator().manual_seed(15485863 + 7 * b + n + m + c)
    x = torch.randint(-3, 4, (b, n, c), generator=g).float()
    y = torch.zeros(b, m, c)
    for i in range(b):
        for j in range(m):
            pick = torch.randperm(c, generator=g)[:4]
            y[i, j, pick] = (torch.randint(0, 2, (4,), generator=g) * 2 - 1).float()
    if m > 2:
        y[:, m - 1] = y[:, 1]
        y[:, m // 2] = y[:, 1]
    x[:, 0] = 0.0
    vals = torch.randn(b, m, dv, generator=g)
    return x.half(), y.half(), vals


def match_mutations(x, y):
    """The indices [B, N] two kernel mistakes would return: ties taken from the higher index (shows on the exact
    family); x's norm used for the inverse norm - the scores then rank by the raw dot product (shows where the keys'
    norms differ: the random families)."""
    s = match_scores_f64(x, y)
    m = s.shape[2]
    best = s.max(dim=2, keepdim=True).values
    high = torch.where(s == best, torch.arange(m).expand_as(s), torch.full_like(s, -1, dtype=torch.int64)).max(2).values
    raw = torch.bmm(x.double(), y.double().transpose(1, 2))
    return {"tie_high": high, "x_norm": raw.argmax(2)}
