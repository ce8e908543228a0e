"""oracle.ntxent — NT-Xent restatements (TEST INFRASTRUCTURE ONLY).

lightly.loss.NTXentLoss (call sites HP/src/pretrain_engine.py:93,725) is not
installed; its 4-block formulation is restated from SURVEY.md Appendix A.  The
reference's own in-tree equivalent experiments/DualViewHair/src/losses/ntxent_loss.py
IS importable in the build container and generated tests/golden/ntxent_*.npz
(tests/golden/make_golden.py); tests/test_oracle_ntxent.py pins both restatements to
those vectors.
"""
from __future__ import annotations

import functools
import itertools
from typing import NamedTuple

import torch
import torch.nn.functional as F


def ntxent_lightly(out0: torch.Tensor, out1: torch.Tensor, temperature: float = 0.5) -> torch.Tensor:
    """lightly NTXentLoss.forward, memory_bank_size=0, gather_distributed=False."""
    if abs(temperature) < 1e-8:
        raise ValueError(f"Illegal temperature: abs({temperature}) < 1e-8")
    b = out0.shape[0]
    out0 = F.normalize(out0, dim=1)
    out1 = F.normalize(out1, dim=1)
    l00 = out0 @ out0.t() / temperature
    l01 = out0 @ out1.t() / temperature
    l10 = out1 @ out0.t() / temperature
    l11 = out1 @ out1.t() / temperature
    off = ~torch.eye(b, dtype=torch.bool)
    l00 = l00[off].view(b, -1)
    l11 = l11[off].view(b, -1)
    logits = torch.cat([torch.cat([l01, l00], 1), torch.cat([l10, l11], 1)], 0)
    labels = torch.arange(b).repeat(2)
    return F.cross_entropy(logits, labels)


def ntxent_dualview(z0: torch.Tensor, z1: torch.Tensor, temperature: float) -> torch.Tensor:
    """experiments/DualViewHair/src/losses/ntxent_loss.py:30-57 restated: 2B x 2B matrix,
    diagonal = -inf, positives i <-> i + B, mean cross-entropy."""
    b = z0.shape[0]
    f = torch.cat([F.normalize(z0, dim=-1), F.normalize(z1, dim=-1)], 0)
    sim = f @ f.t() / temperature
    sim = sim.masked_fill(torch.eye(2 * b, dtype=torch.bool), float("-inf"))
    labels = torch.cat([torch.arange(b, 2 * b), torch.arange(0, b)])
    return F.cross_entropy(sim, labels)


class NtRef(NamedTuple):
    """float64 ground truth of one NT-Xent problem (ntxent_f64(..., full=True))."""
    loss: torch.Tensor   # scalar
    lse: torch.Tensor    # [2B] masked row log-sum-exp
    pos: torch.Tensor    # [2B] positive logit of every row
    u: torch.Tensor      # [2B, D] normalised rows
    p: torch.Tensor      # [2B, 2B] softmax of the masked logits (diagonal 0)
    w: torch.Tensor      # [2B, 2B] p + p^T - 2 [j == pos(i)], diagonal 0
    sim: torch.Tensor    # [2B, 2B] logits, diagonal -inf


def positives(b: int) -> torch.Tensor:
    """pos(i) = (i + B) mod 2B."""
    return torch.cat([torch.arange(b, 2 * b), torch.arange(0, b)])


def ntxent_f64(z0, z1, temperature, full: bool = False):
    """float64 value + per-row log-sum-exp (what hcir_ntxent_fwd returns as row_lse).  full=True: an NtRef with the
    per-row positive logit, the normalised rows, the softmax and the backward's W as well."""
    z0 = z0.double()
    z1 = z1.double()
    b = z0.shape[0]
    f = torch.cat([F.normalize(z0, dim=-1), F.normalize(z1, dim=-1)], 0)
    sim = f @ f.t() / temperature
    sim = sim.masked_fill(torch.eye(2 * b, dtype=torch.bool), float("-inf"))
    lse = torch.logsumexp(sim, dim=1)
    pos = sim[torch.arange(2 * b), positives(b)]
    loss = (lse - pos).mean()
    if not full:
        return loss, lse
    p = torch.exp(sim - lse[:, None])
    w = p + p.t()
    w[torch.arange(2 * b), positives(b)] -= 2.0
    w.fill_diagonal_(0.0)
    return NtRef(loss, lse, pos, f, p, w, sim)


def ntxent_grads_f64(z0, z1, temperature, grad_out: float = 1.0):
    """(dL/dz0, dL/dz1) * grad_out by float64 autograd through ntxent_f64."""
    a0 = z0.detach().double().requires_grad_(True)
    a1 = z1.detach().double().requires_grad_(True)
    (ntxent_f64(a0, a1, temperature)[0] * grad_out).backward()
    return a0.grad, a1.grad


# ---------------------------------------------------------------------------------------------------------------
# Per-row / per-element error bounds of hcir_ntxent_fwd / hcir_ntxent_bwd against the float64 reference taken on
# the inputs the kernel reads (already rounded to the tested dtype).
#
#   u_T   unit roundoff of the tested dtype;  u_in = u_T, but 2^-24 on inputs whose normalised rows and cosines are
#         exact in every dtype (family "exact")
#   c     |grad_out| / (|T| 2B),  rn_i = 1 / ||x_i||
#
#   lse   (2 u_in + 2^-20)/|T| + 2^-19 max(1, |ref|)
#           2 u_in/|T| : both operands of a cosine are rows rounded to the compute dtype (u_in each), times 1/T
#           2^-20/|T|  : fp32 normalisation (sum of squares, sqrt, divide) and fp32 MFMA accumulation of the cosine
#           2^-19 max  : fp32 exp2 / log2 / the online merges, relative to the lse (absolute below 1)
#   loss  the lse bound plus the positive logit's own (2 u_in + 2^-20)/|T|; the mean does not add to the worst row
#   grad  dz_i = c rn_i (g_i - (g_i.u_i) u_i), g = W u.  Element error of g:
#           E_ik = (2^-10 + max(u_T, 2^-11)) (|W| |u|)_ik            W rounded to fp16 (2^-11) after an fp32
#                                                                    exp2 pair (2^-11 of slack), u copied to fp16
#                                                                    from the compute dtype
#                + ((4 u_in + 2^-19)/|T|) ((p + p^T, diag 0) |u|)_ik relative error of p_ij: logit and lse errors
#                + 2^-24 sum_j |u_jk|                                fp16 subnormal flush of W (spacing 2^-24)
#         through the projection: E_ik + |u_ik| sum_m E_im |u_im| + 4 u_T |g_i.u_i| |u_ik| (u itself is rounded),
#         times c rn_i, plus the one store in the output dtype (u_T |ref|) and its subnormal spacing q.
# ---------------------------------------------------------------------------------------------------------------
U_ROUND = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def lse_bound(ref_lse, temperature, u_in):
    return (2 * u_in + 2.0 ** -20) / abs(temperature) + 2.0 ** -19 * ref_lse.abs().clamp_min(1.0)


def loss_bound(ref_loss, temperature, u_in):
    return 2 * (2 * u_in + 2.0 ** -20) / abs(temperature) + 2.0 ** -19 * ref_loss.abs().clamp_min(1.0)


def grad_bound(ref: NtRef, x, dz_ref, temperature, grad_out, dtype, u_in):
    """[2B, D] bound on |dz - dz_ref|; x = cat(z0, z1) in float64, dz_ref = cat(dz0, dz1) of ntxent_grads_f64."""
    u_t = U_ROUND[dtype]
    n = x.shape[0]
    au = ref.u.abs()
    e = (2.0 ** -10 + max(u_t, 2.0 ** -11)) * (ref.w.abs() @ au) \
        + ((4 * u_in + 2.0 ** -19) / abs(temperature)) * ((ref.p + ref.p.t()) @ au) \
        + 2.0 ** -24 * au.sum(0, keepdim=True)
    gu = ((ref.w @ ref.u) * ref.u).sum(1, keepdim=True)
    c = abs(grad_out) / (abs(temperature) * n)
    rn = 1.0 / x.norm(dim=1, keepdim=True)
    q = (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -30) * abs(grad_out)
    return u_t * dz_ref.abs() + c * rn * (e + au * (e * au).sum(1, keepdim=True) + 4 * u_t * gu.abs() * au) + q


F16_MAX_ROUND = 65520.0   # |v| >= this rounds to inf in fp16 (65504 + half a spacing of 32)


def err_over_bound(out, ref, bound, dtype=None):
    """max |out - ref| / bound.  fp16 outputs: an infinity of the reference's sign is the correct rounding of any
    value the bound allows at or beyond the fp16 overflow threshold, and counts as no error there; any other
    non-finite output is an infinite error."""
    out = out.double()
    err = (out - ref).abs()
    if dtype == torch.float16:
        ok = torch.isinf(out) & (torch.sign(out) == torch.sign(ref)) & (ref.abs() + bound >= F16_MAX_ROUND)
        err = torch.where(ok, torch.zeros_like(err), err)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------
# Cases (B, D, T) and input families shared by tests/test_ntxent_host.py and tests/test_ntxent_gpu.py
# ---------------------------------------------------------------------------------------------------------------
FWD_CASES = [(1, 8, 0.5), (4, 8, 0.5), (37, 32, 0.5), (64, 64, 0.2), (100, 72, 0.5), (101, 40, 0.1),
             (128, 96, 0.07), (129, 136, 0.5), (132, 8, 0.2), (100, 72, -0.5)]
BWD_CASES = [(4, 8, 0.5), (64, 64, 0.2), (100, 72, 0.5), (128, 96, 0.07), (132, 8, 0.2), (100, 72, -0.5)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MAIN_FAMILIES = ("exact", "norms", "exact_norms")
DEGENERATE_FAMILIES = ("collapsed", "same", "zero_row")   # zero_row: forward only


def case_dtypes(case):
    """Negative temperature: fp32 and fp16 only."""
    return DTYPES[:2] if case[2] < 0 else DTYPES


def u_in_of(family, dtype):
    return 2.0 ** -24 if family in ("exact", "exact_norms") else U_ROUND[dtype]


def _partner_exponents(b, g):
    """Per-row powers of two in 2^-6 .. 2^6 for z0 and z1; a row's and its partner's always differ."""
    e0 = torch.randint(-6, 7, (b,), generator=g)
    e1 = (e0 + 6 + torch.randint(1, 13, (b,), generator=g)) % 13 - 6
    return (2.0 ** e0.double()).float(), (2.0 ** e1.double()).float()


def make_inputs(family: str, b: int, d: int, seed: int = 0):
    """fp32 CPU (z0, z1) of one family; the caller rounds them to the tested dtype.
      exact     : every row four +-0.5 in the first min(D, 16) positions, rows pairwise distinct, z1 = z0: norms are
                  exactly 1 and every cosine a multiple of 0.25, without rounding in fp32, fp16 and bf16
      norms     : z0 randn, z1 = z0 + 0.5 randn, every row times its own power of two in 2^-6 .. 2^6; a row's and its
                  partner's exponents always differ, so their 1/||x|| differ by 1.4x .. 4096x
      exact_norms: 2B pairwise distinct rows of the exact kind (z1 != z0), every row times its own power of two as in
                  "norms": still exact in every dtype (||x|| is a power of two), but u_pos != u_i and rn_pos != rn_i, so
                  the backward's mistakes show against the fp32-level input term even in bf16 at small |T|
      collapsed : one random row repeated 2B times       same : z0 == z1 random
      zero_row  : random rows, one of z0 all zero"""
    g = torch.Generator().manual_seed(1000003 * seed + 1009 * b + d)
    if family in ("exact", "exact_norms"):
        m = min(d, 16)
        combos = list(itertools.combinations(range(m), 4))
        rows = b if family == "exact" else 2 * b
        pick = torch.randperm(len(combos) * 16, generator=g)[:rows].tolist()
        assert len(pick) == rows
        z = torch.zeros(rows, d)
        for r, code in enumerate(pick):
            for bit, k in enumerate(combos[code // 16]):
                z[r, k] = 0.5 if (code >> bit) & 1 else -0.5
        if family == "exact":
            return z, z.clone()
        e0, e1 = _partner_exponents(b, g)
        return z[:b] * e0[:, None], z[b:] * e1[:, None]
    if family == "norms":
        z0 = torch.randn(b, d, generator=g)
        z1 = z0 + 0.5 * torch.randn(b, d, generator=g)
        e0, e1 = _partner_exponents(b, g)
        return z0 * e0[:, None], z1 * e1[:, None]
    if family == "collapsed":
        row = torch.randn(1, d, generator=g)
        return row.repeat(b, 1), row.repeat(b, 1)
    if family == "same":
        z = torch.randn(b, d, generator=g)
        return z, z.clone()
    if family == "zero_row":
        z0, z1 = torch.randn(b, d, generator=g), torch.randn(b, d, generator=g)
        z0[b // 2] = 0.0
        return z0, z1
    raise ValueError(family)


class NtProblem(NamedTuple):
    z0: torch.Tensor      # CPU, tested dtype
    z1: torch.Tensor
    ref: NtRef
    x: torch.Tensor       # [2B, D] float64 of the rounded inputs
    dz: torch.Tensor      # [2B, D] float64 gradients at grad_out = 1 (None for zero_row)
    u_in: float


@functools.lru_cache(maxsize=None)
def problem(family, case, dtype) -> NtProblem:
    """Inputs and float64 reference of one (family, case, dtype), computed once and shared; treat as read-only."""
    b, d, t = case
    z0, z1 = make_inputs(family, b, d)
    z0, z1 = z0.to(dtype), z1.to(dtype)
    ref = ntxent_f64(z0, z1, t, full=True)
    dz = None
    if family != "zero_row":
        dz = torch.cat(ntxent_grads_f64(z0, z1, t), 0)
    return NtProblem(z0, z1, ref, torch.cat([z0, z1], 0).double(), dz, u_in_of(family, dtype))


# ---------------------------------------------------------------------------------------------------------------
# Plain-torch emulation of the kernels' arithmetic (CPU): what the bounds must cover.
# ---------------------------------------------------------------------------------------------------------------
_LOG2E = 1.44269504088896340736
_LN2 = 0.69314718055994530942


def emulate(z0, z1, temperature, grad_out=1.0, backward=True):
    """fp32 normalise -> round to T; fp32 logits; fp32 log2-domain lse; W and u rounded to fp16; fp32 product; fp32
    finish -> round to T.  Returns (loss, lse, dz0, dz1) with dz in the input dtype (None, None without backward)."""
    dtype = z0.dtype
    b = z0.shape[0]
    n = 2 * b
    f32 = torch.float32
    x = torch.cat([z0, z1], 0).float()
    inv = 1.0 / torch.sqrt((x * x).sum(1)).clamp_min(1e-12)
    zn = (x * inv[:, None]).to(dtype).float()
    inv_t = torch.tensor(1.0 / temperature, dtype=f32)
    scale = inv_t * torch.tensor(_LOG2E, dtype=f32)
    raw = (zn @ zn.t()) * scale
    eye = torch.eye(n, dtype=torch.bool)
    x2 = raw.masked_fill(eye, float("-inf"))
    m = x2.max(1).values
    lse2 = m + torch.log2(torch.exp2(x2 - m[:, None]).sum(1))
    ln2 = torch.tensor(_LN2, dtype=f32)
    lse = lse2 * ln2
    pos = positives(b)
    loss = ((lse2 - raw[torch.arange(n), pos]) * ln2).sum() / n
    if not backward:
        return loss, lse, None, None
    l2 = lse * torch.tensor(_LOG2E, dtype=f32)
    w = torch.exp2(raw - l2[:, None]) + torch.exp2(raw - l2[None, :])
    w[torch.arange(n), pos] -= 2.0
    w = w.masked_fill(eye, 0.0).half().float()
    g = w @ zn.half().float()
    gu = (g * zn).sum(1, keepdim=True)
    coef = torch.tensor(grad_out, dtype=f32) * inv_t / torch.tensor(float(n), dtype=f32)
    dz = ((coef * inv)[:, None] * (g - gu * zn)).to(dtype)
    return loss, lse, dz[:b], dz[b:]


# ---------------------------------------------------------------------------------------------------------------
# Mutations of the float64 reference: the factor by which a specific kernel mistake exceeds the bound, taken at the
# row (and column / tile) where it shows LEAST.  inf = the mutation does not exist at this shape or destroys the value.
# ---------------------------------------------------------------------------------------------------------------
def mutation_factors(pr: NtProblem, case, dtype, backward: bool):
    b, d, t = case
    n = 2 * b
    ref = pr.ref
    pos = positives(b)
    idx = torch.arange(n)
    out = {}
    # (a) one row's positive taken from another off-diagonal column: the mean moves by |logit_ij - logit_ipos| / 2B
    other = torch.ones(n, n, dtype=torch.bool)
    other[idx, idx] = False
    other[idx, pos] = False
    shift = (ref.sim - ref.pos[:, None]).abs() / n
    out["a"] = float(shift[other].min() / loss_bound(ref.loss, t, pr.u_in)) if other.any() else float("inf")
    # (b) one row's diagonal left unmasked
    diag = (ref.u * ref.u).sum(1) / t
    out["b"] = float(((torch.logaddexp(ref.lse, diag) - ref.lse).abs() / lse_bound(ref.lse, t, pr.u_in)).min())
    # (c) one 128-wide column tile's partial dropped from one row's lse
    worst = float("inf")
    for c0 in range(0, n, 128):
        keep = torch.ones(n, dtype=torch.bool)
        keep[c0:c0 + 128] = False
        if not keep.any():
            continue
        part = torch.logsumexp(ref.sim[:, keep], dim=1)
        worst = min(worst, float(((part - ref.lse).abs() / lse_bound(ref.lse, t, pr.u_in)).min()))
    out["c"] = worst
    if backward:
        bound = grad_bound(ref, pr.x, pr.dz, t, 1.0, dtype, pr.u_in)
        rn = 1.0 / pr.x.norm(dim=1)
        # (d) rn of row i replaced by its partner's
        out["d"] = float(((pr.dz.abs() * (rn[pos] / rn - 1.0).abs()[:, None]) / bound).max(1).values.min())
        # (e) the -2 missing at W[i][pos(i)]: g_i gains 2 u_pos
        up = ref.u[pos]
        delta = 2.0 * (up - (up * ref.u).sum(1, keepdim=True) * ref.u).abs() * (rn / (abs(t) * n))[:, None]
        out["e"] = float((delta / bound).max(1).values.min())
    return out
