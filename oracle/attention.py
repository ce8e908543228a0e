"""oracle.attention — float64 attention, per-element error bounds and arithmetic emulations (TEST INFRASTRUCTURE ONLY).

Ground truth for hcir_attn_fwd / hcir_attn_fwd_lse / hcir_attn_bwd (csrc/attn.hip, csrc/attn_bwd.hip) and for
hcir_attn_cls_fwd_lse / hcir_attn_cls_bwd (csrc/attn_cls.hip), taken on the fp16 tensors the kernels read:

    s = scale q k^T      p = softmax(s)      o = p v      lse2 = log2 sum_j exp(s_j)          (per batch, head, query)
    D = <dO, o>   dP = dO v^T   dS = p o (dP - D)   dq = scale dS k   dk = scale dS^T q   dv = p^T dO

Every bound below is a sum of named terms, one per rounding point of the kernel source, written as a function of the
float64 intermediates: it tightens by itself when p or v are small.  u = 2^-24 (fp32), h = 2^-11 (fp16), z = 2^-24
(the fp16 subnormal spacing: covers round-to-nearest and truncation below 2^-14).  The fp32 exp2 / log2 terms are the
2^-19 oracle.ntxent already uses for v_exp_f32 / v_log_f32.

Forward, MFMA kernels (attn_fwd_kernel, attn_fwd2_kernel, attn_fwd_generic_kernel — the same arithmetic)
  w_j = exp2(fma(S_j, c, -mxs)) is an UNNORMALISED weight; whatever is common to all keys of a row (the rounding of
  mxs = max * c, the choice of the maximum) cancels in sum_j fp16(w_j) v_j / sum_j w_j.  Relative error of w_j:
    eta_j = |scale| hd u (|q|.|k_j|)     S: hd exact fp16 products accumulated in fp32 by the MFMA   (attn.hip:113)
          + 3 u |s_j - s_max|            c = fp32(scale) * fp32(log2 e) (2u) and the one fma rounding (attn.hip:139,575)
          + 2^-19                        v_exp_f32                                                   (attn.hip:139)
  o_d bound = (1 + 2^-9) [ sum_j p_j |v_jd| (h                   P to fp16 for the PV MFMA           (attn.hip:155)
                                            + eta_j + sum_k p_k eta_k        numerator and denominator
                                            + (n_sum + n_pv + 2) u           fp32 row sum (16 NKT + 1 adds, :141,:182),
                                                                             fp32 PV accumulation (32 NKT terms, :179),
                                                                             the product with 1 / sum (:198)
                                            + 3 * 2^-23)                     1.0f / sum                   (attn.hip:183)
                             + z p_max sum_{j: p_j < 2^-13 p_max} |v_jd|     fp16 subnormal spacing of tiny P
                             + h |o_d| + z ]                                 the fp16 store               (attn.hip:198)
  (1 + 2^-9): the terms are first order; products of two of them (at most 2^-10 relative) go here.
  lse bound = (1 + 2^-9) [ sum_j p_j (|scale| hd u |q|.|k_j| + 2 u |s_j| + u |s_j - s_max| + 2^-19 + n_sum u) / ln 2
                           + 2^-19 max(1, log2 of the row sum)               v_log_f32                    (attn.hip:185)
                           + 2 u (|lse2| + 1) ]                              mxs + log2(sum) in fp32
  (in the lse mxs does not cancel as a value but as an exact fma operand: only c's own error stays, on the full s_j).

Forward, class-token kernel (attn_cls_fwd_kernel): scores by v_dot2_f32_f16 chains (hd / 2 steps, at most two
  roundings each: the same hd u |q|.|k_j|), s = dot * c rounded (u |s_j|, not common to the row, attn_cls.hip:57),
  s - mx rounded (:64), per-lane sums of 4 and a 6-step butterfly (n_sum = 10), p = w * inv in fp32 (no fp16 P:
  no h and no z term), o = T sequential fp32 fmas (n_pv = T, :76), one fp16 store (:77).

Backward, MFMA kernels (attn_bwd2_kernel T <= 224, attn_bwd_kernel T <= 256).  Given o_err >= |O_given - o| and
  lse_err >= |lse_given - lse2| (the forward bounds when O and lse come from hcir_attn_fwd_lse, as in use):
    E_D   = sum_d |dO_d| o_err_d + (hd + 1) u sum_d |dO_d o_d|       D from the fp16 O it is given (attn_bwd.hip:105,:466)
    eta_ij = ln 2 lse_err_i                                          P recomputed from the given lse  (:168,:553,:656)
           + |scale| hd u |q_i|.|k_j| + (hd + 4) u |lse_i|           fp32 MFMA sums that START at -lse / c (:472,:519)
           + 2 u |s_ij| + u |s_ij - lse_i| + 2^-19                   c, the product / fma rounding, v_exp_f32
    E_G   = E_D + hd u (|dO_i|.|v_j| + |D_i|) + u |dP - D|           dP - D: MFMA started at -D          (:520,:658)
    E_dS  = |dS| (eta + u + h) + p E_G + z [|dS| < 2^-13]            dS to fp16                          (:555,:658,:172)
    E_P   = p (eta + h) + z [p < 2^-13]                              P to fp16                           (:554,:171)
    dv bound = (1 + 2^-9) [ E_P^T |dO| + n u p^T |dO| + h |dv| + z ]                  n = 32 NKT + 8: fp32 MFMA /
    dk bound = (1 + 2^-9) [ |scale| (E_dS^T |q| + n u |dS|^T |q|) + (2 u + h) |dk| + z ]   slab sums (:263), then
    dq bound = (1 + 2^-9) [ |scale| (E_dS |k| + n u |dS| |k|) + (2 u + h) |dq| + z ]       * scale and the store
Backward, class-token kernel: dS and P stay fp32 (no h, no z inside the sums); dk_j = fp16(scale dS_j q_d) and
  dv_j = fp16(p_j dO_d) are single products (:125,:126); D is a product and a 6-step butterfly (8 u, :99).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

U32 = 2.0 ** -24
H16 = 2.0 ** -11
Z16 = 2.0 ** -24
E_EXP2 = 2.0 ** -19      # oracle.ntxent: fp32 exp2 / log2
E_LOG2 = 2.0 ** -19
E_DIV = 3 * 2.0 ** -23
SECOND = 1.0 + 2.0 ** -9
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2


def f32(x: float) -> float:
    """The value a C float argument takes."""
    return float(torch.tensor(x, dtype=torch.float32))


class AttnRef(NamedTuple):
    """float64, [b, h, rows, ...] layout; q has nq rows, k and v have t."""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    scale: float
    s: torch.Tensor        # [b, h, nq, t]
    p: torch.Tensor
    o: torch.Tensor        # [b, h, nq, hd]
    lse2: torch.Tensor     # [b, h, nq]
    do: Optional[torch.Tensor] = None
    d: Optional[torch.Tensor] = None       # [b, h, nq]
    dp: Optional[torch.Tensor] = None
    ds: Optional[torch.Tensor] = None
    dq: Optional[torch.Tensor] = None      # [b, h, nq, hd]
    dk: Optional[torch.Tensor] = None      # [b, h, t, hd]
    dv: Optional[torch.Tensor] = None


def core_f64(q, k, v, scale, do=None) -> AttnRef:
    """Attention of q [b, h, nq, hd] over k, v [b, h, tk, hd], every intermediate from its definition."""
    s = scale * (q @ k.transpose(-1, -2))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / den
    o = p @ v
    lse2 = (m.squeeze(-1) + torch.log(den.squeeze(-1))) * LOG2E
    if do is None:
        return AttnRef(q, k, v, scale, s, p, o, lse2)
    d = (do * o).sum(-1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - d[..., None])
    return AttnRef(q, k, v, scale, s, p, o, lse2, do, d, dp, ds,
                   scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ do)


def split_qkv(qkv, b, t, h, hd):
    """fp16 [b, t, 3, h, hd] (any shape with that many elements) -> float64 q, k, v [b, h, t, hd]."""
    x = qkv.reshape(b, t, 3, h, hd).double().permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads_of(x, b, n, h, hd):
    """[b, n, h * hd] -> float64 [b, h, n, hd]."""
    return x.reshape(b, n, h, hd).double().permute(0, 2, 1, 3)


def rows_of(x):
    """[b, h, n, hd] -> [b, n, h * hd] (the kernels' output layout)."""
    b, h, n, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * hd)


def pack_dqkv(dq, dk, dv):
    """three [b, h, t, hd] -> [b, t, 3, h, hd]; dq with fewer rows than t is padded with zero rows."""
    t = dk.shape[2]
    if dq.shape[2] < t:
        dq = torch.cat([dq, dq.new_zeros(dq.shape[0], dq.shape[1], t - dq.shape[2], dq.shape[3])], 2)
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).contiguous()


def attention_f64(qkv, b, t, h, hd, scale, dout=None, nq=None) -> AttnRef:
    """qkv fp16 [b, t, 3, h, hd]; dout [b, nq, h * hd] (or [b, h * hd] with nq = 1); the first nq query rows."""
    nq = t if nq is None else nq
    q, k, v = split_qkv(qkv, b, t, h, hd)
    do = None if dout is None else heads_of(dout, b, nq, h, hd)
    return core_f64(q[:, :, :nq], k, v, float(scale), do)


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def fwd_bounds(r: AttnRef, kind: str = "mfma"):
    """(bound on o [b, h, nq, hd], bound on lse2 [b, h, nq]); kind "mfma" or "cls"."""
    hd, t = r.q.shape[-1], r.k.shape[-2]
    asc = abs(r.scale)
    av = r.v.abs()
    dot = r.q.abs() @ r.k.abs().transpose(-1, -2)
    smax = r.s.max(-1, keepdim=True).values
    pmax = r.p.max(-1, keepdim=True).values
    nkt = (t + 31) // 32
    if kind == "mfma":
        n_sum, n_pv = 16 * nkt + 1, 32 * nkt
        eta = asc * hd * U32 * dot + 3 * U32 * (r.s - smax).abs() + E_EXP2
        p_round = H16
    else:
        n_sum, n_pv = 10, t
        eta = asc * hd * U32 * dot + 2 * U32 * r.s.abs() + 3 * U32 * (r.s - smax).abs() + E_EXP2
        p_round = U32
    etabar = (r.p * eta).sum(-1, keepdim=True)
    rel = p_round + eta + etabar + (n_sum + n_pv + 2) * U32 + E_DIV
    bo = (r.p * rel) @ av + H16 * r.o.abs() + Z16
    if kind == "mfma":
        tiny = (r.p < 2.0 ** -13 * pmax).double()
        bo = bo + Z16 * pmax * (tiny @ av)
    eta_l = asc * hd * U32 * dot + 2 * U32 * r.s.abs() + U32 * (r.s - smax).abs() + E_EXP2 + n_sum * U32
    logsum = r.lse2 - smax.squeeze(-1) * LOG2E
    bl = (r.p * eta_l).sum(-1) * LOG2E + E_LOG2 * logsum.clamp_min(1.0) + 2 * U32 * (r.lse2.abs() + 1.0)
    return SECOND * bo, SECOND * bl


def bwd_bounds(r: AttnRef, o_err, lse_err, kind: str = "mfma"):
    """(bounds on dq [b, h, nq, hd], dk, dv [b, h, t, hd]) given o_err [b, h, nq, hd] and lse_err [b, h, nq]."""
    hd, t = r.q.shape[-1], r.k.shape[-2]
    asc = abs(r.scale)
    aq, ak, av, ado = r.q.abs(), r.k.abs(), r.v.abs(), r.do.abs()
    tr = lambda x: x.transpose(-1, -2)
    lse = (r.lse2 * LN2)[..., None]
    n_d = hd + 1 if kind == "mfma" else 8
    e_d = (ado * o_err).sum(-1) + n_d * U32 * (ado * r.o.abs()).sum(-1)
    eta = LN2 * lse_err[..., None] + asc * hd * U32 * (aq @ tr(ak)) + (hd + 4) * U32 * lse.abs() \
        + 2 * U32 * r.s.abs() + U32 * (r.s - lse).abs() + E_EXP2
    e_g = e_d[..., None] + hd * U32 * (ado @ tr(av) + r.d.abs()[..., None]) + U32 * (r.dp - r.d[..., None]).abs()
    ads = r.ds.abs()
    if kind == "mfma":
        n = 32 * ((t + 31) // 32) + 8
        e_ds = ads * (eta + U32 + H16) + r.p * e_g + Z16 * (ads < 2.0 ** -13).double()
        e_p = r.p * (eta + H16) + Z16 * (r.p < 2.0 ** -13).double()
        bdv = tr(e_p) @ ado + n * U32 * (tr(r.p) @ ado) + H16 * r.dv.abs() + Z16
        bdk = asc * (tr(e_ds) @ aq + n * U32 * (tr(ads) @ aq)) + (2 * U32 + H16) * r.dk.abs() + Z16
        bdq = asc * (e_ds @ ak + n * U32 * (ads @ ak)) + (2 * U32 + H16) * r.dq.abs() + Z16
    else:
        e_ds = ads * (eta + 2 * U32) + r.p * e_g
        bdv = tr(r.p * (eta + U32)) @ ado + H16 * r.dv.abs() + Z16
        bdk = asc * (tr(e_ds) @ aq) + (3 * U32 + H16) * r.dk.abs() + Z16
        bdq = asc * (e_ds @ ak + t * U32 * (ads @ ak)) + (2 * U32 + H16) * r.dq.abs() + Z16
    return SECOND * bdq, SECOND * bdk, SECOND * bdv


def ratio(out, ref, bound) -> float:
    """max |out - ref| / bound; a non-finite output is an infinite error."""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err / bound).max()) if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# input families: fp16 CPU qkv [b, t, 3, h, hd]
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("sharp", "flat", "uniform", "marker_last", "marker_first", "negdom")
NEG_LEVELS = (9.0, 10.5, 12.0, 14.0, 16.0, 18.0, 30.0)   # -score (natural units) of the non-dominant keys


def uniform_v(t, hd):
    """Small integers that depend asymmetrically on (key, dim): no permutation of keys or dims leaves them alone."""
    j = torch.arange(t)[:, None]
    d = torch.arange(hd)[None, :]
    return ((j * 7 + d * 3 + (j * d) % 5 + (j // 3) * (d % 2)) % 17 - 8).float()


def make_qkv(family: str, b: int, t: int, h: int, hd: int, seed: int = 0) -> torch.Tensor:
    """sharp        randn * 1.5, query 5 % t of every head aligned with key 150 % t (score ~ 2 |k|^2 scale)
    flat         randn * 0.4
    uniform      K = 0: P = 1 / t exactly, O = mean of V; V = uniform_v (dims 0..3 constant along the keys: a dout
                 that lives in those dims alone gives dS = 0 exactly)
    marker_last  flat, but dim 0 of every q is 1 and the LAST key has k[0] = 16 hd^0.5 / 8 (score ~ +2 with every
                 query) and a V row 16 x larger than the rest;  marker_first: the same on key 0
    negdom       dims 0 / 1 of q are 8 hd^0.5 / 8 on even / odd queries; every key's dims 0 and 1 are -level_j with
                 level_j cycling through NEG_LEVELS (scores -9 .. -30), except key t // 3 (dim 0 = 0: dominant for
                 even queries) and key t - 1 (dim 1 = 0: dominant for odd queries): P runs through the fp16
                 subnormals down to 0."""
    g = torch.Generator().manual_seed(7919 * seed + 104729 * t + 31 * b + 7 * h + hd + 1000003 * FAMILIES.index(family))
    amp = {"sharp": 1.5}.get(family, 0.4)
    x = torch.randn(b, t, 3, h, hd, generator=g) * amp
    root = hd ** 0.5 / 8.0
    if family == "sharp":
        x[:, 5 % t, 0] = x[:, 150 % t, 1] * 2.0
    elif family == "uniform":
        x[:, :, 1] = 0.0
        v = uniform_v(t, hd)
        v[:, :4] = torch.arange(1, 5).float()
        x[:, :, 2] = v[None, :, None, :]
    elif family in ("marker_last", "marker_first"):
        j = t - 1 if family == "marker_last" else 0
        x[:, :, 0, :, 0] = 1.0
        x[:, j, 1, :, 0] = 16.0 * root
        x[:, j, 2] *= 16.0
    elif family == "negdom":
        lv = torch.tensor([NEG_LEVELS[j % len(NEG_LEVELS)] for j in range(t)])
        x[:, :, 0, :, :2] = 0.0
        x[:, 0::2, 0, :, 0] = 8.0 * root
        x[:, 1::2, 0, :, 1] = 8.0 * root
        x[:, :, 1, :, 0] = -lv[None, :, None]
        x[:, :, 1, :, 1] = -lv[None, :, None]
        x[:, t // 3, 1, :, 0] = 0.0
        x[:, t - 1, 1, :, 1] = 0.0
    elif family != "flat":
        raise ValueError(family)
    return x.half()


def make_dout(b, n, h, hd, seed=0, amp=0.1):
    g = torch.Generator().manual_seed(15485863 * seed + 97 * n + b + h)
    return (torch.randn(b, n, h * hd, generator=g) * amp).half()


# ---------------------------------------------------------------------------------------------------------------
# emulations of the kernels' arithmetic (CPU, for tests/test_attention_host.py): fp32 torch ops at the kernels'
# rounding points.  The order of the fp32 sums differs from the hardware's; the bounds do not depend on it.
# ---------------------------------------------------------------------------------------------------------------
def _c32(scale):
    return torch.tensor(f32(scale), dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate_fwd(qkv, b, t, h, hd, scale, nq=None):
    """MFMA forward family -> (out fp16 [b, nq, h * hd], lse fp32 [b, h, nq])."""
    nq = t if nq is None else nq
    q, k, v = [x.float() for x in split_qkv(qkv, b, t, h, hd)]
    c = _c32(scale)
    s = q[:, :, :nq] @ k.transpose(-1, -2)
    mxs = s.max(-1, keepdim=True).values * c
    w = torch.exp2(_fma(s, c, -mxs))
    tot = w.sum(-1, keepdim=True)
    o = ((w.half().float() @ v) * (1.0 / tot)).half()
    return rows_of(o), (mxs + torch.log2(tot)).squeeze(-1)


def emulate_bwd(qkv, out, dout, lse, b, t, h, hd, scale):
    """MFMA backward family (the arithmetic of attn_bwd2_kernel) -> dqkv fp16 [b, t, 3, h, hd]."""
    q, k, v = [x.float() for x in split_qkv(qkv, b, t, h, hd)]
    o, do = heads_of(out, b, t, h, hd).float(), heads_of(dout, b, t, h, hd).float()
    c, sc = _c32(scale), torch.tensor(f32(scale), dtype=torch.float32)
    d = (o * do).sum(-1, keepdim=True)
    start = -lse.float()[..., None] * (1.0 / c)
    p = torch.exp2((start + q @ k.transpose(-1, -2)) * c)
    g = (-d) + do @ v.transpose(-1, -2)
    p16, ds16 = p.half().float(), (p * g).half().float()
    dv = (p16.transpose(-1, -2) @ do).half()
    dk = ((ds16.transpose(-1, -2) @ q) * sc).half()
    dq = ((ds16 @ k) * sc).half()
    return pack_dqkv(dq, dk, dv)


def emulate_cls_fwd(qkv, b, t, h, hd, scale):
    """attn_cls_fwd_kernel -> (out fp16 [b, h * hd], lse fp32 [b, h])."""
    q, k, v = [x.float() for x in split_qkv(qkv, b, t, h, hd)]
    c = _c32(scale)
    s = (q[:, :, :1] @ k.transpose(-1, -2)) * c
    mx = s.max(-1, keepdim=True).values
    w = torch.exp2(s - mx)
    tot = w.sum(-1, keepdim=True)
    o = ((w * (1.0 / tot)) @ v).half()
    return rows_of(o)[:, 0], (torch.log2(tot) + mx)[:, :, 0, 0]


def emulate_cls_bwd(qkv, out, dout, lse, b, t, h, hd, scale):
    """attn_cls_bwd_kernel -> dqkv fp16 [b, t, 3, h, hd] (dq rows 1 .. t-1 zero)."""
    q, k, v = [x.float() for x in split_qkv(qkv, b, t, h, hd)]
    o, do = heads_of(out, b, 1, h, hd).float(), heads_of(dout, b, 1, h, hd).float()
    c, sc = _c32(scale), torch.tensor(f32(scale), dtype=torch.float32)
    dd = (o * do).sum(-1, keepdim=True)
    p = torch.exp2((q[:, :, :1] @ k.transpose(-1, -2)) * c - lse.float()[..., None, None])
    ds = p * (do @ v.transpose(-1, -2) - dd)
    dq = (sc * (ds @ k)).half()
    dk = ((sc * ds).transpose(-1, -2) * q[:, :, :1]).half()
    dv = (p.transpose(-1, -2) * do).half()
    return pack_dqkv(dq, dk, dv)
