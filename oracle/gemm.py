"""oracle.gemm — float64 GEMM epilogues, per-element error bounds and arithmetic emulations (TEST INFRASTRUCTURE ONLY).

Ground truth for hcir_gemm_f16 / hcir_gemm_f16_resid / hcir_gemm_f16_gelu_dual / hcir_gemm_f16_fused /
hcir_ln_stats_finalize (csrc/gemm.hip) and hcir_gemm_f16_tn (csrc/gemm_tn.hip), taken on the tensors the kernels read:
fp16 A [m, k] and W [n, k], fp32 bias, scale, (mean, rstd) and c1.  Every function works on the device of its inputs.

Notation   S = sum_k a w,   A = sum_k |a w|,   x = S + bias,   u = 2^-24 (fp32), h = 2^-11 (fp16), z = 2^-24 (the fp16
subnormal spacing), K = k.  The fp16 products are exact in fp32; the MFMA accumulation counts as K u A (the convention
of oracle.attention); every bound is multiplied by (1 + 2^-9) for products of two first-order terms.

  e_acc = K u A                                                                  (gemm.hip:497 / :721 / :815, MFMA sums)
  BIAS_F32          e_acc + u|x|                     the bias add                                     (gemm.hip:90, :424)
  BIAS_F16          ... + h|x| + z                   the fp16 store                                   (gemm.hip:100, :316)
  BIAS_GELU_F16     1.13 (e_acc + u|x|) + e_gelu(x) + h|g| + z        sup|gelu'| = 1.1290 at x = sqrt 2; g = gelu(x)
    e_gelu(x) = |x| (0.75e-7                         Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7, q = erfc / 2 (act.h:6)
                     + e E_PT                        e = exp(-x^2/2); P(t) t: den (fma, u) and p/sqrt2 as a float (u),
                                                     v_rcp_f32 (1 ulp = 2u): t to 4u, |d(P t)/dt| t <= 1.72 -> 7u; four
                                                     Horner fmas on values <= 0.75 (3u); p * t (0.5u): E_PT = 16u (act.h:17-25)
                     + q (2^-19 + 1.5 u x^2 + u)     v_exp_f32; its argument (x x) kNW2 carries 2 roundings and the
                                                     constant's own (1.5 u x^2 relative on e); pt * e      (act.h:23-26)
                     + 0.5 u)                        0.5 - pt e                                           (act.h:26)
                + u|g|                               the last fma                                         (act.h:27)
  dual              out_pre as BIAS_F16, out_act as BIAS_GELU_F16 (GELU of the fp32 x, not of the rounded one)  (:307)
  AFFINE_F32        |s| e_acc + u|x|,  x = s S + bias: one fma                                        (gemm.hip:87, :418)
  AFFINE_RELU_F16   the same (ReLU is 1-Lipschitz) + h|relu x| + z                                    (gemm.hip:99, :299)
  BIAS_RESID_F32    |s| (e_acc + u|x|) + u|y|,  y = r + s x: the bias add, then one fma               (gemm.hip:119, :421)
  BIAS_RESID_F16    |s| (e_acc + u|x|) + u|s x| + h|s x| + z + h|y| + z     the contract of include/hcir.h
                    (HCIR_EPI_BIAS_RESID_F16): fp16(s (acc + bias)), then the fp16 sum rounded once - what the
                    persistent epilogue does (gemm.hip:301, :359).  The 128 x 128 kernel's single fma and ONE rounding
                    (gemm.hip:110) has the terms |s| (e_acc + u|x|) + u|y| + h|y| + z only: inside the same bound.  Both
                    are right; neither is to be "fixed".
  LayerNorm fold    e_x = rstd (e_acc + u|mean c1| + u|S - mean c1|) + u|x|,  x = rstd (S - mean c1) + bias on the GIVEN
                    fp32 (mean, rstd) and c1 (two fmas, gemm.hip:297); then the fp16 store, or the GELU terms on e_x.
                    Whether the fold IS a LayerNorm is test_gemm_fused_layernorm's question, not this module's.
  statistics        per 64-feature slice of the STORED fp16 row (gemm.hip:373-386): mean_s by an 8-add chain and a DPP
                    sum of 8 (11 adds): d_mean_s = 11 u mean|x|;  M2_s about the computed mean_s (xv - mean_s rounded,
                    squared and summed by 8 fmas and the DPP sum): d_M2_s = 13 u M2' + 64 d_mean_s^2, M2' = M2 + 64 d_mean_s^2.
  finalize          (ln_stats_finalize_kernel, gemm.hip "Chan") P slices in index order:
                    d_mean = mean_p(d_mean_s) + u sum_p|mean_p| + 2u|mean|                  P adds, one division
                    d_dm_p = d_mean + d_mean_p + u|dm_p|                                    dm = mean_p - mean
                    d_var  = [ sum_p (d_M2_p + 64 (2|dm_p| d_dm_p + d_dm_p^2) + 3u (M2_p + 64 dm_p^2)) + P u m2 ] / (64 P)
                             + 3u var                                                       64 dm dm, the add, P adds, /
                    d_rstd = rstd (d_var / (2 (var + eps)) + 6u)                            var + eps, sqrtf, 1 / x
  gemm_tn           dW = sum_s P_s,  P_s the partial of split s over its `steps_s` 64-row steps (gemm_tn.hip:116):
                    sum_s steps_s 64 u A_s  +  (splits - 1) u sum_s |P_s| (split_sum.h:20)  +  u|old + dW| with
                    accumulate (split_sum.h:26).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from oracle.attention import E_EXP2, H16, SECOND, U32, Z16, ratio  # noqa: F401  (ratio is re-exported)

GELU_LIP = 1.13
E_AS = 0.75e-7
E_PT = 16 * U32
SQRT1_2 = math.sqrt(0.5)
LN_EPS = 1e-6

# hcir_epilogue values, by name
EPI = {"bias_f16": 0, "gelu_f16": 1, "resid_f32": 2, "bias_f32": 3, "affine_relu_f16": 4, "affine_f32": 5, "resid_f16": 6}
F32_KINDS = ("resid_f32", "bias_f32", "affine_f32")
ROUTE_SMALL, ROUTE_MID, ROUTE_BIG, ROUTE_SPLIT = range(4)
ROUTE_EPI_DUAL = 10


class Acc(NamedTuple):
    s: torch.Tensor     # [m, n] float64
    a: torch.Tensor     # [m, n] float64, sum_k |a w|
    k: int


def acc_f64(a, w, rows=8192) -> Acc:
    """S and A of fp16 a [m, k], w [n, k], in row blocks (memory)."""
    w64 = w.double().t().contiguous()
    wa = w64.abs()
    s = torch.empty((a.shape[0], w.shape[0]), dtype=torch.float64, device=a.device)
    ab = torch.empty_like(s)
    for r0 in range(0, a.shape[0], rows):
        x = a[r0:r0 + rows].double()
        s[r0:r0 + rows] = x @ w64
        ab[r0:r0 + rows] = x.abs() @ wa
    return Acc(s, ab, a.shape[1])


def gelu_f64(x):
    return 0.5 * x * torch.special.erfc(-x * SQRT1_2)


def gelu_tanh_f64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_err(x):
    """e_gelu(x): the error of act.h's gelu_erf2 on an exact fp32 x."""
    ax = x.abs()
    e = torch.exp(-0.5 * x * x)
    q = 0.5 * torch.special.erfc(ax * SQRT1_2)
    return ax * (E_AS + e * E_PT + q * (E_EXP2 + 1.5 * U32 * x * x + U32) + 0.5 * U32) + U32 * gelu_f64(x).abs()


def epilogue_f64(kind, acc: Acc, bias=None, scale=None, resid=None, stats=None, c1=None):
    """kind: a key of EPI, "ln_bias_f16", "ln_gelu_f16" or "dual" -> [(reference, bound), ...], one per output.
    stats [m, 2] fp32 (mean, rstd) and c1 [n] fp32 for the fold; resid [m, n] of the output's type."""
    s, e_acc = acc.s, acc.k * U32 * acc.a
    b = torch.zeros(s.shape[1], dtype=torch.float64, device=s.device) if bias is None else bias.double()
    sc = None if scale is None else scale.double()
    f16 = lambda v: H16 * v.abs() + Z16
    if kind in ("ln_bias_f16", "ln_gelu_f16"):
        mean, rstd, c = stats[:, :1].double(), stats[:, 1:].double(), c1.double()[None, :]
        inner = s - mean * c
        x = rstd * inner + b
        e_x = rstd.abs() * (e_acc + U32 * (mean * c).abs() + U32 * inner.abs()) + U32 * x.abs()
        if kind == "ln_bias_f16":
            return [(x, SECOND * (e_x + f16(x)))]
        g = gelu_f64(x)
        return [(g, SECOND * (GELU_LIP * e_x + gelu_err(x) + f16(g)))]
    if kind in ("affine_relu_f16", "affine_f32"):
        x = s * sc + b
        e_x = sc.abs() * e_acc + U32 * x.abs()
        if kind == "affine_f32":
            return [(x, SECOND * e_x)]
        r = x.clamp_min(0.0)
        return [(r, SECOND * (e_x + f16(r)))]
    x = s + b
    e_x = e_acc + U32 * x.abs()
    if kind == "bias_f32":
        return [(x, SECOND * e_x)]
    if kind == "bias_f16":
        return [(x, SECOND * (e_x + f16(x)))]
    if kind in ("gelu_f16", "dual"):
        g = gelu_f64(x)
        act = (g, SECOND * (GELU_LIP * e_x + gelu_err(x) + f16(g)))
        return [act] if kind == "gelu_f16" else [(x, SECOND * (e_x + f16(x))), act]
    sx = x if sc is None else sc * x
    e_sx = e_x if sc is None else sc.abs() * e_x
    y = resid.double() + sx
    if kind == "resid_f32":
        return [(y, SECOND * (e_sx + U32 * y.abs()))]
    if kind == "resid_f16":
        return [(y, SECOND * (e_sx + U32 * sx.abs() + f16(sx) + f16(y)))]
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------
# per-row statistics: slices [P, m] of 64 features, and their combination
# ---------------------------------------------------------------------------------------------------------------
def slice_stats_f64(rows):
    """Stored fp16 rows [m, n] -> (mean_p, M2_p, d_mean_p, d_M2_p), each [n / 64, m] float64."""
    x = rows.double().reshape(rows.shape[0], -1, 64)
    mean = x.mean(-1)
    m2 = ((x - mean[..., None]) ** 2).sum(-1)
    d_mean = 11 * U32 * x.abs().mean(-1)
    d_m2 = 13 * U32 * (m2 + 64 * d_mean ** 2) + 64 * d_mean ** 2
    return tuple(SECOND ** i * t.t().contiguous() for t, i in ((mean, 0), (m2, 0), (d_mean, 1), (d_m2, 1)))


def finalize_f64(mean_p, m2_p, eps, d_mean_p=0.0, d_m2_p=0.0):
    """Slices [P, m] (the values the kernel is given, or float64 truths with their errors d_*) ->
    (mean, rstd, bound on mean, bound on rstd), each [m] float64."""
    mean_p, m2_p = mean_p.double(), m2_p.double()
    p = mean_p.shape[0]
    zero = torch.zeros_like(mean_p)
    d_mean_p, d_m2_p = zero + d_mean_p, zero + d_m2_p
    mean = mean_p.mean(0)
    dm = mean_p - mean
    tot = (m2_p + 64 * dm * dm).sum(0)
    var = tot / (64 * p)
    rstd = (var + eps).rsqrt()
    d_mean = d_mean_p.mean(0) + U32 * mean_p.abs().sum(0) + 2 * U32 * mean.abs()
    d_dm = d_mean + d_mean_p + U32 * dm.abs()
    d_tot = (d_m2_p + 64 * (2 * dm.abs() * d_dm + d_dm ** 2) + 3 * U32 * (m2_p + 64 * dm * dm)).sum(0) + p * U32 * tot
    d_var = d_tot / (64 * p) + 3 * U32 * var
    d_rstd = rstd * (d_var / (2 * (var + eps)) + 6 * U32)
    return mean, rstd, SECOND * d_mean, SECOND * d_rstd


# ---------------------------------------------------------------------------------------------------------------
# hcir_gemm_f16_tn
# ---------------------------------------------------------------------------------------------------------------
def tn_plan(m, n, k):
    """(splits, rows_per_split) of gemm_tn.hip's tn_plan; tests check `splits` against the workspace size the library
    reports, so that a changed plan fails loudly."""
    tiles = (n // 256) * (k // 256)
    steps = m // 64
    splits = max(1, min(256 // tiles, steps))
    rows = -(-steps // splits) * 64
    return -(-m // rows), rows


# (m, n, k) of the weight-gradient tests, n = k = 256 (one tile) and 512 (four): one step; every split one step;
# a shorter last split; tiles * splits = 256 (with one and with two steps per split)
TN_SHAPES = [(64, 256, 256), (100 * 64, 256, 256), (301 * 64, 256, 256), (256 * 64, 256, 256),
             (64, 512, 512), (64 * 64, 512, 512), (130 * 64, 512, 512), (128 * 64, 512, 512)]


def tn_f64(a, b, old=None, accumulate=0):
    """a [m, n], b [m, k] fp16 -> (dW [n, k] float64, bound, partials [splits, n, k] float64)."""
    m, n, k = a.shape[0], a.shape[1], b.shape[1]
    splits, rows = tn_plan(m, n, k)
    parts, bound = [], 0.0
    for s in range(splits):
        xa, xb = a[s * rows:(s + 1) * rows].double(), b[s * rows:(s + 1) * rows].double()
        parts.append(xa.t() @ xb)
        bound = bound + (xa.shape[0] // 64) * 64 * U32 * (xa.abs().t() @ xb.abs())
    parts = torch.stack(parts)
    dw = parts.sum(0)
    bound = bound + (splits - 1) * U32 * parts.abs().sum(0)
    if accumulate:
        dw = dw + old.double()
        bound = bound + U32 * dw.abs()
    return dw, SECOND * bound, parts


# ---------------------------------------------------------------------------------------------------------------
# input families: fp16 / fp32 CPU tensors
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "tail", "cancel", "offset", "marker")


def marker_pos(m, k):
    """The one-hot column of marker row i: every k consecutive rows use every column once, in an order that changes
    from one run of k rows to the next."""
    i = torch.arange(m)
    return (i * 5 + (i // k) * 3 + 1) % k if k % 5 else (i + (i // k) * 3 + 1) % k


def make_problem(family, m, n, k, seed=0):
    """dict(a [m, k] fp16, w [n, k] fp16, bias [n], scale [n] fp32 (both signs), resid [m, n] fp32 (tests round it to
    fp16 for fp16 outputs), stats [m, 2] fp32 = (mean, rstd) of the rows of a, c1 [n] fp32 = sum_k w).
    plain    randn / 2 with per-row offsets; W rows and columns scaled unevenly
    tail     small A, bias in [-4, -1.5]: the negative GELU tail, |gelu(x)| << |x|
    cancel   a common component 1 in A and 1/4 in W (|S| ~ k / 4), bias = -(column mean of S): |x| << |acc|
    offset   the first quarter of the rows of a and resid carry +60 (|mean| / std ~ 50), channel 5 of the others is
             scaled by 20 (on the offset rows it would drown the offset: |mean| / std < 1)
             and W has a common component of one standard deviation, so that |c1| ~ sum_k |w| and the accumulator of an
             offset row is nearly all mean * c1 (|S| ~ A)
    marker   one-hot a rows, marker_pos: every output is one W element."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * m + 104729 * n + 31 * k + 15485863 * FAMILIES.index(family))
    rnd = lambda *s: torch.randn(*s, generator=g)
    a = rnd(m, k) * 0.5 + rnd(m, 1) * 0.25
    w = rnd(n, k) * k ** -0.5 * (1.0 + 0.5 * torch.rand(n, 1, generator=g)) * (1.0 + 0.25 * torch.rand(1, k, generator=g))
    bias = rnd(n)
    scale = (torch.rand(n, generator=g) + 0.5) * torch.where(torch.arange(n) % 7 == 3, -1.0, 1.0)
    resid = rnd(m, n) + rnd(m, 1)
    if family == "tail":
        a = a * 0.1
        bias = -1.5 - 2.5 * torch.rand(n, generator=g)
    elif family == "cancel":
        a = a * 0.5 + 1.0
        w = w + 0.25
    elif family == "offset":
        q = max(1, m // 4)
        a = rnd(m, k) + rnd(m, 1) * 2.0
        a[:q] += 60.0
        a[q:, 5 % k] *= 20.0
        w = w + k ** -0.5
        resid = rnd(m, n) + rnd(m, 1) * 2.0
        resid[:q] += 60.0
        resid[q:, 5 % n] *= 20.0
    elif family == "marker":
        a = torch.zeros(m, k)
        a[torch.arange(m), marker_pos(m, k)] = 1.0
    elif family != "plain":
        raise ValueError(family)
    a, w = a.half(), w.half()
    if family == "cancel":
        bias = -(a.double() @ w.double().t()).mean(0).float()
    x = a.double()
    stats = torch.stack([x.mean(1), (x.var(1, unbiased=False) + LN_EPS).rsqrt()], 1).float()
    return dict(a=a, w=w, bias=bias.float(), scale=scale.float(), resid=resid.float(), stats=stats,
                c1=w.double().sum(1).float())


def make_tn(m, n, k, seed=0):
    """a [m, n], b [m, k] fp16 with uneven rows and columns, old [n, k] fp32."""
    g = torch.Generator().manual_seed(424243 * seed + 31 * m + 7 * n + k)
    rnd = lambda *s: torch.randn(*s, generator=g)
    a = rnd(m, n) * 0.1 * (1.0 + torch.rand(m, 1, generator=g)) + 0.02 * rnd(1, n)
    b = rnd(m, k) * 0.5 * (1.0 + torch.rand(1, k, generator=g)) + 0.1 * rnd(m, 1)
    return a.half(), b.half(), rnd(n, k)


# ---------------------------------------------------------------------------------------------------------------
# emulations of the kernels' arithmetic (CPU, for tests/test_gemm_host.py): fp32 torch ops at the kernels' rounding
# points.  The order of the fp32 sums differs from the hardware's; the bounds do not depend on it.
# ---------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _c(v):
    return torch.tensor(v, dtype=torch.float32)


def emulate_gelu(x):
    """act.h gelu_erf2 on fp32 x (1 / den and exp2 correctly rounded here, 1 ulp on the device)."""
    kpw, knw2 = _c(0.3275911) * _c(0.70710678118654752440), _c(-0.5) * _c(1.44269504088896340736)
    ax = x.abs()
    t = 1.0 / _fma(ax, kpw, _c(1.0))
    p = _fma(t, _c(0.5) * _c(1.061405429), _c(0.5) * _c(-1.453152027))
    for coef in (1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, _c(0.5) * _c(coef))
    e = torch.exp2((x * x) * knw2)
    qn = _fma(-(p * t), e, _c(0.5))
    return _fma(ax, qn, 0.5 * x)


def emulate(kind, a, w, bias=None, scale=None, resid=None, stats=None, c1=None, form="persistent"):
    """The epilogue arithmetic of gemm_epilogue_lds_impl ("persistent") or gemm_epilogue_t ("small") -> list of
    outputs in their storage types."""
    acc = a.float() @ w.float().t()
    b = torch.zeros(w.shape[0]) if bias is None else bias
    if kind in ("ln_bias_f16", "ln_gelu_f16"):
        x = _fma(stats[:, 1:], _fma(-stats[:, :1], c1[None, :], acc), b)
        return [(emulate_gelu(x) if kind == "ln_gelu_f16" else x).half()]
    if kind == "affine_f32":
        return [_fma(acc, scale, b)]
    if kind == "affine_relu_f16":
        return [_fma(acc, scale, b).clamp_min(0.0).half()]
    x = acc + b
    if kind == "bias_f32":
        return [x]
    if kind == "bias_f16":
        return [x.half()]
    if kind == "gelu_f16":
        return [emulate_gelu(x).half()]
    if kind == "dual":
        return [x.half(), emulate_gelu(x).half()]
    if kind == "resid_f32":
        return [resid + x if scale is None else _fma(scale, x, resid)]
    if kind == "resid_f16":
        r = resid.half()
        if form == "small":
            return [_fma(torch.ones_like(b) if scale is None else scale, x, r.float()).half()]
        sx = (x if scale is None else scale * x).half()
        return [(sx.double() + r.double()).half()]     # the exact sum of two fp16 numbers, rounded once
    raise ValueError(kind)


def emulate_slices(rows):
    """gemm.hip:373-386 on stored fp16 rows [m, n] -> stats_part [n / 64, m, 2] fp32."""
    x = rows.float().reshape(rows.shape[0], -1, 8, 8)          # [m, slice, lane of the line, 8 values]
    s1 = torch.zeros_like(x[..., 0])
    for e in range(8):
        s1 = s1 + x[..., e]
    mean = s1.sum(-1) * (1.0 / 64.0)
    m2 = torch.zeros_like(s1)
    for e in range(8):
        dv = x[..., e] - mean[..., None]
        m2 = _fma(dv, dv, m2)
    return torch.stack([mean, m2.sum(-1)], -1).permute(1, 0, 2).contiguous()


def emulate_finalize(part, eps):
    """ln_stats_finalize_kernel on stats_part [P, m, 2] fp32 -> [m, 2] fp32."""
    p = part.shape[0]
    ms = torch.zeros_like(part[0, :, 0])
    for i in range(p):
        ms = ms + part[i, :, 0]
    mean = ms / float(p)
    m2 = torch.zeros_like(ms)
    for i in range(p):
        dm = part[i, :, 0] - mean
        m2 = m2 + (part[i, :, 1] + (64.0 * dm) * dm)
    var = m2 / (64.0 * float(p))
    return torch.stack([mean, 1.0 / torch.sqrt(var + _c(eps))], 1)


def emulate_tn(a, b, old=None, accumulate=0):
    m, n, k = a.shape[0], a.shape[1], b.shape[1]
    splits, rows = tn_plan(m, n, k)
    tot = None
    for s in range(splits):
        part = a[s * rows:(s + 1) * rows].float().t() @ b[s * rows:(s + 1) * rows].float()
        tot = part if tot is None else tot + part
    return tot + old if accumulate else tot
