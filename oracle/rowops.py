"""oracle.rowops — float64 references, per-element error bounds and arithmetic emulations of the row-wise ViT kernels
(TEST INFRASTRUCTURE ONLY).

Ground truth for hcir_layernorm_f16 / hcir_cls_head / hcir_patch_mean (csrc/norm.hip) and hcir_layernorm_bwd(_fused) /
hcir_gelu_fwd_f16 / hcir_gelu_bwd_f16 / hcir_gelu_bwd_colsum_f16 / hcir_colsum_f16 / hcir_add_f32_f16 (csrc/train.hip,
csrc/act.h), taken on the tensors the kernels read: x fp16 or fp32 widened exactly, dy / u / dh fp16, gamma / beta fp32.

Notation   u = 2^-24 (fp32), h = 2^-11 (fp16), z = 2^-24 (the fp16 subnormal spacing) as in oracle.gemm; a sum whose
longest chain of additions has `depth` roundings is off by at most depth u sum|terms| (first order); every bound is
multiplied by (1 + 2^-9) for products of two first-order terms.  G = ceil(d / 256) is the number of LIVE column groups
of a row (a dead group adds exact zeros), c = x - mean, xhat = c rstd, y = xhat gamma + beta.

statistics, forward (norm.hip ln_row)
  d_mean = (G + 7) u mean|x| + u|mean|     per lane (v0 + v1) + (v2 + v3) (2), s += over G groups (the first add to 0 is
                                           exact: G - 1), six wave_sum steps (6)  (norm.hip:32,34); the division  (:34)
  var'   = var + d_mean^2                  the variance is taken about the COMPUTED mean: sum (x - m)^2 / d = var + (m - mean)^2
  d_var  = d_mean^2 + (4 G + 9) u var'     c = x - m rounded (u; 2u on c c), 4 G fmas per lane, wave_sum (6), the
                                           division (1)                                               (norm.hip:42-43,47)
  d_rstd = rstd (d_var / (2 (var + eps)) + 6u)          var + eps, sqrtf, 1 / x                              (norm.hip:47)
statistics, backward (train.hip layernorm_bwd_kernel): the same with the plain chain s += x over 4 G elements per lane
  d_mean = (4 G + 5) u mean|x| + u|mean|                                                           (train.hip:127,135)
  d_var, d_rstd as above                                                                           (train.hip:143-148)

LayerNorm forward   e_y = |gamma| (rstd (d_mean + 3u|c|) + |c| d_rstd) + u|y|
                    x - mean (the mean's error, u), * rstd (rstd's error, u), * gamma (u), + beta (u|y|)   (norm.hip:70)
  hcir_layernorm_f16   e_y + h|y| + z                                                        the fp16 store (norm.hip:70)
  hcir_cls_head        without l2: e_y (fp32), e_y + h|y| + z (fp16); without gamma / beta e_y = 0: a copy    (:107,122)
    with l2: N = max(|y|_2, 1e-12), n2 = sum y^2;  d_n2 = sum 2|y| e_y + (4 G + 6) u n2   fmas, wave_sum (norm.hip:110,113)
             e_o = e_y / N + |y| / N (d_n2 / (2 n2) + 5u)         sqrtf and 1 / x at 1 ulp each, v * inv   (norm.hip:113,122)
             the returned rows have |o|_2 = 1 to ((4 G + 6) / 2 + 6) u  (fp32; the sum's error, sqrtf, 1 / x, the product
             and the store), + h + z sqrt(d) for the fp16 copy: norm_bound()
  hcir_patch_mean      out = sum_i y_i / (t - 1):  [ sum_i e_y_i + (ceil((t - 1) / 4) + 3) u sum_i |y_i| ] / (t - 1)
                       the wave's own rows in order, (p0 + p1) + (p2 + p3), the division              (norm.hip:165,180)

LayerNorm backward  g = dy gamma, mg = mean(g), mgx = mean(g xhat), inner = g - mg - xhat mgx, dx = rstd inner
  e_xh    = rstd (d_mean + 2u|c|) + |c| d_rstd                                                          (train.hip:158)
  e_g     = u|g|                                                                                        (train.hip:159)
  d_mg    = (4 G + 7) u mean|g| + u|mg|           e_g, the chain of 4 G, wave_sum; the division    (train.hip:164,170)
  d_mgx   = mean(e_g|xhat| + |g| e_xh) + (4 G + 7) u mean|g xhat| + u|mgx|      fmas               (train.hip:165,170)
  e_inner = e_g + d_mg + u|g - mg| + e_xh|mgx| + |xhat| d_mgx + e_xh d_mgx + u|xhat mgx| + u|inner|       (train.hip:178)
            e_xh d_mgx is second order, but it is multiplied by rstd: on a constant row (rstd = 1000, xhat = mgx = 0 in
            float64, the computed xhat = -rstd (m - mean) in every column) it is the whole error of xhat mgx
  dres_out  rstd e_inner + |inner| d_rstd + u|dx| + u|dx + dres_in|                                (train.hip:178,180)
  dres16    fp16 of the RETURNED fp32 dres_out, bit for bit: no float64 bound                           (train.hip:186)
  column sums, three stages: a wave's rows in order (trips = ceil(rows / (4 blocks)), train.hip:100,160-161,187), the
  four waves through LDS in wave order (3, train.hip:205-207), colsum_finalize_kernel: lane q over parts q, q + 16, ...
  (ceil(blocks / 16)) and the sixteen lanes in order (15) (train.hip:237,243):  D = trips + ceil(blocks / 16) + 18
  dbeta        D u sum_r|dy|                       (+ u|old + dbeta| with accumulate, train.hip:244)
  dgamma       sum_r |dy| e_xh + D u sum_r|dy xhat|          one fma per row                            (train.hip:160)
  dres_colsum  D u sum_r|dres16| on the STORED fp16 copy; always assigned                          (train.hip:187,496)

GELU forward   e_gelu(u) + h|g| + z on an exact fp16 u (oracle.gemm.gelu_err)                           (train.hip:26-28)
GELU backward  gelu'(x) = Phi(x) + x phi(x); q = erfc(|x| / sqrt 2) / 2, e = exp(-x^2 / 2)                 (act.h:34-46)
  e_q       = 0.75e-7 + e E_PT + q (2^-19 + 1.5 u x^2 + u)    Abramowitz-Stegun, P(t) t (v_rcp_f32, Horner), v_exp_f32 and
                                                            its argument, p t * e: the terms of e_gelu     (act.h:38-44)
  e_grad(x) = e_q + u Phi [x >= 0: 1 - q]                                                                 (act.h:45)
              + |x phi| (2^-19 + 1.5 u x^2 + 1.5u)          e again; x * (1 / sqrt(2 pi)) and the constant  (act.h:46)
              + u|gelu'|                                    the last fma                                   (act.h:46)
  du        |dh| e_grad + u|dh gelu'| + h|du| + z                                                     (train.hip:43,300)
  For |x| >= 16 exp2 underflows to 0: gelu = max(x, 0) and gelu' = [x > 0] exactly (act.h:10), tested as equalities.

column sums (colsum_kernel / gelu_bwd_colsum_kernel on the stored du): row lane rl adds rows r0 + rl + 8 i in order
  (ceil(rows_per / 8), train.hip:260-263), the 8 row lanes in order (8, :273), the finalize tree over
  hcir_colsum_chunks(m) parts (ceil(chunks / 16) + 15):   D u sum|x|,  + u|old + sum| with accumulate.

hcir_add_f32_f16: one IEEE fp32 add and one round-to-nearest-even conversion; compared bit for bit, no bound.
"""
from __future__ import annotations

import math

import torch

from oracle.attention import E_EXP2, H16, SECOND, U32, Z16, ratio  # noqa: F401  (ratio is re-exported)
from oracle.gemm import E_AS, E_PT, LN_EPS, SQRT1_2, emulate_gelu, gelu_err, gelu_f64, gelu_tanh_f64  # noqa: F401

F32, F16 = 0, 1            # hcir_dtype
TINY = 1e-300              # a bound of exactly 0 (a copy): err / TINY is 0 or inf
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def cdiv(a, b):
    return -(-a // b)


def groups(d):
    return cdiv(d, 256)


def nv_of(d):
    """template NV of norm.hip's DISPATCH_NV"""
    g = groups(d)
    return g if g in (3, 4, 5) else (2 if g <= 2 else 8)


def nj_of(d):
    """template NJ of hcir_layernorm_bwd_fused"""
    g = groups(d)
    return g if g <= 4 else (8 if g <= 8 else 16)


def ln_bwd_blocks(rows):
    return max(1, min(1024, cdiv(rows, 64)))


def colsum_chunks(m):
    return max(1, min(256, cdiv(m, 512)))


def ln_bwd_depth(rows):
    blocks = ln_bwd_blocks(rows)
    return cdiv(rows, 4 * blocks) + cdiv(blocks, 16) + 18


def colsum_depth(m):
    chunks = colsum_chunks(m)
    return cdiv(cdiv(m, chunks), 8) + 8 + cdiv(chunks, 16) + 15


# ---------------------------------------------------------------------------------------------------------------
# float64 references with bounds
# ---------------------------------------------------------------------------------------------------------------
class Stats:
    """mean, var, rstd [rows, 1] float64 of x [rows, d] with their bounds; `bwd` selects the backward's mean chain."""

    def __init__(self, x, eps=LN_EPS, bwd=False):
        x = x.double()
        d = x.shape[-1]
        g = groups(d)
        self.mean = x.mean(-1, keepdim=True)
        self.c = x - self.mean
        self.var = (self.c * self.c).mean(-1, keepdim=True)
        self.rstd = (self.var + eps).rsqrt()
        self.d_mean = ((4 * g + 5) if bwd else (g + 7)) * U32 * x.abs().mean(-1, keepdim=True) + U32 * self.mean.abs()
        self.d_var = self.d_mean ** 2 + (4 * g + 9) * U32 * (self.var + self.d_mean ** 2)
        self.d_rstd = self.rstd * (self.d_var / (2 * (self.var + eps)) + 6 * U32)
        self.xhat = self.c * self.rstd


def ln_apply(x, mean, rstd, gamma, beta):
    return (x.double() - mean) * rstd * gamma.double() + beta.double()


def ln_rows_f64(x, gamma, beta, eps=LN_EPS):
    """(y, e_y): the fp32 value (v - mean) * rstd * g + b of norm.hip before any store; gamma None: (x, 0)."""
    if gamma is None:
        return x.double(), torch.zeros_like(x, dtype=torch.float64)
    st = Stats(x, eps)
    ga = gamma.double().abs()
    y = ln_apply(x, st.mean, st.rstd, gamma, beta)
    e_y = ga * (st.rstd * (st.d_mean + 3 * U32 * st.c.abs()) + st.c.abs() * st.d_rstd) + U32 * y.abs()
    return y, e_y


def f16_store(v):
    return H16 * v.abs() + Z16


def layernorm_f64(x, gamma, beta, eps=LN_EPS):
    """hcir_layernorm_f16 -> (reference, bound)"""
    y, e_y = ln_rows_f64(x, gamma, beta, eps)
    return y, SECOND * (e_y + f16_store(y))


def cls_head_f64(tok, gamma, beta, eps=LN_EPS, l2=0, token=0):
    """hcir_cls_head on tok [b, t, d] -> (reference, bound of emb_f32, bound of emb_f16)"""
    y, e_y = ln_rows_f64(tok[:, token], gamma, beta, eps)
    if l2:
        g = groups(tok.shape[-1])
        n2 = (y * y).sum(-1, keepdim=True)
        norm = n2.sqrt().clamp_min(1e-12)
        d_n2 = (2 * y.abs() * e_y).sum(-1, keepdim=True) + (4 * g + 6) * U32 * n2
        y, e_y = y / norm, e_y / norm + y.abs() / norm * (d_n2 / (2 * n2).clamp_min(1e-300) + 5 * U32)
    return y, (SECOND * e_y).clamp_min(TINY), (SECOND * (e_y + f16_store(y))).clamp_min(TINY)


def norm_bound(d, fp16):
    """| |o|_2 - 1 | of a returned l2-normalised row"""
    return SECOND * (((4 * groups(d) + 6) / 2 + 6) * U32 + ((H16 + Z16 * math.sqrt(d)) if fp16 else 0.0))


def patch_mean_f64(tok, gamma, beta, eps=LN_EPS, first=1, div=None, rows=None):
    """hcir_patch_mean on tok [b, t, d] -> (reference, bound); first / div / rows let a test restate a mistake."""
    b, t, d = tok.shape
    y, e_y = ln_rows_f64(tok.reshape(b * t, d), gamma, beta, eps)
    y, e_y = y.view(b, t, d), e_y.view(b, t, d)
    sel = list(range(first, t)) if rows is None else rows
    ref = y[:, sel].sum(1) / float(t - 1 if div is None else div)
    bound = (e_y[:, 1:].sum(1) + (cdiv(t - 1, 4) + 3) * U32 * y[:, 1:].abs().sum(1)) / float(t - 1)
    return ref, (SECOND * bound).clamp_min(TINY)


def colsum_f64(x, old=None, accumulate=0, depth=None, rows=None):
    """column sums of the stored fp16 x [m, n] -> (reference, bound); `rows` restricts the reference (mistakes)."""
    xd = x.double()
    depth = colsum_depth(x.shape[0]) if depth is None else depth
    ref = (xd if rows is None else xd[rows]).sum(0)
    bound = depth * U32 * xd.abs().sum(0)
    if accumulate:
        ref = ref + old.double()
        bound = bound + U32 * ref.abs()
    return ref, (SECOND * bound).clamp_min(TINY)


def layernorm_bwd_f64(x, dy, gamma, eps=LN_EPS, dres_in=None, old=None, accumulate=0):
    """hcir_layernorm_bwd -> dict(dres=(ref, bound), dgamma=(...), dbeta=(...)) and the pieces a test may restate a
    mistake from (st, g, mg, mgx, dx).  old = (dgamma, dbeta) before the call, with accumulate."""
    st = Stats(x, eps, bwd=True)
    d = x.shape[-1]
    grp = groups(d)
    dyd, ga = dy.double(), gamma.double()
    xh = st.xhat
    e_xh = st.rstd * (st.d_mean + 2 * U32 * st.c.abs()) + st.c.abs() * st.d_rstd
    g = dyd * ga
    e_g = U32 * g.abs()
    mg = g.mean(-1, keepdim=True)
    mgx = (g * xh).mean(-1, keepdim=True)
    d_mg = (4 * grp + 7) * U32 * g.abs().mean(-1, keepdim=True) + U32 * mg.abs()
    d_mgx = (e_g * xh.abs() + g.abs() * e_xh).mean(-1, keepdim=True) + \
        (4 * grp + 7) * U32 * (g * xh).abs().mean(-1, keepdim=True) + U32 * mgx.abs()
    inner = g - mg - xh * mgx
    e_inner = e_g + d_mg + U32 * (g - mg).abs() + e_xh * mgx.abs() + xh.abs() * d_mgx + e_xh * d_mgx + \
        U32 * (xh * mgx).abs() + U32 * inner.abs()
    dx = st.rstd * inner
    out = dx if dres_in is None else dx + dres_in.double()
    e_out = st.rstd * e_inner + inner.abs() * st.d_rstd + U32 * dx.abs() + U32 * out.abs()
    depth = ln_bwd_depth(x.shape[0])
    dgamma = (dyd * xh).sum(0)
    e_dgamma = (dyd.abs() * e_xh).sum(0) + depth * U32 * (dyd * xh).abs().sum(0)
    dbeta = dyd.sum(0)
    e_dbeta = depth * U32 * dyd.abs().sum(0)
    if accumulate:
        dgamma, dbeta = dgamma + old[0].double(), dbeta + old[1].double()
        e_dgamma, e_dbeta = e_dgamma + U32 * dgamma.abs(), e_dbeta + U32 * dbeta.abs()
    return dict(dres=(out, SECOND * e_out), dgamma=(dgamma, (SECOND * e_dgamma).clamp_min(TINY)),
                dbeta=(dbeta, (SECOND * e_dbeta).clamp_min(TINY)), st=st, g=g, mg=mg, mgx=mgx, dx=dx, xh=xh)


def dres_colsum_f64(dres16, rows=None):
    """dres_colsum of the STORED fp16 copy [rows, d] -> (reference, bound)"""
    return colsum_f64(dres16, depth=ln_bwd_depth(dres16.shape[0]), rows=rows)


def gelu_fwd_f64(u):
    g = gelu_f64(u.double())
    return g, SECOND * (gelu_err(u.double()) + f16_store(g))


def _q_e(x):
    return 0.5 * torch.special.erfc(x.abs() * SQRT1_2), torch.exp(-0.5 * x * x)


def gelu_grad_f64(x):
    q, e = _q_e(x)
    return torch.where(x >= 0, 1.0 - q, q) + x * e * INV_SQRT_2PI


def gelu_grad_err(x):
    """e_grad(x): the error of act.h's gelu_erf_grad on an exact fp32 x."""
    q, e = _q_e(x)
    rel_e = E_EXP2 + 1.5 * U32 * x * x
    e_q = E_AS + e * E_PT + q * (rel_e + U32)
    return e_q + U32 * torch.where(x >= 0, 1.0 - q, torch.zeros_like(q)) + \
        (x * e * INV_SQRT_2PI).abs() * (rel_e + 1.5 * U32) + U32 * gelu_grad_f64(x).abs()


def gelu_bwd_f64(u, dh):
    x, g = u.double(), dh.double()
    gp = gelu_grad_f64(x)
    du = g * gp
    return du, SECOND * (g.abs() * gelu_grad_err(x) + U32 * du.abs() + f16_store(du))


def all_finite_f16():
    """every fp16 code in code order, the 2048 non-finite ones replaced by small distinct finite values"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16).clone()
    bad = ~torch.isfinite(v)
    v[bad] = (torch.arange(int(bad.sum()), dtype=torch.float32) / 256.0 - 4.0).half()
    return v


DH_PATTERNS = ("one", "mixed")


def dh_pattern(name, n=65536):
    """`one`: 1 everywhere.  `mixed`: both signs, fp16 subnormals, values up to 5e4 (|gelu'| <= 1.13: the product stays
    finite in fp16), zeros."""
    if name == "one":
        return torch.ones(n, dtype=torch.float16)
    i = torch.arange(n)
    mag = torch.tensor([1.0, 2.0 ** -24, 3.0 * 2.0 ** -22, 5e4, 0.37, 2.0 ** -14, 0.0, 311.0, 1e-3])[i % 9]
    vary = torch.where(mag < 4e4, 1.0 + (i % 5).float() * 0.125, torch.ones(n))
    return (mag * vary * torch.where(i % 4 == 1, -1.0, 1.0)).half()


# ---------------------------------------------------------------------------------------------------------------
# input families: fp32 / fp16 CPU tensors
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "offset", "constant", "cancel", "marker")


def marker_pos(rows, d, step=5):
    """the one-hot column of marker row i: distinct for d consecutive rows (step prime to d), shifted per run"""
    i = torch.arange(rows)
    step = step if math.gcd(step, d) == 1 else 1
    return (i * step + (i // d) * 3 + 1) % d


def make_problem(family, rows, d, seed=0, cancel_row=None):
    """dict(x [rows, d] fp32 (tests round it to fp16 for fp16 input), gamma, beta [d] fp32, dy [rows, d] fp16,
    dres_in [rows, d] fp32, old_dgamma, old_dbeta [d] fp32, cancel_row).
    plain     randn rows with standard deviations from 0.01 to 3 (eps matters on the small ones) and small offsets
    offset    row mean 50 x the row's standard deviation
    constant  rows of one repeated value (0.1, -0.3, 0.7, ... scaled per row): variance 0, rstd = eps^-1/2; beta is 0
              on every other column so that the error of the mean is not hidden behind the fp16 rounding of beta
    cancel    plain with beta = -gamma xhat of row cancel_row (default rows // 2): y of that row is about 0; and
              dres_in = -dx of that row: its dres_out is about 0
    marker    one-hot x rows and one-hot dy rows (marker_pos with steps 5 and 7), values distinct per row and column."""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 104729 * d + 15485863 * FAMILIES.index(family))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    uni = lambda *s: torch.rand(*s, generator=gen)
    scale = 10.0 ** (uni(rows, 1) * 2.5 - 2.0)
    x = rnd(rows, d) * scale + rnd(rows, 1) * 0.3 * scale
    gamma = (1.0 + 0.3 * rnd(d)) * torch.where(torch.arange(d) % 7 == 3, -1.0, 1.0)
    beta = 0.5 * rnd(d)
    dy = rnd(rows, d) * (0.5 + uni(rows, 1))
    dres_in = rnd(rows, d) + 0.5 * rnd(rows, 1)
    cancel_row = rows // 2 if cancel_row is None else cancel_row
    if family == "offset":
        sd = 0.5 + uni(rows, 1)
        x = rnd(rows, d) * sd + 50.0 * sd * torch.where(torch.arange(rows)[:, None] % 2 == 0, 1.0, -1.0)
    elif family == "constant":
        vals = torch.tensor([0.1, -0.3, 0.7, 1.1, -2.3])[torch.arange(rows) % 5] * (1.0 + torch.arange(rows) // 5)
        x = vals[:, None].expand(rows, d).clone()
        beta[::2] = 0.0
    elif family == "marker":
        r = torch.arange(rows)
        x = torch.zeros(rows, d)
        px = marker_pos(rows, d, 5)
        x[r, px] = 1.0 + (r % 13).float() * 0.25 + (px % 11).float() * 0.0625
        dy = torch.zeros(rows, d)
        py = marker_pos(rows, d, 7)
        dy[r, py] = (0.5 + (r % 7).float() * 0.125 + (py % 5).float() * 0.03125) * torch.where(r % 3 == 0, -1.0, 1.0)
    elif family not in ("plain", "cancel"):
        raise ValueError(family)
    x, dy = x.float(), dy.half()
    p = dict(x=x, gamma=gamma.float(), beta=beta.float(), dy=dy, dres_in=dres_in.float(), old_dgamma=rnd(d) * 3.0,
             old_dbeta=rnd(d) * 3.0, cancel_row=cancel_row)
    if family == "cancel":
        p = apply_cancel(p, x)
    return p


MAT_FAMILIES = ("plain", "zero_mean", "marker")


def make_matrix(family, m, n):
    """(fp16 [m, n], old [n] fp32) for the column sums: randn with uneven columns around 0.25; the same around 0;
    one-hot rows (marker_pos)"""
    g = torch.Generator().manual_seed(31 * m + n)
    x = torch.randn(m, n, generator=g) * (0.5 + torch.rand(1, n, generator=g))
    if family == "plain":
        x = x + 0.25
    elif family == "marker":
        r = torch.arange(m)
        x = torch.zeros(m, n)
        x[r, marker_pos(m, n, 5)] = (1.0 + (r % 13).float() * 0.25) * torch.where(r % 3 == 0, -1.0, 1.0)
    elif family != "zero_mean":
        raise ValueError(family)
    return x.half(), torch.randn(n, generator=g) * 3.0


def apply_cancel(p, x):
    """beta and dres_in of the `cancel` family for the rows x the kernel will read (x itself, or its fp16 rounding)"""
    r = p["cancel_row"]
    st = Stats(x[r:r + 1])
    beta = (-p["gamma"].double() * st.xhat[0]).float()
    dx = layernorm_bwd_f64(x[r:r + 1], p["dy"][r:r + 1], p["gamma"])["dx"][0]
    dres_in = p["dres_in"].clone()
    dres_in[r] = (-dx).float()
    return {**p, "beta": beta, "dres_in": dres_in}


# ---------------------------------------------------------------------------------------------------------------
# emulations of the kernels' arithmetic (CPU, for tests/test_rowops_host.py): fp32 torch ops in the kernels' order
# ---------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _c(v):
    return torch.tensor(v, dtype=torch.float32)


_XOR = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def wave_sum(v):
    """common.h wave_sum over the last axis (64 lanes): the xor butterfly; every lane ends with the same value"""
    for idx in _XOR:
        v = v + v[..., idx]
    return v[..., :1]


def lanes(x, ng):
    """[rows, d] -> [rows, ng, 64, 4] fp32 (element 4 (lane + 64 j) + e at [j][lane][e]) and the live mask"""
    rows, d = x.shape
    buf = torch.zeros(rows, ng * 256, dtype=torch.float32)
    buf[:, :d] = x.float()
    live = (torch.arange(ng * 256) < d).view(1, ng, 64, 4).expand(rows, -1, -1, -1)
    return buf.view(rows, ng, 64, 4), live


def unlanes(v, d):
    return v.reshape(v.shape[0], -1)[:, :d]


def emulate_ln_row(x, eps=LN_EPS):
    """norm.hip ln_row -> (v [rows, NV, 64, 4], live, mean [rows, 1, 1, 1], rstd)"""
    d = x.shape[1]
    v, live = lanes(x, nv_of(d))
    s = torch.zeros(v.shape[0], 64)
    for j in range(v.shape[1]):
        s = s + ((v[:, j, :, 0] + v[:, j, :, 1]) + (v[:, j, :, 2] + v[:, j, :, 3]))
    mean = wave_sum(s) / _c(float(d))
    q = torch.zeros_like(s)
    for j in range(v.shape[1]):
        for e in range(4):
            c = v[:, j, :, e] - mean
            q = torch.where(live[:, j, :, e], _fma(c, c, q), q)
    rstd = _c(1.0) / torch.sqrt(wave_sum(q) / _c(float(d)) + _c(eps))
    return v, live, mean[:, :, None, None], rstd[:, :, None, None]


def _emulate_rows(x, gamma, beta, eps):
    """the fp32 rows (v - mean) * rstd * g + b in lane layout (the affine's last step as an fma), or x itself"""
    d = x.shape[1]
    if gamma is None:
        return lanes(x, nv_of(d))[0]
    v, live, mean, rstd = emulate_ln_row(x, eps)
    g, b = lanes(gamma[None], nv_of(d))[0], lanes(beta[None], nv_of(d))[0]
    return torch.where(live, _fma((v - mean) * rstd, g, b), v)


def emulate_layernorm(x, gamma, beta, eps=LN_EPS):
    return unlanes(_emulate_rows(x, gamma, beta, eps), x.shape[1]).half()


def emulate_cls_head(tok, gamma, beta, eps=LN_EPS, l2=0):
    """-> (emb_f32, emb_f16)"""
    d = tok.shape[-1]
    v = _emulate_rows(tok[:, 0], gamma, beta, eps)
    inv = _c(1.0)
    if l2:
        ss = torch.zeros(v.shape[0], 64)
        for j in range(v.shape[1]):
            for e in range(4):
                ss = _fma(v[:, j, :, e], v[:, j, :, e], ss)
        inv = (_c(1.0) / torch.sqrt(wave_sum(ss)).clamp_min(_c(1e-12)))[:, :, None, None]
    o = unlanes(v * inv, d)
    return o, o.half()


def emulate_patch_mean(tok, gamma, beta, eps=LN_EPS):
    b, t, d = tok.shape
    y = unlanes(_emulate_rows(tok.reshape(b * t, d), gamma, beta, eps), d).view(b, t, d)
    part = []
    for wave in range(4):
        acc = torch.zeros(b, d)
        for i in range(1 + wave, t, 4):
            acc = acc + y[:, i]
        part.append(acc)
    return ((part[0] + part[1]) + (part[2] + part[3])) / _c(float(t - 1))


def emulate_finalize(part, old=None, accumulate=0):
    """colsum_finalize_kernel on part [parts, n] fp32"""
    parts, n = part.shape
    red = []
    for q in range(16):
        s = torch.zeros(n)
        for p in range(q, parts, 16):
            s = s + part[p]
        red.append(s)
    t = red[0]
    for q in range(1, 16):
        t = t + red[q]
    return old + t if accumulate else t


def emulate_layernorm_bwd(x, dy, gamma, eps=LN_EPS, dres_in=None, old=None, accumulate=0, fused=False):
    """layernorm_bwd_kernel + colsum_finalize_kernel -> dict(dres, dgamma, dbeta[, dres16, dres_colsum])"""
    rows, d = x.shape
    nj = nj_of(d)
    xv, live = lanes(x, nj)
    dv = lanes(dy, nj)[0]
    gm = lanes(gamma[None], nj)[0]
    rin = lanes(dres_in, nj)[0] if dres_in is not None else torch.zeros_like(xv)
    df = _c(float(d))
    s = torch.zeros(rows, 64)
    for j in range(nj):
        for e in range(4):
            s = s + xv[:, j, :, e]
    mean = (wave_sum(s) / df)[:, :, None, None]
    t = torch.where(live, xv - mean, torch.zeros_like(xv))
    v = torch.zeros(rows, 64)
    for j in range(nj):
        for e in range(4):
            v = _fma(t[:, j, :, e], t[:, j, :, e], v)
    rstd = (_c(1.0) / torch.sqrt(wave_sum(v) / df + _c(eps)))[:, :, None, None]
    xh = torch.where(live, (xv - mean) * rstd, torch.zeros_like(xv))
    g = dv * gm
    sg, sgx = torch.zeros(rows, 64), torch.zeros(rows, 64)
    for j in range(nj):
        for e in range(4):
            sg = sg + g[:, j, :, e]
            sgx = _fma(g[:, j, :, e], xh[:, j, :, e], sgx)
    mg, mgx = (wave_sum(sg) / df)[:, :, None, None], (wave_sum(sgx) / df)[:, :, None, None]
    o = rstd * _fma(-xh, mgx, g - mg) + rin
    o16 = o.half()
    # the wave's rows in order, the four waves in wave order, the finalize tree
    blocks = ln_bwd_blocks(rows)
    zero = torch.zeros(blocks, 4, nj, 64, 4)
    gsum, bsum, rsum = zero.clone(), zero.clone(), zero.clone()
    for r0 in range(0, rows, 4 * blocks):
        n = min(4 * blocks, rows - r0)
        pad = lambda a: torch.cat([a[r0:r0 + n], torch.zeros(4 * blocks - n, nj, 64, 4)]).view(blocks, 4, nj, 64, 4)
        gsum = _fma(pad(dv), pad(xh), gsum)
        bsum = bsum + pad(dv)
        rsum = rsum + pad(o16.float())
    out = dict(dres=unlanes(o, d))
    for name, acc in (("dgamma", gsum), ("dbeta", bsum)) + ((("dres_colsum", rsum),) if fused else ()):
        part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
        prev = None if old is None else {"dgamma": old[0], "dbeta": old[1]}.get(name)
        out[name] = emulate_finalize(unlanes(part, d), prev, accumulate and name != "dres_colsum")
    if fused:
        out["dres16"] = unlanes(o16, d)
    return out


def emulate_colsum(x, old=None, accumulate=0):
    """colsum_kernel + colsum_finalize_kernel on fp16 x [m, n]"""
    m, n = x.shape
    chunks = colsum_chunks(m)
    rows_per = cdiv(m, chunks)
    trips = cdiv(rows_per, 8)
    buf = torch.zeros(chunks, trips * 8, n)
    for ch in range(chunks):
        seg = x[ch * rows_per:min(m, (ch + 1) * rows_per)].float()
        buf[ch, :seg.shape[0]] = seg
    buf = buf.view(chunks, trips, 8, n)
    acc = torch.zeros(chunks, 8, n)
    for i in range(trips):
        acc = acc + buf[:, i]
    s = torch.zeros(chunks, n)
    for w in range(8):
        s = s + acc[:, w]
    return emulate_finalize(s, old, accumulate)


def emulate_gelu_fwd(u):
    return emulate_gelu(u.float()).half()


def emulate_gelu_grad(x):
    """act.h gelu_erf_grad on fp32 x (1 / den and exp2 correctly rounded here, 1 ulp on the device)"""
    kpw, knw2 = _c(0.3275911) * _c(0.70710678118654752440), _c(-0.5) * _c(1.44269504088896340736)
    ax = x.abs()
    t = 1.0 / _fma(ax, kpw, _c(1.0))
    p = _fma(t, _c(0.5) * _c(1.061405429), _c(0.5) * _c(-1.453152027))
    for coef in (1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, _c(0.5) * _c(coef))
    e = torch.exp2(x * x * knw2)
    q = p * t * e
    cdf = torch.where(x >= 0, 1.0 - q, q)
    return _fma(x * _c(0.39894228040143267794), e, cdf)


def emulate_gelu_bwd(u, dh):
    return (dh.float() * emulate_gelu_grad(u.float())).half()
