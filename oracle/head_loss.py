"""Float64 references, error bounds, fp32 emulations of the reduction orders and a list of kernel mistakes for the
kernels that close the HSimCLR training step and finish an embedding: hcir_bn1d_fwd / _bwd (csrc/augment.hip),
hcir_triplet_margin_fwd / _bwd, hcir_mse_fwd / _bwd (csrc/train.hip), hcir_l2_normalize, hcir_convert_f32
(csrc/rownorm.hip).  Plain torch, any device.  tests/test_head_loss_host.py shows the bounds honest (the emulations
stay inside) and sharp (every mistake is seen); tests/test_head_loss_elements_gpu.py holds the kernels to them through
oracle.attention.ratio (err / bound <= 1).

u = 2^-24 (fp32 unit roundoff), h = 2^-11 (fp16), z = 2^-24 (the smallest fp16 subnormal).  Every bound is linear and
worst case: each rounding costs u times the magnitude of what is rounded; second order is covered by 1 + 2^-9 where
bounds multiply.  No constant is set against the emulation: every figure below is a count of roundings.  For the record,
the fp32 emulations below reach, over every family and shape of the GPU tests and three seeds (profiles/
head_loss_bounds.txt): bn1d mean 0.46, rstd 0.38, running_var 0.46, dbeta 0.44, dgamma 0.52 of their bounds; triplet dist
0.27, row_loss 0.33, loss 0.14; mse loss 0.08; l2_normalize 0.24; an fp16 output reaches the half-ulp of its store (0.99).

bn1d, x fp32 [rows, f].  Four row lanes take rows rl, rl + 4, ...; P = ceil(rows / 4) rows per lane; D = P + 3.
  mean   P - 1 additions in a lane (the first is to a zero), 3 additions of the lane partials in lane order, one
         division:                        |mean - mu| <= D u sum|x| / rows = b_mean
  var    second pass d = x - mean (the kernel's mean, 1 rounding, twice in d d), P fused multiply-adds, 3 additions, one
         division: D + 3 roundings on sum (x - mean)^2 = rows (var64 + (mean - mu)^2):
                                          |var - var64| <= (D + 3) u (var64 + b_mean^2) + b_mean^2 = b_var
  rstd   = 1 / sqrt(var + eps): the sum, the root, the reciprocal:
                                          |rstd - rstd64| <= rstd64 (b_var / (2 (var64 + eps)) + 4 u)
  running  (1 - momentum) old + momentum new, new = mean or m2 / (rows - 1) (rows = 1: the biased variance, 0):
         the factor, the product, the fused sum: momentum b_new + 4 u (|(1 - momentum) old| + |momentum new|)
  y      from the kernel's own save_mean, save_rstd: g = gamma rstd, y64 = relu?((x - mean) g + beta):
                                          |y32 - y64| <= 4 u |x - mean| |g| + 2 u |beta| + 2^-126
         (x - mean, g, the fused product-sum: 3 on the first term, 1 on beta; the bound leaves one more on each);
         y16 adds h |y64| + z.  Under ReLU an element whose unclamped y64 is below minus that bound must be exactly 0.
  dbeta, dgamma   terms g = fl(dy dy_scale) [relu_out_f16 > 0] and g xh, xh = fl(fl(x - mean) rstd): the fp32 values the
         kernel forms (bit-equal in torch fp32), summed in float64.  P additions or fused multiply-adds per lane and 3
         of the partials, at most D roundings:          |sum - sum64| <= D u sum|terms|
         (the roundings inside a term are held by the autograd check below).
  dx     from the kernel's own dgamma, dbeta: k = gamma rstd / rows, dx64 = k (rows g - dbeta - xh dgamma):
                                          |dx - dx64| <= h |dx64| + 8 u |k| (rows |g| + |dbeta| + |xh| |dgamma|) + z
         (g, rows g, - dbeta, the fused - xh dgamma, k twice, the product: 7 on g; xh twice: 6 on the last term).
  truth  F.batch_norm(training=True) (+ ReLU) in float64 and its autograd (rows >= 2: torch refuses one row); y and dx
         are held to the elementwise bound plus the statistics and sum bounds carried through to first order, as
         oracle.bn2d.truth_f64 does.  The ReLU mask is the kernel's own y16 > 0.

triplet, a, p, n fp32 [b, d], eps and margin as their fp32 values.  One wavefront per row, lane l takes columns l + 64 j.
  dist   t = fl(fl(a - p) + eps): |t - t64| <= u (|a - p| + |t|); Q = ceil(d / 64) fused multiply-adds per lane, 6
         butterfly levels: |s - s64| <= (Q + 6) u s64 + 2 u sum |t| (|a - p| + |t|) = b_s;  the root:
                                          |dist - dist64| <= b_s / (2 dist64) + u dist64
  row_loss = max(dp - dn + margin, 0):  b_dp + b_dn + 2 u (dp + dn + |margin|)   (max is 1-Lipschitz)
  loss   from the kernel's own row_loss: ceil(b / 256) additions per thread, 8 tree levels, fl(1 / b) and the product:
                                          (ceil(b / 256) + 10) u sum|row_loss| / b
  da, dp, dn   from the kernel's own dist, active = the kernel's own row_loss > 0 (the forward check holds row_loss: a
         row within its bound of the hinge may fall on either side), gs = grad_out / b, up = t / dist:
         e_up = u (|a - p| + 2 |t|) / dist;  |dp| : |gs| (e_up + 2 u |up|);  |da| : |gs| (e_up + e_un + 3 u (|up| + |un|)).
         An inactive row is exactly 0.

mse, n elements.  blocks = min(max(ceil(n / 4096), 1), 256), T = ceil(n / (256 blocks)) trips of a thread.
  loss   fl(x - y) squared (2), T fused multiply-adds, 8 tree levels, mean_kernel over the partials (1 + 8), fl(1 / n)
         and the product (2):             |loss - loss64| <= (T + 21) u loss64
  dx = 2 (x - y) grad_out / n: the difference, the product, the division, (float) n: 4 u |dx64| + 2^-126;  dy == -dx
         bit for bit.

l2_normalize, x fp32 [n, d], d % 4 == 0.  Lane l takes x[4 (l + 64 j) + e], C = 4 ceil(d / 256) fused multiply-adds, 6
  butterfly levels (the row_invnorm chain), the root, max(., eps), one division:
                                          |y - y64| <= |y64| ((C + 6) / 2 + 2) u (1 + 2^-9) + 2^-126
  y64 = x / max(||x||, eps); the fp16 copy adds h |y64| + z.  A zero row gives exactly 0.  The inputs keep sum x^2 of
  every nonzero row inside the fp32 range, between 2^-100 and 3e38 (|x| from 1e-15 to 1e15 at d <= 2048): above it the
  kernel returns 0 for a finite row; a square below 2^-126 is rounded by at most 2^-150, less than u^2 of such a sum,
  and a sum of nothing but such squares would have no relative bound.

convert: bit-equal to x.to(dtype) of torch on the CPU (round to nearest even), NaN by isnan.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.attention import H16, SECOND, U32, Z16, f32, ratio  # noqa: F401  (ratio is re-exported)

EPS, MOMENTUM = f32(1e-5), f32(0.1)
TINY = 1e-300
MIN32 = 2.0 ** -126
NAN = float("nan")
BN_COLS = 64

BN_SHAPES = [(1, 1), (2, 64), (3, 65), (4, 100), (5, 192), (9, 768), (258, 65), (1023, 100), (258, 768), (1023, 64),
             (5, 1), (1, 100)]                                          # (rows, f)
BN_SCALES = (None, 2.0 ** -7, 3.0)
TRIPLET_SHAPES = [(1, 1), (1, 512), (3, 63), (4, 64), (5, 65), (258, 130), (258, 1), (5, 512), (4, 130), (3, 64)]
MARGINS = (f32(0.7), f32(0.05))
TRIPLET_EPS = f32(1e-7)
TRIPLET_GRAD = 3.0
MSE_SIZES = [1, 255, 256, 257, 4097, 256 * 4096 + 3 * 4096 + 5]
MSE_GRAD = 0.5
L2_SHAPES = [(1, 4), (5, 252), (4, 256), (7, 260), (3, 768), (9, 2048)]
L2_EPS = f32(1e-12)
CONVERT_SIZES = [1, 2, 3, 4, 5, 1023, 1025, 4096 * 1024 + 1027]


def cdiv(a, b):
    return -(-a // b)


def bn_depth(rows):
    return cdiv(rows, 4) + 3


def _holds(cond):
    return 0.0 if bool(cond) else float("inf")


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "large_mean", "constant", "scaled", "random_buffers")


def _shape_family(x, family):
    """x ~ N(0, 1) [rows, cols] -> the family's map (columns are the axis of the per-column kernels)"""
    cols = x.shape[1]
    if family == "large_mean":
        x = 50.0 + x
    elif family == "constant":
        x = x.clone()
        x[:, ::7] = 1.5                # sums of 1.5 are exact up to 2^23 rows: the mean is 1.5, the variance 0
    elif family == "scaled":
        s = torch.full((cols,), 1e3, device=x.device)
        s[1::2] = 1e-3
        x = x * s
    return x


def make_bn1d(family, rows, f, seed=0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, device=device)
    rand = lambda *s: torch.rand(*s, generator=g, device=device)
    p = dict(x=_shape_family(randn(rows, f), family), dy=randn(rows, f), gamma=rand(f) + 0.5, beta=0.2 * randn(f),
             rm=torch.zeros(f, device=device), rv=torch.ones(f, device=device))
    if family == "random_buffers":
        p["rm"], p["rv"] = randn(f), rand(f) + 0.5
    return p


def exact_bn1d(rows, f, device="cpu"):
    """small-integer fp32 maps: every partial sum is an integer below 2^24; mean 0, rstd 1, gamma 1"""
    r = torch.arange(rows, device=device)[:, None]
    c = torch.arange(f, device=device)[None, :]
    return dict(dy=(((7 * r + c) % 5) - 2).float(), x=(((3 * r + 5 * c) % 7) - 3).float(),
                y16=torch.where((r + 2 * c) % 3 == 0, 0.0, 1.0).half().to(device),
                gamma=torch.ones(f, device=device), mean=torch.zeros(f, device=device), rstd=torch.ones(f, device=device))


def hot_rows(rows):
    return sorted({r for r in (0, 3, 4, rows - 1) if 0 <= r < rows})


def make_rows(family, n, d, seed=0, device="cpu", count=1):
    """`count` matrices [n, d] of the family (triplet, mse, l2_normalize)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return [_shape_family(torch.randn(n, d, generator=g, device=device), family) for _ in range(count)]


def make_triplet(family, b, d, seed=0, device="cpu"):
    """anchor, positive, negative.  p - a = 0.5 N; n - a = 0.05 N' in the even rows (active: dn < dp) and 3 N' in the odd
    ones (inactive: dn > dp + margin); row 0: p == a exactly and n at distance 0.01, active under both margins"""
    a, dp, dn = make_rows(family, b, d, seed, device, 3)
    if family == "large_mean":
        dp, dn = dp - 50.0, dn - 50.0
    c = torch.where(torch.arange(b, device=device) % 2 == 0, 0.05, 3.0)[:, None]
    p, n = a + 0.5 * dp, a + c * dn
    p[0] = a[0]
    n[0] = a[0] + (0.01 / d ** 0.5) * (1.0 - 2.0 * (torch.arange(d, device=device) % 2))
    return a, p, n


def make_l2(n, d, seed=0, device="cpu", eps=L2_EPS):
    """N(0, 1) rows; from the last row up, as far as n reaches and leaving row 0 as it is: a zero row, a row below eps,
    rows scaled by 1e-15 and 1e15"""
    x = make_rows("normal", n, d, seed, device)[0]
    for row, s in zip(range(n - 1, 0, -1), (0.0, 0.01 * eps, 1e-15, 1e15)):
        x[row] *= s
    return x


def convert_input(n, device="cpu"):
    """N(0, 1) scaled over 80 binades, with the special values planted from element 0 (the vector body, when n > 4) and
    again at the end (the scalar tail, when n % 4 != 0): +-0, fp16 subnormals, overflow to +-inf, +-inf, NaN, exact ties
    of both formats (1 + 2^-11: to even, down; 1 + 3 2^-11: up; 1 + 2^-8, 1 + 3 2^-8 for bf16; 65520: fp16 tie to inf)"""
    g = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=g) * 2.0 ** torch.randint(-40, 40, (n,), generator=g).float()
    special = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25, 65519.99, 65520.0,
                            -65520.0, 1e10, -1e10, float("inf"), float("-inf"), NAN, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
                            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -11), 3.4e38, -3.4e38, 1e-40, 2.0 ** -149,
                            NAN, float("-inf"), 1 + 2.0 ** -8, 1 + 2.0 ** -11, 3 * 2.0 ** -25, 65520.0])
    k = min(n, special.numel())
    x[:k] = special[:k]
    if n > special.numel():
        x[n - k:] = special.flip(0)[:k].flip(0)
    return x.to(device)


# ---------------------------------------------------------------------------------------------------------------
# bn1d: float64 references with bounds
# ---------------------------------------------------------------------------------------------------------------
def stats_f64(x):
    xd = x.double()
    mean = xd.mean(0)
    return mean, ((xd - mean) ** 2).mean(0)


def stat_bounds(x, var):
    rows = x.shape[0]
    d = bn_depth(rows)
    b_mean = (d * U32 * x.double().abs().sum(0) / rows).clamp_min(TINY)
    return b_mean, ((d + 3) * U32 * (var + b_mean ** 2) + b_mean ** 2).clamp_min(TINY)


def rstd_f64(var, eps=EPS):
    return (var + eps).rsqrt()


def rstd_bound(var, b_var, eps=EPS):
    return rstd_f64(var, eps) * (b_var / (2 * (var + eps)) + 4 * U32) * SECOND


def _unb(rows, unbiased=True):
    return rows / (rows - 1) if unbiased and rows > 1 else 1.0


def running_f64(rm, rv, mean, var, rows, momentum=MOMENTUM, unbiased=True):
    return ((1 - momentum) * rm.double() + momentum * mean,
            (1 - momentum) * rv.double() + momentum * var * _unb(rows, unbiased))


def running_bounds(rm, rv, mean, var, b_mean, b_var, rows, momentum=MOMENTUM):
    unb = _unb(rows)
    return (momentum * b_mean + 4 * U32 * ((1 - momentum) * rm.double().abs() + momentum * mean.abs()),
            momentum * b_var * unb + 4 * U32 * ((1 - momentum) * rv.double().abs() + momentum * var * unb))


def fwd_f64(x, mean, rstd, gamma, beta, relu):
    """-> (y64, fp32 bound, fp16 bound, must_be_zero) from the vectors given (the kernel's own, or float64)"""
    xc = x.double() - mean.double()
    g = gamma.double() * rstd.double()
    pre = xc * g + beta.double()
    b32 = 4 * U32 * xc.abs() * g.abs() + 2 * U32 * beta.double().abs() + MIN32
    y = pre.clamp_min(0.0) if relu else pre
    return y, b32, b32 + H16 * y.abs() + Z16, (pre < -b32) if relu else None


def bwd_terms(dy, x, mean, rstd, scale, y16):
    """the fp32 terms the kernel forms: g = fl(dy scale) [y16 > 0], xh = fl(fl(x - mean) rstd)"""
    g = dy.float() if scale is None else dy.float() * torch.tensor(scale, dtype=torch.float32, device=dy.device)
    if y16 is not None:
        g = torch.where(y16 > 0, g, torch.zeros_like(g))
    return g, (x.float() - mean.float()) * rstd.float()


def sums_f64(g, xh, rows):
    """-> (dbeta, bound, dgamma, bound): float64 sums of the fp32 terms"""
    d = bn_depth(rows)
    gd, t = g.double(), g.double() * xh.double()
    return (gd.sum(0), (d * U32 * gd.abs().sum(0)).clamp_min(TINY), t.sum(0), (d * U32 * t.abs().sum(0)).clamp_min(TINY))


def dx_f64(dy, x, mean, rstd, gamma, dgamma, dbeta, scale, y16):
    rows = x.shape[0]
    g = dy.double() * (1.0 if scale is None else f32(scale))
    if y16 is not None:
        g = g * (y16 > 0)
    xh = (x.double() - mean.double()) * rstd.double()
    k = gamma.double() * rstd.double() / rows
    dx = k * (rows * g - dbeta.double() - xh * dgamma.double())
    mag = rows * g.abs() + dbeta.double().abs() + xh.abs() * dgamma.double().abs()
    return dx, H16 * dx.abs() + 8 * U32 * k.abs() * mag + Z16


def truth_f64(x, dy, gamma, beta, relu, mask, scale, eps=EPS):
    """F.batch_norm(training=True) (+ ReLU) and its autograd in float64 -> {name: (value, fp16 bound)} of y and dx, the
    statistics and sum bounds carried through to first order.  mask: the kernel's y16 > 0 where the backward is given
    the ReLU output, else None (the gradient of the BatchNorm alone)."""
    rows = x.shape[0]
    d = bn_depth(rows)
    xd = x.double().requires_grad_(True)
    w, b = gamma.double(), beta.double()
    with torch.backends.cudnn.flags(enabled=False):
        pre = F.batch_norm(xd, None, None, w, b, True, 0.0, eps)
    g = dy.double() * (1.0 if scale is None else f32(scale))
    (pre * mask if mask is not None else pre).backward(g)
    y = pre.detach().clamp_min(0.0) if relu else pre.detach()
    mean, var = stats_f64(x)
    rstd = rstd_f64(var, eps)
    b_mean, b_var = stat_bounds(x, var)
    b_rstd = rstd_bound(var, b_var, eps)
    xc = x.double() - mean
    _, _, y_bound, _ = fwd_f64(x, mean, rstd, gamma, beta, relu)
    y_bound = y_bound + SECOND * (w.abs() * rstd * b_mean + xc.abs() * w.abs() * b_rstd)
    if mask is not None:
        g = g * mask
    xh = xc * rstd
    b_xh = rstd * b_mean + xc.abs() * b_rstd + 3 * U32 * xh.abs()
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    b_dbeta = (d + 1) * U32 * g.abs().sum(0)
    b_dgamma = (d + 1) * U32 * (g * xh).abs().sum(0) + (g.abs() * b_xh).sum(0)
    _, dx_bound = dx_f64(dy, x, mean, rstd, gamma, dgamma, dbeta, scale, None if mask is None else mask.half())
    a = w * rstd
    inner = g - dbeta / rows - xh * dgamma / rows
    dx_bound = dx_bound + SECOND * (w.abs() * b_rstd * inner.abs() +
                                    a.abs() * (b_dbeta / rows + (b_xh * dgamma.abs() + xh.abs() * b_dgamma) / rows))
    return {"y": (y, y_bound), "dx": (xd.grad, dx_bound)}


# ---------------------------------------------------------------------------------------------------------------
# bn1d: the kernels' order in fp32 (x [rows, n]: any n columns), and the chain in float64 with a mistake on request
# ---------------------------------------------------------------------------------------------------------------
def _lanes(v):
    """[rows, n] -> [P, 4, n], rows past the last zero"""
    rows, n = v.shape
    p = cdiv(rows, 4)
    return torch.cat([v, v.new_zeros(4 * p - rows, n)]).view(p, 4, n)


def _lane_order(part):
    return ((part[0] + part[1]) + part[2]) + part[3]


def emulate_bn1d(prob, relu, scale=None, use_mask=False, eps=EPS, momentum=MOMENTUM):
    """fp32 CPU, operation by operation as bn1d_fwd_kernel and bn1d_bwd_kernel order them -> {name: tensor}"""
    x, dy, gamma, beta = (prob[k].float() for k in ("x", "dy", "gamma", "beta"))
    rows, n = x.shape
    fr = torch.tensor(float(rows))
    xp = _lanes(x)
    valid = (torch.arange(xp.shape[0] * 4).view(-1, 4) < rows)[..., None]
    s = torch.zeros(4, n)
    for i in range(xp.shape[0]):
        s = s + xp[i]
    mean = _lane_order(s) / fr
    v = torch.zeros(4, n)
    for i in range(xp.shape[0]):
        dlt = xp[i] - mean
        v = torch.where(valid[i], _fma(dlt, dlt, v), v)
    m2 = _lane_order(v)
    var = m2 / fr
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps))
    mom = torch.tensor(momentum)
    out = {"save_mean": mean, "save_rstd": rstd,
           "running_mean": _fma(mom, mean, (1.0 - mom) * prob["rm"].float()),
           "running_var": _fma(mom, m2 / (fr - 1.0) if rows > 1 else var, (1.0 - mom) * prob["rv"].float())}
    y = _fma(x - mean, gamma * rstd, beta)
    y = y.clamp_min(0.0) if relu else y
    out["y32"], out["y16"] = y, y.half()
    g, xh = bwd_terms(dy, x, mean, rstd, scale, out["y16"] if use_mask else None)
    gp, xhp = _lanes(g), _lanes(xh)
    s1, s2 = torch.zeros(4, n), torch.zeros(4, n)
    for i in range(gp.shape[0]):
        s1 = s1 + gp[i]
        s2 = _fma(gp[i], xhp[i], s2)
    out["dbeta"], out["dgamma"] = _lane_order(s1), _lane_order(s2)
    k = gamma * rstd / fr
    out["dx"] = (k * _fma(-xh, out["dgamma"], fr * g - out["dbeta"])).half()
    return out


MISTAKES = ("bn1d: one row of a ragged last pass dropped from the sums",
            "bn1d: the last column block skipped",
            "bn1d: the biased variance in running_var (the unbiased one at rows = 1)",
            "bn1d: dy_scale missing from dgamma",
            "bn1d: the ReLU mask ignored in the backward",
            "triplet: eps left out of the difference",
            "triplet: dp with the wrong sign",
            "mse: divided by n - 1",
            "l2_normalize: nrm not clamped at eps")
LOST, LASTBLOCK, BIASED, NOSCALE, NOMASK, NOEPS, DPSIGN, NM1, NOCLAMP = MISTAKES


def _r32(t):
    """a vector the kernel stores in fp32 and reads back"""
    return t.float().double()


def chain_bn1d(prob, relu, scale=None, use_mask=False, mistake=None, given=None, eps=EPS):
    """every output of the forward and the backward in float64, each step from the (fp32-stored) vectors of the step
    before.  given = (mean, rstd, y16): the backward alone.  An unwritten element is NaN."""
    x, dy = prob["x"], prob["dy"]
    rows, f = x.shape
    xd = x.double()
    keep = torch.ones(rows, dtype=torch.bool, device=x.device)
    if mistake == LOST and rows % 4:
        keep[rows - 1] = False
    out = {}
    if given is None:
        mean = _r32(xd[keep].sum(0) / rows)
        var = ((xd[keep] - mean) ** 2).sum(0) / rows
        rstd = _r32(rstd_f64(var, eps))
        out["save_mean"], out["save_rstd"] = mean, rstd
        out["running_mean"], out["running_var"] = running_f64(prob["rm"], prob["rv"], mean, var, rows,
                                                              unbiased=mistake != BIASED)
        if mistake == BIASED and rows == 1:       # the unbiased variance of one row: m2 / 0
            out["running_var"] = out["running_var"] + float("inf")
        y = fwd_f64(x, mean, rstd, prob["gamma"], prob["beta"], relu)[0]
        out["y32"], out["y16"] = y, y
        y16 = y.half() if use_mask else None
    else:
        mean, rstd, y16 = given[0].double(), given[1].double(), given[2]
    mask16 = None if mistake == NOMASK else y16
    sc = 1.0 if scale is None else f32(scale)
    g = dy.double() * sc
    if mask16 is not None:
        g = g * (mask16 > 0)
    xh = (xd - mean) * rstd
    gk = g * keep[:, None]
    out["dbeta"] = _r32(gk.sum(0))
    out["dgamma"] = _r32((gk * xh).sum(0) / (sc if mistake == NOSCALE else 1.0))
    out["dx"] = dx_f64(dy, x, mean, rstd, prob["gamma"], out["dgamma"], out["dbeta"], scale, mask16)[0]
    if mistake == LASTBLOCK:
        lo = (cdiv(f, BN_COLS) - 1) * BN_COLS
        for name in out:
            out[name] = out[name].clone()
            out[name][..., lo:] = NAN
    return out


def check_bn1d(prob, relu, out, scale=None, use_mask=False, truth=True, eps=EPS):
    """The checks of tests/test_head_loss_elements_gpu.py on one forward + backward -> {check: err / bound}; out as the
    kernels (or chain_bn1d, emulate_bn1d) give it; y32 / y16 may be missing (an output not asked for)."""
    x, dy, gamma, beta = prob["x"], prob["dy"], prob["gamma"], prob["beta"]
    rows = x.shape[0]
    mean, var = stats_f64(x)
    b_mean, b_var = stat_bounds(x, var)
    w = {"save_mean": ratio(out["save_mean"], mean, b_mean),
         "save_rstd": ratio(out["save_rstd"], rstd_f64(var, eps), rstd_bound(var, b_var, eps))}
    if out.get("running_mean") is not None:
        rm, rv = running_f64(prob["rm"], prob["rv"], mean, var, rows)
        b_rm, b_rv = running_bounds(prob["rm"], prob["rv"], mean, var, b_mean, b_var, rows)
        w["running_mean"], w["running_var"] = ratio(out["running_mean"], rm, b_rm), ratio(out["running_var"], rv, b_rv)
    k_mean, k_rstd = out["save_mean"], out["save_rstd"]
    y64, b32, b16, zero = fwd_f64(x, k_mean, k_rstd, gamma, beta, relu)
    for name, b in (("y32", b32), ("y16", b16)):
        if out.get(name) is not None:
            w[name] = ratio(out[name], y64, b)
            if relu:
                w[name + " >= 0"] = _holds((out[name] >= 0).all())
                w[name + " == 0 below -bound"] = _holds((out[name][zero] == 0).all())
    y16 = None
    if use_mask:
        y16 = out["y16"] if out["y16"].dtype == torch.float16 else out["y16"].half()
    w.update(check_bn1d_bwd(dy, x, gamma, k_mean, k_rstd, scale, y16, out))
    if truth and rows > 1:
        t = truth_f64(x, dy, gamma, beta, relu, (y16 > 0) if use_mask else None, scale, eps)
        if out.get("y16") is not None:
            w["y16 / autograd"] = ratio(out["y16"], *t["y"])
        w["dx / autograd"] = ratio(out["dx"], *t["dx"])
    return w


def check_bn1d_bwd(dy, x, gamma, mean, rstd, scale, y16, out):
    g, xh = bwd_terms(dy, x, mean, rstd, scale, y16)
    dbeta, b_dbeta, dgamma, b_dgamma = sums_f64(g, xh, x.shape[0])
    return {"dbeta": ratio(out["dbeta"], dbeta, b_dbeta), "dgamma": ratio(out["dgamma"], dgamma, b_dgamma),
            "dx": ratio(out["dx"], *dx_f64(dy, x, mean, rstd, gamma, out["dgamma"], out["dbeta"], scale, y16))}


# ---------------------------------------------------------------------------------------------------------------
# triplet margin loss
# ---------------------------------------------------------------------------------------------------------------
def _dist_f64(a, p, eps):
    """-> (t, dist, bound)"""
    dlt = a.double() - p.double()
    t = dlt + eps
    d = a.shape[1]
    s = (t * t).sum(1)
    b_s = (cdiv(d, 64) + 6) * U32 * s + 2 * U32 * (t.abs() * (dlt.abs() + t.abs())).sum(1)
    dist = s.sqrt()
    return t, dist, (SECOND * b_s / (2 * dist.clamp_min(TINY)) + U32 * dist).clamp_min(TINY)


def triplet_fwd_f64(a, p, n, margin, eps=TRIPLET_EPS):
    """-> {dist: (ref [2, b], bound), row_loss: (ref [b], bound)}"""
    _, dp, b_dp = _dist_f64(a, p, eps)
    _, dn, b_dn = _dist_f64(a, n, eps)
    return {"dist": (torch.stack([dp, dn]), torch.stack([b_dp, b_dn])),
            "row_loss": ((dp - dn + margin).clamp_min(0.0), b_dp + b_dn + 2 * U32 * (dp + dn + abs(margin)))}


def mean_f64(v, count, scale_roundings=2):
    """mean_kernel over v with scale 1 / count -> (ref, bound)"""
    n = v.numel()
    return v.double().sum() / count, ((cdiv(n, 256) + 8 + scale_roundings) * U32 * v.double().abs().sum() / count
                                      ).clamp_min(TINY)


def triplet_bwd_f64(a, p, n, row_loss, dist, grad_out, eps=TRIPLET_EPS, dp_sign=-1.0):
    """from the kernel's own row_loss and dist -> {da, dp, dn: (ref, bound)}"""
    b = a.shape[0]
    gs = (row_loss.double() > 0)[:, None] * (grad_out / b)
    out = {}
    u, e = [], []
    for other, dst in ((p, dist[0]), (n, dist[1])):
        dlt = a.double() - other.double()
        t = dlt + eps
        dd = dst.double()[:, None]
        u.append(t / dd)
        e.append(U32 * (dlt.abs() + 2 * t.abs()) / dd.abs())
    out["da"] = (gs * (u[0] - u[1]), (gs.abs() * (e[0] + e[1] + 3 * U32 * (u[0].abs() + u[1].abs()))).clamp_min(TINY))
    out["dp"] = (dp_sign * gs * u[0], (gs.abs() * (e[0] + 2 * U32 * u[0].abs())).clamp_min(TINY))
    out["dn"] = (gs * u[1], (gs.abs() * (e[1] + 2 * U32 * u[1].abs())).clamp_min(TINY))
    return out


def chain_triplet(a, p, n, margin, grad_out=TRIPLET_GRAD, eps=TRIPLET_EPS, mistake=None):
    fw = triplet_fwd_f64(a, p, n, margin, 0.0 if mistake == NOEPS else eps)
    out = {"dist": _r32(fw["dist"][0]), "row_loss": _r32(fw["row_loss"][0])}
    out["loss"] = out["row_loss"].sum() / a.shape[0]
    bw = triplet_bwd_f64(a, p, n, out["row_loss"], out["dist"], grad_out, 0.0 if mistake == NOEPS else eps,
                         1.0 if mistake == DPSIGN else -1.0)
    out.update({k: v[0] for k, v in bw.items()})
    return out


def _wave_chain(t):
    """[rows, d] terms t t summed as a wavefront does: lane l over columns l + 64 j (fused), butterfly 32 .. 1"""
    rows, d = t.shape
    q = cdiv(d, 64)
    tp = torch.cat([t, t.new_zeros(rows, 64 * q - d)], 1).view(rows, q, 64)
    s = torch.zeros(rows, 64)
    for j in range(q):
        s = _fma(tp[:, j], tp[:, j], s)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, torch.arange(64) ^ o]
    return s[:, 0]


def emulate_mean(v, count):
    n = v.numel()
    vp = torch.cat([v.float().flatten(), torch.zeros(256 * cdiv(n, 256) - n)]).view(-1, 256)
    s = torch.zeros(256)
    for i in range(vp.shape[0]):
        s = s + vp[i]
    o = 128
    while o:
        s = s[:o] + s[o:2 * o]
        o //= 2
    return s[0] * (torch.tensor(1.0) / torch.tensor(float(count)))


def emulate_triplet(a, p, n, margin, grad_out=TRIPLET_GRAD, eps=TRIPLET_EPS):
    a, p, n = a.float(), p.float(), n.float()
    e = torch.tensor(eps)
    tp, tn = (a - p) + e, (a - n) + e
    dp, dn = torch.sqrt(_wave_chain(tp)), torch.sqrt(_wave_chain(tn))
    row_loss = ((dp - dn) + torch.tensor(margin)).clamp_min(0.0)
    gs = torch.where(row_loss > 0, torch.tensor(grad_out) / torch.tensor(float(a.shape[0])), torch.tensor(0.0))[:, None]
    up, un = tp / dp[:, None], tn / dn[:, None]
    return {"dist": torch.stack([dp, dn]), "row_loss": row_loss, "loss": emulate_mean(row_loss, a.shape[0]),
            "da": gs * (up - un), "dp": -gs * up, "dn": gs * un}


def check_triplet(a, p, n, margin, out, grad_out=TRIPLET_GRAD, eps=TRIPLET_EPS):
    fw = triplet_fwd_f64(a, p, n, margin, eps)
    w = {"dist": ratio(out["dist"], *fw["dist"]), "row_loss": ratio(out["row_loss"], *fw["row_loss"]),
         "row_loss >= 0": _holds((out["row_loss"] >= 0).all()),
         "loss": ratio(out["loss"].reshape(()), *mean_f64(out["row_loss"], a.shape[0]))}
    truth = fw["row_loss"][0].mean()
    w["loss / truth"] = ratio(out["loss"].reshape(()), truth, mean_f64(fw["row_loss"][0], a.shape[0])[1] +
                              fw["row_loss"][1].mean())
    bw = triplet_bwd_f64(a, p, n, out["row_loss"], out["dist"], grad_out, eps)
    for k in ("da", "dp", "dn"):
        w[k] = ratio(out[k], *bw[k])
        w[k + " inactive == 0"] = _holds((out[k][~(out["row_loss"] > 0)] == 0).all())
    return w


# ---------------------------------------------------------------------------------------------------------------
# mse
# ---------------------------------------------------------------------------------------------------------------
def mse_blocks(n):
    return min(max(cdiv(n, 4096), 1), 256)


def mse_trips(n):
    return cdiv(n, 256 * mse_blocks(n))


def mse_f64(x, y, grad_out=MSE_GRAD, denom=None):
    """-> {loss, dx: (ref, bound)}; x, y flat"""
    n = x.numel()
    dlt = x.double() - y.double()
    loss = (dlt * dlt).sum() / (n if denom is None else denom)
    dx = 2.0 * dlt * grad_out / (n if denom is None else denom)
    return {"loss": (loss, ((mse_trips(n) + 21) * U32 * loss).clamp_min(TINY)), "dx": (dx, 4 * U32 * dx.abs() + MIN32)}


def emulate_mse(x, y, grad_out=MSE_GRAD):
    n = x.numel()
    blocks, trips = mse_blocks(n), mse_trips(n)
    dlt = x.float() - y.float()
    dp = torch.cat([dlt, torch.zeros(trips * blocks * 256 - n)]).view(trips, blocks, 256)
    s = torch.zeros(blocks, 256)
    for i in range(trips):
        s = _fma(dp[i], dp[i], s)
    o = 128
    while o:
        s = s[:, :o] + s[:, o:2 * o]
        o //= 2
    dx = 2.0 * dlt * torch.tensor(grad_out) / torch.tensor(float(n))
    return {"loss": emulate_mean(s[:, 0], n), "dx": dx, "dy": -dx}


def chain_mse(x, y, grad_out=MSE_GRAD, mistake=None):
    r = mse_f64(x, y, grad_out, x.numel() - 1 if mistake == NM1 else None)
    return {"loss": r["loss"][0], "dx": r["dx"][0], "dy": -r["dx"][0]}


def check_mse(x, y, out, grad_out=MSE_GRAD):
    r = mse_f64(x, y, grad_out)
    w = {}
    if out.get("loss") is not None:
        w["loss"] = ratio(out["loss"].reshape(()), *r["loss"])
    if out.get("dx") is not None:
        w["dx"] = ratio(out["dx"], *r["dx"])
    if out.get("dy") is not None:
        w["dy"] = ratio(out["dy"], -r["dx"][0], r["dx"][1])
    if out.get("dx") is not None and out.get("dy") is not None:
        if out["dx"].dtype == torch.float32:
            w["dy == -dx"] = _holds(torch.equal(out["dy"].view(torch.int32), (-out["dx"]).view(torch.int32)))
        else:
            w["dy == -dx"] = _holds(torch.equal(out["dy"], -out["dx"]))
    return w


# ---------------------------------------------------------------------------------------------------------------
# l2_normalize, convert
# ---------------------------------------------------------------------------------------------------------------
def l2_f64(x, eps=L2_EPS, clamp=True):
    """-> (y64, fp32 bound, fp16 bound)"""
    d = x.shape[1]
    nrm = x.double().norm(dim=1, keepdim=True)
    y = x.double() / (nrm.clamp_min(eps) if clamp else nrm)
    b32 = y.abs() * ((4 * cdiv(d, 256) + 6) / 2 + 2) * U32 * SECOND + MIN32
    return y, b32, b32 + H16 * y.abs() + Z16


def emulate_l2(x, eps=L2_EPS):
    n, d = x.shape
    c = cdiv(d, 256)
    xp = torch.cat([x.float(), torch.zeros(n, 256 * c - d)], 1).view(n, c, 64, 4)
    s = torch.zeros(n, 64)
    for j in range(c):
        for e in range(4):
            s = _fma(xp[:, j, :, e], xp[:, j, :, e], s)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, torch.arange(64) ^ o]
    y = x.float() / torch.sqrt(s[:, :1]).clamp_min(eps)
    return {"y32": y, "y16": y.half()}


def chain_l2(x, eps=L2_EPS, mistake=None):
    y = l2_f64(x, eps, mistake != NOCLAMP)[0]
    return {"y32": y, "y16": y}


def check_l2(x, out, eps=L2_EPS):
    y, b32, b16 = l2_f64(x, eps)
    zero = (x == 0).all(1)
    w = {}
    for name, b in (("y32", b32), ("y16", b16)):
        if out.get(name) is not None:
            w[name] = ratio(out[name], y, b)
            w[name + " zero row == 0"] = _holds((out[name][zero] == 0).all())
    return w


def convert_ref(x, dtype):
    return x.detach().cpu().to(dtype)


def check_convert(x, got, dtype):
    """bit for bit, NaN by isnan"""
    want, got = convert_ref(x, dtype), got.detach().cpu()
    nan = torch.isnan(want)
    same = torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))
    return {"bits": _holds(got.dtype == dtype and same)}
