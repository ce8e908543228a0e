"""Float64 references, error bounds, an fp32 emulation of the reduction order and a list of kernel mistakes for the
batch-statistics BatchNorm2d kernels (csrc/bn2d.hip, geometry csrc/bn2d_plan.h).  Plain torch, any device; the maps
are [M = B H W, C].  tests/test_bn2d_host.py shows the bounds honest (the emulation stays inside) and sharp (every
mistake is seen); tests/test_bn2d_elements_gpu.py holds the kernels to them.

u = 2^-24 (fp32 unit roundoff), h = 2^-11 (fp16), z = 2^-24 (the smallest fp16 subnormal: twice the error of a store
in the subnormal range).

plan(m, c)   bn2d_plan() restated, with the figures that say which branch of the kernels a shape reaches: passes per
  chunk (the trips of the reductions' row loop: the 4-row unrolled body of the statistics kernel runs from 5 on, since
  a lane's first row is its shift), rows of the last chunk, apply trips = ceil(passes / apply_blocks) (the grid stride
  of the elementwise kernels), per = ceil(chunks / 64) (chunks a finalize lane merges), and whether the chunk count
  was clamped by the grid cap.

Elementwise kernels, every element, from the kernel's own fp32 vectors (exact in float64):
  y    mu = save_mean, sc = save_rstd gamma, y64 = relu?((x - mu) sc + beta (+ r)):
         |y - y64| <= h |y64| + 4 u (|x - mu| |sc| + |beta| + |r|) + z
       roundings: x - mu (u |x - mu| |sc|), sc (the same), the fma (u (|x - mu| |sc| + |beta|)), the residual add
       (u (|x - mu| |sc| + |beta| + |r|)): at most 4 u on the first term, 2 u on beta, u on r; then one fp16 store.
       Under ReLU the stored value is max(v, 0): where y64 = 0 and the unclamped float64 value is <= -(the fp32 part
       of the bound) the kernel's v is <= 0 and y must be exactly 0.
  dx   a = gamma rstd, b = dbeta / M, cc = rstd dgamma / M (the kernel's dgamma, dbeta), dx64 = a (g - b - (x - mu) cc):
         |dx - dx64| <= h |dx64| + 8 u |a| (|g| + |b| + |x - mu| |cc|) + z
       roundings: a (1), fp32(1 / M) (1), b (1), rstd / M and cc (2), x - mu (1), the product, g - b, the difference and
       the final product (1 each): at most 4 on g, 6 on b, 8 on the last term.
  dresid  where(y > 0, dy, 0) or dy: bit-equal, no bound.

Plain sums (dbeta, dgamma): D u sum|terms| with D = passes per chunk + rpp + per + 6, the longest addition chain of the
  plan (a lane's rows, the pass rows in LDS, a finalize lane's chunks, the 6 levels of the wavefront tree; the three
  first additions to a zero leave room for the roundings of x - mean and of the rstd factor).  Worst case, linear: it
  does not see one lost row among 10^5.  The exact integer sums and the hot-row probes do.

Statistics, per channel, against float64 of the fp16 input (sigma^2 the biased variance):
         |mean - mu| <= STAT (|mu| + sigma),      |var - var64| <= STAT (sigma^2 + |mu| sigma),      STAT = 2^-19
  The constant is not derived.  It is set against the emulation below, which must stay within a quarter of it on every
  family and shape (the GPU's fma contraction and division need not match the emulation bit for bit), else it is raised
  to the next power of two.  At the house headroom of 16 u = 2^-20 the emulation reaches 0.33 (variance, M = 75,
  normal) and 0.23 (mean, M = 75, large_mean) over the sample of tests/test_bn2d_host.py (each shape's own channels,
  three seeds), 0.29 for the mean over other seeds: a workgroup's 32 pass rows merge one after the other, and each
  merge rounds a mean near |mu|.  At 2^-19 the sample stays at or below 0.17.
  rstd = (var + eps)^-1/2 follows with  rstd (b_var / (2 (var + eps)) + 8 u)  (the division by M, the sum with eps, the
  square root and the reciprocal), the running statistics with
  momentum b + 5 u (|(1 - momentum) old| + |momentum new|).

Ground truth: F.batch_norm(training=True) and its autograd in float64 (truth_f64); y and dx are held to the elementwise
  bound plus the statistics bounds carried through |gamma| rstd, |x - mu| |gamma| and, for dx, through dgamma and dbeta
  (first order, times 1 + 2^-9).  The ReLU mask of the gradient is the kernel's own y > 0: the forward check holds that
  mask; an element at |y64| below its bound may round to either side.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F

from oracle.attention import H16, SECOND, U32, Z16, f32, ratio  # noqa: F401  (ratio is re-exported)

THREADS, GRID_CAP, MIN_PASSES = 256, 8 * 256, 4      # csrc/bn2d_plan.h
EPS, MOMENTUM = f32(1e-5), f32(0.1)
STAT = 2.0 ** -19
HOT_TOL = 2.0 ** -20       # the hot-row probes: relative, against the closed form
TINY = 1e-300
NAN = float("nan")

SMALL_SHAPES = [(2, 1, 1, 64), (3, 5, 5, 64), (4, 7, 7, 2048), (4, 14, 14, 256), (3, 28, 28, 128)]    # G1
CAPPED_SHAPES = [(101, 57, 57, 64), (49, 41, 41, 256), (49, 29, 29, 512), (15, 37, 37, 1024), (61, 13, 13, 2048)]
STRIDED_SHAPES = [(7, 73, 73, 128), (5, 67, 67, 192), (3, 67, 67, 320), (3, 61, 61, 384)]
PROBE_SHAPES = [(101, 57, 57, 64), (61, 13, 13, 2048), (3, 67, 67, 320)]
HOT = 1024.0


def cdiv(a, b):
    return -(-a // b)


def rows_of(shape):
    return shape[0] * shape[1] * shape[2]


class Plan(NamedTuple):
    cv: int
    wv_log2: int
    slabs: int
    rpp: int
    chunks: int
    rows_per_chunk: int
    apply_blocks: int
    chunk_passes: int      # passes per chunk: rows_per_chunk / rpp
    last_rows: int         # rows of the last chunk
    trips: int             # ceil(passes / apply_blocks): trips of the elementwise kernels' grid-stride loop
    per: int               # ceil(chunks / 64): chunks per finalize lane
    clamped: bool          # the chunk count was cut by the grid cap

    @property
    def depth(self):
        return self.chunk_passes + self.rpp + self.per + 6


def plan(m, c):
    assert m >= 2 and c >= 64 and c % 64 == 0 and c <= 1 << 16 and m < 1 << 31
    cv = c // 8
    wv_log2 = 6 if cv % 64 == 0 else 5 if cv % 32 == 0 else 4 if cv % 16 == 0 else 3
    slabs = cv >> wv_log2
    rpp = 4 * (64 >> wv_log2)
    cap = max(GRID_CAP // slabs, 1)
    passes = cdiv(m, rpp)
    wanted = cdiv(passes, MIN_PASSES)
    rows_per_chunk = cdiv(passes, min(wanted, cap)) * rpp
    chunks = cdiv(m, rows_per_chunk)
    apply_blocks = min(passes, cap)
    return Plan(cv, wv_log2, slabs, rpp, chunks, rows_per_chunk, apply_blocks, rows_per_chunk // rpp,
                m - (chunks - 1) * rows_per_chunk, cdiv(passes, apply_blocks), cdiv(chunks, 64), wanted > cap)


def probe_rows(m, p):
    last0 = (p.chunks - 1) * p.rows_per_chunk
    rows = {0, p.rpp - 1, p.rpp, p.rows_per_chunk - 1, p.rows_per_chunk, last0, m - 1, p.apply_blocks * p.rpp - 1,
            p.apply_blocks * p.rpp}
    return sorted(r for r in rows if 0 <= r < m)


# ---------------------------------------------------------------------------------------------------------------
# inputs: [M, C] maps (fp16) and [C] vectors (fp32), made on `device`
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "large_mean", "random_buffers", "scaled")


def make_problem(family, m, c, seed=0, device="cpu"):
    """normal: N(0, 1); large_mean: 100 + 0.25 N(0, 1); random_buffers: N(0, 1) with random running statistics;
    scaled: a per-channel scale in [0.01, 30] (log-uniform) and an offset in [-50, 50]."""
    g = torch.Generator(device=device).manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, device=device)
    rand = lambda *s: torch.rand(*s, generator=g, device=device)
    x = randn(m, c)
    if family == "large_mean":
        x = 100.0 + 0.25 * x
    elif family == "scaled":
        x = (100.0 * rand(c) - 50.0) + 0.01 * 3000.0 ** rand(c) * x
    p = dict(x=x.half(), resid=randn(m, c).half(), dy=randn(m, c).half(), gamma=rand(c) + 0.5, beta=0.2 * randn(c),
             rm=torch.zeros(c, device=device), rv=torch.ones(c, device=device))
    if family == "random_buffers":
        p["rm"], p["rv"] = randn(c), rand(c) + 0.5
    return p


def exact_problem(m, c, with_mask, device="cpu", c0=0):
    """small-integer fp16 maps whose every partial sum is an integer below 2^24; mean 0, rstd 1, gamma 1"""
    r = torch.arange(m, device=device)[:, None]
    ch = torch.arange(c0, c0 + c, device=device)[None, :]
    p = dict(dy=(((7 * r + ch) % 5) - 2).half(), x=(((3 * r + 5 * ch) % 7) - 3).half(),
             gamma=torch.ones(c, device=device), mean=torch.zeros(c, device=device), rstd=torch.ones(c, device=device))
    p["y"] = torch.where((r + 2 * ch) % 3 == 0, -1.0, 1.0).half() if with_mask else None
    return p


def exact_sums(p):
    """int64 (dbeta, dgamma) of an exact_problem"""
    g = p["dy"].long()
    if p["y"] is not None:
        g = g * (p["y"] > 0)
    return g.sum(0), (g * p["x"].long()).sum(0)


def hot_x(m, c, row, device="cpu"):
    x = torch.zeros(m, c, dtype=torch.float16, device=device)
    x[row] = HOT
    return x


def hot_stats(m, eps=EPS):
    """closed form (mean, rstd) of a map that is HOT in one row and 0 elsewhere"""
    mean = HOT / m
    return mean, (HOT * HOT * (m - 1) / (m * m) + eps) ** -0.5


def hot_dy(m, c, row, device="cpu", c0=0):
    dy = torch.zeros(m, c, dtype=torch.float16, device=device)
    dy[row] = ((torch.arange(c0, c0 + c, device=device) % 5) - 2).half()
    return dy


# ---------------------------------------------------------------------------------------------------------------
# float64 references with bounds
# ---------------------------------------------------------------------------------------------------------------
def stats_f64(x):
    """(mean, biased variance) float64 [C] of x [M, C]"""
    xd = x.double()
    mean = xd.mean(0)
    return mean, ((xd - mean) ** 2).mean(0)


def stat_bounds(mean, var):
    sigma = var.sqrt()
    return STAT * (mean.abs() + sigma).clamp_min(TINY), STAT * (var + mean.abs() * sigma).clamp_min(TINY)


def rstd_f64(var, eps=EPS):
    return (var + eps).rsqrt()


def rstd_bound(var, b_var, eps=EPS):
    return rstd_f64(var, eps) * (b_var / (2 * (var + eps)) + 8 * U32)


def running_f64(rm, rv, mean, var, m, momentum=MOMENTUM, unbiased=True):
    unb = m / (m - 1) if unbiased else 1.0
    return (1 - momentum) * rm.double() + momentum * mean, (1 - momentum) * rv.double() + momentum * var * unb


def running_bounds(rm, rv, mean, var, b_mean, b_var, m, momentum=MOMENTUM):
    unb = m / (m - 1)
    return (momentum * b_mean + 5 * U32 * ((1 - momentum) * rm.double().abs() + momentum * mean.abs()),
            momentum * b_var * unb + 5 * U32 * ((1 - momentum) * rv.double().abs() + momentum * var * unb))


def fwd_f64(x, mean, rstd, gamma, beta, resid=None, relu=False):
    """-> (y64, bound, must_be_zero): from the vectors given (the kernel's own fp32 ones, or float64)"""
    xc = x.double() - mean.double()
    sc = rstd.double() * gamma.double()
    pre = xc * sc + beta.double()
    mag = xc.abs() * sc.abs() + beta.double().abs()
    if resid is not None:
        pre = pre + resid.double()
        mag = mag + resid.double().abs()
    y = pre.clamp_min(0.0) if relu else pre
    fp32_part = 4 * U32 * mag
    return y, H16 * y.abs() + fp32_part + Z16, (pre <= -fp32_part) if relu else None


def masked(dy, y):
    """g = dy [y > 0], or dy without a ReLU"""
    return dy if y is None else torch.where(y > 0, dy, torch.zeros_like(dy))


def sums_f64(g, x, mean, rstd, depth):
    """-> (dbeta, its bound, dgamma, its bound, sum g (x - mean))"""
    gd = g.double()
    t = gd * (x.double() - mean.double())
    r = rstd.double()
    s2 = t.sum(0)
    return (gd.sum(0), (depth * U32 * gd.abs().sum(0)).clamp_min(TINY), r * s2,
            (depth * U32 * r.abs() * t.abs().sum(0)).clamp_min(TINY), s2)


def dx_f64(g, x, mean, rstd, gamma, dgamma, dbeta, m, inv=None):
    """-> (dx64, bound) from the vectors given; inv: the reciprocal the mean terms are scaled with (1 / M)"""
    inv = 1.0 / m if inv is None else inv
    xc = x.double() - mean.double()
    a = gamma.double() * rstd.double()
    b = dbeta.double() * inv
    cc = rstd.double() * dgamma.double() * inv
    gd = g.double()
    dx = a * (gd - b - xc * cc)
    return dx, H16 * dx.abs() + 8 * U32 * a.abs() * (gd.abs() + b.abs() + xc.abs() * cc.abs()) + Z16


def truth_f64(x, resid, dy, gamma, beta, mask, depth, eps=EPS):
    """F.batch_norm(training=True) (+ resid) (+ ReLU) and its autograd in float64 -> {name: (value, bound)} of y and dx:
    the elementwise bound evaluated at the truth plus the propagated statistics and sum bounds.  mask: the kernel's
    y > 0 (bool) under ReLU, else None."""
    m = x.shape[0]
    xd = x.double().requires_grad_(True)
    w, b = gamma.double(), beta.double()
    with torch.backends.cudnn.flags(enabled=False):
        pre = F.batch_norm(xd, None, None, w, b, True, 0.0, eps)
    if resid is not None:
        pre = pre + resid.double()
    out = pre * mask if mask is not None else pre
    out.backward(dy.double())
    y = (pre.detach().clamp_min(0.0) if mask is not None else pre.detach())
    dx = xd.grad
    mean, var = stats_f64(x)
    rstd = rstd_f64(var, eps)
    b_mean, b_var = stat_bounds(mean, var)
    b_rstd = rstd_bound(var, b_var, eps)
    xc = x.double() - mean
    _, y_bound, _ = fwd_f64(x, mean, rstd, gamma, beta, resid, mask is not None)
    y_bound = y_bound + SECOND * (w.abs() * rstd * b_mean + xc.abs() * w.abs() * b_rstd)
    g = dy.double() * mask if mask is not None else dy.double()
    dbeta, b_dbeta, dgamma, b_dgamma, s2 = sums_f64(g, x, mean, rstd, depth)
    b_dgamma = b_dgamma + b_rstd * s2.abs() + rstd * b_mean * dbeta.abs()
    _, dx_bound = dx_f64(g, x, mean, rstd, gamma, dgamma, dbeta, m)
    a, cc = w * rstd, rstd * dgamma / m
    inner = g - dbeta / m - xc * cc
    d_cc = (b_rstd * dgamma.abs() + rstd * b_dgamma) / m
    dx_bound = dx_bound + SECOND * (w.abs() * b_rstd * inner.abs() +
                                    a.abs() * (b_dbeta / m + b_mean * cc.abs() + xc.abs() * d_cc))
    return {"y": (y, y_bound), "dx": (dx, dx_bound)}


# ---------------------------------------------------------------------------------------------------------------
# the kernels' reduction order in fp32 (CPU): x [M, n] holds any n channels, the order is the same for each
# ---------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _lanes(v, m, p):
    """[M, n] -> [chunks, passes, rpp, n], rows past M zero"""
    pad = p.chunks * p.rows_per_chunk - m
    v = torch.cat([v, v.new_zeros(pad, v.shape[1])])
    return v.view(p.chunks, p.chunk_passes, p.rpp, v.shape[1])


def _per_lane(v, p):
    """[chunks, ...] -> [64, per, ...]: finalize lane l holds chunks [l per, (l + 1) per), zeros past the last"""
    pad = 64 * p.per - v.shape[0]
    v = torch.cat([v, v.new_zeros((pad,) + tuple(v.shape[1:]))])
    return v.view((64, p.per) + tuple(v.shape[1:]))


def chan_merge(na, ma, Ma, nb, mb, Mb):
    n = na + nb
    d = mb - ma
    f = nb / n.clamp_min(1.0)
    m2 = ma + d * f
    M2 = Ma + (Mb + d * d * na * f)
    skip, take = nb == 0, na == 0
    pick = lambda a, b, c: torch.where(skip, a, torch.where(take, b, c))
    return pick(na, nb, n), pick(ma, mb, m2), pick(Ma, Mb, M2)


def emulate_stats(x, p, eps=EPS, shift=True, last_count=None):
    """-> fp32 (mean, var = M2 / M, rstd) as bn2d_stats_kernel and bn2d_stats_finalize_kernel order them.
    shift=False: k = 0, the lane's variance from sum x^2 - (sum x)^2 / n (a mistake); last_count: the count the
    finalize gives the last chunk (a mistake when it is not its rows)."""
    m, n = x.shape
    xp = _lanes(x.float(), m, p)
    rows = torch.arange(p.chunks * p.rows_per_chunk).view(p.chunks, p.chunk_passes, p.rpp)
    valid = (rows < m)[..., None]
    k = xp[:, 0] if shift else torch.zeros_like(xp[:, 0])
    s, q = torch.zeros_like(k), torch.zeros_like(k)
    for i in range(1 if shift else 0, p.chunk_passes):
        d = xp[:, i] - k
        s = torch.where(valid[:, i], s + d, s)
        q = torch.where(valid[:, i], _fma(d, d, q), q)
    nt = valid.sum(1).float()                                    # [chunks, rpp, 1]
    inv = torch.where(nt > 0, 1.0 / nt.clamp_min(1.0), torch.zeros_like(nt))
    ds = s * inv
    lane_mean, lane_m2 = k + ds, (q - s * ds).clamp_min(0.0)
    z = torch.zeros(p.chunks, n)
    na, ma, Ma = torch.zeros(p.chunks, 1), z, z.clone()
    for g in range(p.rpp):
        na, ma, Ma = chan_merge(na, ma, Ma, nt[:, g], lane_mean[:, g], lane_m2[:, g])
    count = torch.full((p.chunks, 1), float(p.rows_per_chunk))
    count[-1] = float(p.last_rows if last_count is None else last_count)
    cn, cm, cM = _per_lane(count, p), _per_lane(ma, p), _per_lane(Ma, p)
    na, ma, Ma = torch.zeros(64, 1), torch.zeros(64, n), torch.zeros(64, n)
    for j in range(p.per):
        na, ma, Ma = chan_merge(na, ma, Ma, cn[:, j], cm[:, j], cM[:, j])
    while na.shape[0] > 1:            # lane l (a multiple of 2 o) merges lane l + o: the lanes still live, pairwise
        na, ma, Ma = chan_merge(na[0::2], ma[0::2], Ma[0::2], na[1::2], ma[1::2], Ma[1::2])
    mean, var = ma[0], Ma[0] / torch.tensor(float(m))
    return mean, var, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))


def emulate_sums(g, x, mean, rstd, p):
    """-> fp32 (dbeta, dgamma) as bn2d_bwd_reduce_kernel and bn2d_bwd_finalize_kernel order them; g the masked dy"""
    m, n = x.shape
    gp, xc = _lanes(g.float(), m, p), _lanes(x.float() - mean.float(), m, p)      # pad rows: g = 0
    s1, s2 = torch.zeros_like(gp[:, 0]), torch.zeros_like(gp[:, 0])
    for i in range(p.chunk_passes):
        s1 = s1 + gp[:, i]
        s2 = _fma(gp[:, i], xc[:, i], s2)
    out = []
    for part in (s1, s2):
        a = part[:, 0]
        for r in range(1, p.rpp):
            a = a + part[:, r]
        v = _per_lane(a, p)
        s = torch.zeros(64, n)
        for j in range(p.per):
            s = s + v[:, j]
        while s.shape[0] > 1:
            s = s[0::2] + s[1::2]
        out.append(s[0])
    return out[0], out[1] * rstd.float()


# ---------------------------------------------------------------------------------------------------------------
# the whole chain in float64, with a kernel mistake on request
# ---------------------------------------------------------------------------------------------------------------
MISTAKES = ("one row of a ragged last pass left out of the sums but counted",
            "the last chunk's rows counted as rows_per_chunk",
            "the second apply trip not written",
            "the variance as sum x^2 - (sum x)^2 / n",
            "the biased variance in running_var",
            "the ReLU mask taken from x instead of y",
            "dgamma without the rstd factor",
            "1 / M taken over the chunk instead of the map")
LOST, COUNT, TRIP, NAIVE, BIASED, MASKX, NORSTD, INVM = MISTAKES


def chain_f64(prob, p, relu, resid, mistake=None, given=None):
    """prob: make_problem's tensors (any subset of channels) -> {name: float64 tensor} of every output of the forward
    and the backward, each step from the float64 result of the step before.  given = (mean, rstd): skip the
    statistics (the exact-sum checks).  An unwritten element is NaN."""
    x, dy = prob["x"], prob["dy"]
    m = x.shape[0]
    xd = x.double()
    keep = torch.ones(m, dtype=torch.bool)
    if mistake == LOST:
        keep[m - 1] = False
    out = {}
    if given is None:
        if mistake == NAIVE:
            mean, var, _ = (t.double() for t in emulate_stats(x, p, shift=False))
        elif mistake == COUNT:
            xp = _lanes(xd, m, p).flatten(1, 2)                              # [chunks, rows_per_chunk, n]
            cnt = torch.full((p.chunks, 1), float(p.rows_per_chunk), dtype=torch.float64)
            true = cnt.clone()
            true[-1] = p.last_rows
            cmean = xp.sum(1) / true
            inside = (torch.arange(p.rows_per_chunk)[None, :, None] < true[:, :, None])
            cm2 = (((xp - cmean[:, None]) ** 2) * inside).sum(1)
            mean = (cnt * cmean).sum(0) / cnt.sum()
            var = (cm2.sum(0) + (cnt * (cmean - mean) ** 2).sum(0)) / m
        else:
            mean = xd[keep].sum(0) / m
            var = ((xd[keep] - mean) ** 2).sum(0) / m
        rstd = rstd_f64(var)
        out["save_mean"], out["save_rstd"] = mean, rstd
        out["running_mean"], out["running_var"] = running_f64(prob["rm"], prob["rv"], mean, var, m,
                                                              unbiased=mistake != BIASED)
        r = prob["resid"] if resid else None
        out["y"] = fwd_f64(x, mean, rstd, prob["gamma"], prob["beta"], r, relu)[0]
        mask_src = out["y"]
    else:
        mean, rstd = (t.double() for t in given)
        mask_src = prob.get("y")
        relu = mask_src is not None
    gamma = prob["gamma"].double()
    g = dy.double()
    if relu:
        g = g * ((xd if mistake == MASKX else mask_src.double()) > 0)
    out["dresid"] = g.clone()
    gk = g * keep[:, None]
    out["dbeta"] = gk.sum(0)
    s2 = (gk * (xd - mean)).sum(0)
    out["dgamma"] = s2 if mistake == NORSTD else rstd * s2
    out["dx"] = dx_f64(g, x, mean, rstd, gamma, out["dgamma"], out["dbeta"], m,
                       1.0 / p.rows_per_chunk if mistake == INVM else None)[0]
    if mistake == TRIP:
        lo = p.apply_blocks * p.rpp
        for name in ("y", "dx", "dresid"):
            if name in out:
                out[name][lo:min(2 * lo, m)] = NAN
    return out


def _holds(cond):
    return 0.0 if bool(cond) else float("inf")


def _same_bits(a, b):
    """bit for bit where both are fp16 (-0 is not +0); a float64 chain is compared by value"""
    if a.dtype == b.dtype == torch.float16:
        return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
    return torch.equal(a.double(), b.double())


def check_outputs(prob, p, relu, resid, out, truth=True):
    """The checks of tests/test_bn2d_elements_gpu.py on one forward + backward: out = {name: tensor} as the kernels
    (or chain_f64) give them -> {check: err / bound}, a broken equality being an infinite error.  Statistics against
    float64 of the input; y, dbeta, dgamma, dx each from the vectors in `out` that the kernel computed them from;
    dresid bit for bit; y and dx against the float64 autograd as well."""
    x, dy, gamma, beta = prob["x"], prob["dy"], prob["gamma"], prob["beta"]
    m = x.shape[0]
    mean, var = stats_f64(x)
    b_mean, b_var = stat_bounds(mean, var)
    rm, rv = running_f64(prob["rm"], prob["rv"], mean, var, m)
    b_rm, b_rv = running_bounds(prob["rm"], prob["rv"], mean, var, b_mean, b_var, m)
    w = {"save_mean": ratio(out["save_mean"], mean, b_mean),
         "save_rstd": ratio(out["save_rstd"], rstd_f64(var), rstd_bound(var, b_var)),
         "running_mean": ratio(out["running_mean"], rm, b_rm), "running_var": ratio(out["running_var"], rv, b_rv)}
    k_mean, k_rstd = out["save_mean"], out["save_rstd"]
    r = prob["resid"] if resid else None
    y64, b_y, zero = fwd_f64(x, k_mean, k_rstd, gamma, beta, r, relu)
    w["y"] = ratio(out["y"], y64, b_y)
    if relu:
        w["y >= 0"] = _holds((out["y"] >= 0).all())
        w["y == 0 where y64 <= -bound"] = _holds((out["y"][zero] == 0).all())
    g = masked(dy, out["y"] if relu else None)
    if out.get("dresid") is not None:
        w["dresid"] = _holds(_same_bits(out["dresid"], g))
    dbeta, b_dbeta, dgamma, b_dgamma, _ = sums_f64(g, x, k_mean, k_rstd, p.depth)
    w["dbeta"], w["dgamma"] = ratio(out["dbeta"], dbeta, b_dbeta), ratio(out["dgamma"], dgamma, b_dgamma)
    w["dx"] = ratio(out["dx"], *dx_f64(g, x, k_mean, k_rstd, gamma, out["dgamma"], out["dbeta"], m))
    if truth:
        t = truth_f64(x, r, dy, gamma, beta, (out["y"] > 0) if relu else None, p.depth)
        w["y / autograd"], w["dx / autograd"] = ratio(out["y"], *t["y"]), ratio(out["dx"], *t["dx"])
    return w
