"""Shared by tests/test_optim_host.py, tests/test_optim_gpu.py and tests/test_train_fused_optim_gpu.py: the optimizer
tail (unscale, non-finite test, global norm, clip coefficient, coupled-L2 Adam with bias correction, GradScaler.update)
  1. restated in float64 on given fp32 inputs (`tail64`),
  2. with a per-element bound for p', m', v' and a bound for total_norm (`bounds`), each a sum of named terms, one per
     rounding point of csrc/optim.hip,
  3. and emulated in numpy fp32 in the kernels' exact operation order (`emulate`), optionally with one of MISTAKES.
Test infrastructure, like tests/_stem_ref.py: no test lives here.

A problem is a list of tensors, each a dict(p, g, m, v: fp32 numpy arrays of one length, g None = no gradient;
step: int; wd, lr: float; g_aligned: whether the gradient's address is a multiple of 16 bytes - the norm kernel's
summation order depends on it) and a Cfg.

The bound.  u = 2^-24 (fp32 round to nearest).  fp contraction is off in the kernels, so every product, sum, quotient
and square root is one rounding of relative size u.  Written X^ for the kernel's value of X:

  total_norm   the kernel's sum of squares S^ has only non-negative terms, so every rounding is relative to (at most)
               S: N_UNSCALE (inv_scale to fp32, g * inv_scale: 2 roundings, doubled by the square) + N_SQUARE +
               N_LANE (per-lane sequential additions: at most CHUNK / 256 on the 4-byte path; the 16-byte path has
               CHUNK / 1024 + 2 + 1, fewer) + N_WAVE (6 butterfly levels) + N_BLOCK (3 additions across the 4 waves)
               + the fp64 finalize (below 2^-40, counted as N_F64); the square root halves the relative error and
               the result is rounded to fp32 once more (N_OUT).
  c            c^ = fp32(inv_scale * clip) is formed in double from the double norm: the norm's relative error where
               the clip can be active, + 1 rounding.
  g            |grad c| (e_c + u)  +  |wd p| (u [wd to fp32] + u [product])  +  (|grad c| + |wd p|) u [sum]
  m'           (1-b1) E_g  +  (1-b1) |g - m| (u [difference] + u [1-b1 to fp32] + u [product])  +  |m'| u [sum]
  v'           (1-b2) (2 |g| E_g + E_g^2)  +  (1-b2) g^2 (u [square] + u [1-b2 to fp32] + u [product])
               +  b2 v (u [b2 to fp32] + u [product])  +  |v'| u [sum]
  p'           r = sqrt(v'): E_r = min(E_v / sqrt(v'), sqrt(E_v)) + r u [sqrt];
               den = r / bc2 + eps: E_den = (E_r + r (u [bc2 to fp32] + u [quotient])) / bc2 + eps u [eps to fp32]
                                            + den u [sum]
               q = m' / den: E_q = E_m / (den - E_den) + |m'| E_den / (den (den - E_den)) + |q| u [quotient]
               t = ss q:     E_t = ss (E_q + |q| (u [step_size to fp32] + u [product]));      E_p = E_t + |p'| u [sum]
Every bound is multiplied by SECOND_ORDER (products of two of the terms above) and gets UNDERFLOW added (an fp32
operation whose result is subnormal is off by up to 2^-150, not by a relative u).
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
UNDERFLOW = 16 * 2.0 ** -149
N_UNSCALE, N_SQUARE, N_WAVE, N_BLOCK, N_F64, N_OUT = 4, 1, 6, 3, 2.0 ** -16, 1

MISTAKES = ("decoupled_wd", "wd_on_no_decay_group", "no_bias_correction", "step_off_by_one", "eps_inside_sqrt",
            "clip_not_clamped", "no_unscale", "v_from_unclipped_grad", "state_updated_on_found_inf")


@dataclass
class Cfg:
    scale: Optional[float] = 65536.0      # None: no scaler (inv_scale = 1, found_inf forced false)
    tracker: int = 0
    growth_factor: float = 2.0
    backoff_factor: float = 0.5
    growth_interval: int = 2000
    max_norm: Optional[float] = 1.0       # None: no clip
    use_norm: bool = True                 # False: the plain step (no norm pass at all)
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    chunk: int = 16384                    # hcir.optim._CHUNK


# tail64, bounds and worst_ratio take numpy arrays or torch tensors (float64 on a device is how the train-step test
# affords eleven million elements): the few array functions they need, for both
def _is_np(a):
    return isinstance(a, np.ndarray)


def _f64(a):
    return a.astype(np.float64) if _is_np(a) else a.double()


def _sqrt(a):
    return np.sqrt(a) if _is_np(a) else a.sqrt()


def _minimum(a, b):
    return np.minimum(a, b) if _is_np(a) else torch_mod().minimum(a, b)


def _where(c, a, b):
    if _is_np(c):
        return np.where(c, a, b)
    t = torch_mod()
    return t.where(c, a if t.is_tensor(a) else t.full_like(b, a), b if t.is_tensor(b) else t.full_like(a, b))


def _all_finite(a):
    return bool(np.isfinite(a).all()) if _is_np(a) else bool(torch_mod().isfinite(a).all())


def torch_mod():
    import torch
    return torch


def _scaler_update(found, scale, tracker, cfg):
    """torch.amp.GradScaler.update in fp32 (exact in the tests: factors are powers of two)."""
    if scale is None:
        return None, tracker
    s = np.float32(scale)
    if found:
        return float(s * np.float32(cfg.backoff_factor)), 0
    ok = tracker + 1
    if ok == cfg.growth_interval:
        grown = s * np.float32(cfg.growth_factor)
        return float(grown if np.isfinite(grown) else s), 0
    return float(s), ok


def tail64(ts, cfg):
    """The tail in float64.  Returns dict(norm, found_inf, coef, c, scale, tracker, out=[dict(p, m, v, step, g) or
    None for a tensor without gradient])."""
    inv = 1.0 / float(np.float32(cfg.scale)) if cfg.scale is not None else 1.0
    live = [t for t in ts if t["g"] is not None]
    with np.errstate(all="ignore"):
        found = cfg.scale is not None and any(not _all_finite(_f64(t["g"]) * inv) for t in live)
        if cfg.use_norm:
            norm = float(np.sqrt(np.float64(sum(float(((_f64(t["g"]) * inv) ** 2).sum()) for t in live))))
        else:
            norm = 0.0
        coef_raw = cfg.max_norm / (norm + 1e-6) if (cfg.use_norm and cfg.max_norm is not None) else 1.0
    coef = min(1.0, coef_raw) if not math.isnan(coef_raw) else coef_raw
    c = inv * coef
    scale, tracker = _scaler_update(found, cfg.scale, cfg.tracker, cfg)
    out = []
    for t in ts:
        if t["g"] is None:
            out.append(None)
            continue
        p, m, v = (_f64(t[k]) for k in ("p", "m", "v"))
        if found:
            out.append(dict(p=p, m=m, v=v, step=t["step"], g=None))
            continue
        step = t["step"] + 1
        with np.errstate(all="ignore"):
            g = _f64(t["g"]) * c + t["wd"] * p
            m2 = m + (g - m) * (1.0 - cfg.beta1)
            v2 = v * cfg.beta2 + (1.0 - cfg.beta2) * g * g
            ss = t["lr"] / (1.0 - cfg.beta1 ** step)
            bc2 = math.sqrt(1.0 - cfg.beta2 ** step)
            den = _sqrt(v2) / bc2 + cfg.eps
            p2 = p - ss * (m2 / den)
        out.append(dict(p=p2, m=m2, v=v2, step=step, g=g, ss=ss, bc2=bc2, den=den, m_in=m, v_in=v, p_in=p))
    return dict(norm=norm, found_inf=bool(found), coef=coef, coef_raw=coef_raw, c=c, inv=inv, scale=scale,
                tracker=tracker, out=out)


def norm_rel_bound(cfg):
    """Relative bound of total_norm (see the module docstring)."""
    n_lane = cfg.chunk // 256
    sum_rel = (N_UNSCALE + N_SQUARE + n_lane + N_WAVE + N_BLOCK + N_F64) * U
    return (0.5 * sum_rel + N_OUT * U) * SECOND_ORDER


def bounds(ts, r, cfg):
    """dict(norm=bound of total_norm, out=[dict(p, m, v) of per-element bounds or None]) for the result r of tail64."""
    e_n = norm_rel_bound(cfg) if cfg.use_norm else 0.0
    res = dict(norm=e_n * r["norm"] + UNDERFLOW, out=[])
    clipping = cfg.use_norm and cfg.max_norm is not None
    # the clip is exactly 1 in the kernel too when the exact ratio stays above 1 under the norm's own error
    e_clip = e_n if (clipping and r["coef_raw"] * (1.0 - 2.0 * e_n) < 1.0) else 0.0
    e_c = e_clip + (U if (cfg.scale is not None or clipping) else 0.0)
    b1, b2 = cfg.beta1, cfg.beta2
    for t, o in zip(ts, r["out"]):
        if o is None:
            res["out"].append(None)
            continue
        if r["found_inf"]:
            z = o["p"] * 0.0
            res["out"].append(dict(p=z, m=z, v=z))
            continue
        a = abs(_f64(t["g"]) * r["c"])
        b = abs(t["wd"] * o["p_in"])
        g = o["g"]
        e_g = a * (e_c + U) + b * (U + U) + (a + b) * U
        d = abs(g - o["m_in"]) + e_g
        e_m = (1 - b1) * e_g + (1 - b1) * d * (U + U + U) + abs(o["m"]) * U
        e_v = ((1 - b2) * (2 * abs(g) * e_g + e_g * e_g) + (1 - b2) * g * g * (U + U + U)
               + b2 * o["v_in"] * (U + U) + abs(o["v"]) * U)
        e_m, e_v = e_m * SECOND_ORDER + UNDERFLOW, e_v * SECOND_ORDER + UNDERFLOW
        rt = _sqrt(o["v"])
        with np.errstate(divide="ignore", invalid="ignore"):
            e_r = _minimum(_where(rt > 0, e_v / rt, math.inf), _sqrt(e_v)) + rt * U
        den = o["den"]
        e_den = (e_r + rt * (U + U)) / o["bc2"] + cfg.eps * U + den * U
        den_lo = den - e_den
        assert (den_lo > 0).all()
        q = o["m"] / den
        e_q = e_m / den_lo + abs(o["m"]) * e_den / (den * den_lo) + abs(q) * U
        e_t = o["ss"] * (e_q + abs(q) * (U + U))
        e_p = (e_t + abs(o["p"]) * U) * SECOND_ORDER + UNDERFLOW
        res["out"].append(dict(p=e_p, m=e_m, v=e_v))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# numpy fp32 emulation of csrc/optim.hip, operation by operation
F = np.float32


def _chunk_sumsq(g, inv, vec):
    """grad_sumsq_kernel on one chunk: (fp32 partial, flag)."""
    with np.errstate(all="ignore"):
        u = g * inv
        sq = u * u
        bad = not np.isfinite(u).all()
        n = len(g)
        n4 = n // 4 if vec else 0
        lanes = np.zeros(256, F)
        if n4:
            it = -(-n4 // 256)
            body = np.zeros((it * 256, 4), F)
            body[:n4] = sq[:n4 * 4].reshape(n4, 4)
            body = body.reshape(it, 256, 4)
            acc = np.zeros((256, 4), F)
            for j in range(it):
                acc = acc + body[j]
            lanes = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
        tail = sq[n4 * 4:]
        if len(tail):
            it = -(-len(tail) // 256)
            tl = np.zeros(it * 256, F)
            tl[:len(tail)] = tail
            for row in tl.reshape(it, 256):
                lanes = lanes + row
        w = lanes.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w[:, :o] + w[:, o:2 * o]
        w = w[:, 0]
        return ((w[0] + w[1]) + w[2]) + w[3], bad


def _finalize_sum(partials):
    """optim_finalize_kernel's fp64 sum: lane t adds partials t, t + 256, ... ascending, then a halving tree."""
    with np.errstate(all="ignore"):
        n = len(partials)
        it = max(1, -(-n // 256))
        pad = np.zeros(it * 256, np.float64)
        pad[:n] = np.asarray(partials, np.float64)
        red = np.zeros(256, np.float64)
        for row in pad.reshape(it, 256):
            red = red + row
        o = 128
        while o:
            red = red[:o] + red[o:2 * o]
            o //= 2
        return float(red[0])


def emulate(ts, cfg, mistake=None):
    """The three kernels in numpy fp32.  Returns what tail64 returns (norm as the fp32 the caller gets back)."""
    assert mistake is None or mistake in MISTAKES
    has_scaler = cfg.scale is not None
    scale32 = F(cfg.scale) if has_scaler else None
    unscale = has_scaler and mistake != "no_unscale"
    inv32 = F(1.0 / np.float64(scale32)) if unscale else F(1.0)
    inv64 = 1.0 / float(scale32) if unscale else 1.0
    live = [t for t in ts if t["g"] is not None]
    partials, bad = [], False
    if cfg.use_norm:
        for t in live:
            for off in range(0, len(t["g"]), cfg.chunk):
                s, b = _chunk_sumsq(t["g"][off:off + cfg.chunk], inv32, t.get("g_aligned", True))
                partials.append(s)
                bad |= b
    found = bool(has_scaler and bad)
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64(_finalize_sum(partials))))
        coef = 1.0
        if cfg.use_norm and cfg.max_norm is not None:
            coef = cfg.max_norm / (norm + 1e-6)
            if coef > 1.0 and mistake != "clip_not_clamped":
                coef = 1.0
        c32 = F(inv64 * coef)
        c_unclipped = F(inv64)
    scale, tracker = _scaler_update(found, cfg.scale, cfg.tracker, cfg)
    skip = found and mistake != "state_updated_on_found_inf"
    b2f, om1, om2, epsf = F(cfg.beta2), F(1.0 - cfg.beta1), F(1.0 - cfg.beta2), F(cfg.eps)
    wd_max = max(t["wd"] for t in ts)
    out = []
    for t in ts:
        if t["g"] is None:
            out.append(None)
            continue
        p, m, v = t["p"].copy(), t["m"].copy(), t["v"].copy()
        if skip:
            out.append(dict(p=p, m=m, v=v, step=t["step"]))
            continue
        step = t["step"] + 1
        k = step + 1 if mistake == "step_off_by_one" else step
        ss = F(t["lr"] / (1.0 - cfg.beta1 ** k))
        bc2 = F(math.sqrt(1.0 - cfg.beta2 ** k))
        if mistake == "no_bias_correction":
            ss, bc2 = F(t["lr"]), F(1.0)
        wd = F(wd_max if mistake == "wd_on_no_decay_group" else t["wd"])
        with np.errstate(all="ignore"):
            if mistake == "decoupled_wd":
                p = p * F(1.0 - t["lr"] * t["wd"])
                g = t["g"] * c32
            else:
                g = t["g"] * c32 + wd * p
            m = m + (g - m) * om1
            gv = t["g"] * c_unclipped + wd * p if mistake == "v_from_unclipped_grad" else g
            v = v * b2f + om2 * (gv * gv)
            if mistake == "eps_inside_sqrt":
                denom = np.sqrt(v + epsf) / bc2
            else:
                denom = np.sqrt(v) / bc2 + epsf
            p = p - ss * (m / denom)
        out.append(dict(p=p, m=m, v=v, step=step))
    return dict(norm=float(F(norm)), found_inf=found, coef=float(F(coef)), c=float(c32), scale=scale, tracker=tracker,
                out=out)


# ---------------------------------------------------------------------------------------------------------------------
# input families
SIZES_HOST = (1, 3, 5, 1023, 1024 + 7)


def make_tensors(sizes, seed, g_std, p_std=0.05, preload_step=0, wds=(1e-4, 0.0), lr=1e-3, none_at=None,
                 misaligned_at=None):
    """Two groups (tensor i is in group i % 2), p ~ N(0, p_std), g ~ N(0, g_std) already multiplied by the loss scale
    by the caller's choice of g_std; preload_step > 0 preloads m ~ N(0, 0.01) and v = squares of N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    ts = []
    for i, n in enumerate(sizes):
        t = dict(p=(p_std * rng.standard_normal(n)).astype(F), g=(g_std * rng.standard_normal(n)).astype(F),
                 m=np.zeros(n, F), v=np.zeros(n, F), step=preload_step, wd=wds[i % 2], lr=lr, g_aligned=True)
        if preload_step:
            t["m"] = (0.01 * rng.standard_normal(n)).astype(F)
            t["v"] = ((0.01 * rng.standard_normal(n)) ** 2).astype(F)
        if i == none_at:
            t["g"] = None
        if i == misaligned_at:
            t["g_aligned"] = False
        ts.append(t)
    return ts


def families(sizes, none_at=None, misaligned_at=None):
    """name -> (tensors, Cfg).  With n = sum(sizes) elements the unscaled norm is about g_std / scale * sqrt(n)."""
    kw = dict(none_at=none_at, misaligned_at=misaligned_at)
    n = float(sum(sizes))
    fam = {
        # unscaled gradients N(0, 1): norm = sqrt(n) (>> 1 whenever n >> 1; the GPU sizes give ~ 630): clip active
        "unit_clip_active": (make_tensors(sizes, 1, 65536.0, **kw), Cfg()),
        # |g * inv_scale| ~ 1e-12 << eps = 1e-8, norm << 1: clip inactive
        "tiny_below_eps": (make_tensors(sizes, 2, 65536.0 * 1e-12, **kw), Cfg()),
        # unscaled norm 0.1: clip inactive, coefficient exactly 1
        "small_norm_clip_inactive": (make_tensors(sizes, 3, 65536.0 * 0.1 / math.sqrt(n), **kw), Cfg()),
        # bias correction far from step 1
        "preloaded_step_999": (make_tensors(sizes, 4, 65536.0, preload_step=999, **kw), Cfg()),
    }
    return fam


def with_non_finite(ts):
    """An inf in the first gradient that has one and a NaN in the last."""
    live = [t for t in ts if t["g"] is not None and len(t["g"])]
    live[0]["g"] = live[0]["g"].copy()
    live[-1]["g"] = live[-1]["g"].copy()
    live[0]["g"][len(live[0]["g"]) // 2] = np.inf
    live[-1]["g"][-1] = np.nan
    return ts


def worst_ratio(got, want, bound):
    """max over elements of |got - want| / bound (0 for an empty tensor; inf where got is not finite or the bound is
    0 and the error is not)."""
    if (got.size if _is_np(got) else got.numel()) == 0:
        return 0.0
    err = abs(_f64(got) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = _where(err == 0, 0.0, err / bound)
    ratio = _where(_f64(got) - _f64(got) == 0, ratio, math.inf)        # inf or NaN in got: x - x is NaN
    return float(ratio.max())
