"""SupConLoss restatement, error bounds, kernel emulation and mutations (TEST INFRASTRUCTURE ONLY), in the manner of
oracle/ntxent.py.

The loss is the supervised contrastive loss of HairPretraining/utils/losses.py:8-101 (contrast_mode 'all'), restated
in our own words in float64; tests/golden/supcon_ref.npz (tests/golden/make_supcon_golden.py) pins the restatement to
the reference class.

  features [B, V, D];  row r = v*B + i (view v of sample i), N = V*B;  y_r = labels[r mod B] (None: r mod B)
  x_r = row, or row / max(||row||, 1e-12) with normalize;  s_ij = x_i.x_j / T;  lse_i = log sum_{j != i} exp(s_ij)
  m_ij = [y_i == y_j, j != i], n_i = sum_j m_ij, a_i = [n_i > 0], P_i = sum_j m_ij s_ij
  loss = mean_i (T / T_base) a_i (lse_i - P_i / max(n_i, 1))
  p_ij = exp(s_ij - lse_i) (diagonal 0), G = a (p - m / n), W = G + G^T, g = W x, dL/dx_i = grad_out / (T_base N) g_i,
  with normalize through rn_i (g_i - (g_i.u_i) u_i).
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import torch

from oracle.ntxent import U_ROUND, err_over_bound, make_inputs  # noqa: F401  (re-exported for the tests)

_LOG2E = 1.44269504088896340736
_LN2 = 0.69314718055994530942

# (B, V, D, T, T_base): around the 128-row tile edge (N = 2, 8, 74, 128, 136, 202, 264, 258, 144, 136, 200), D below
# one K stage, D on the LDS-DMA path (64, 128 elements per stage) and off it, V = 1, 2, 3, T != T_base, negative T
CASES = [(1, 2, 8, .5, .07), (4, 2, 8, .07, .07), (37, 2, 32, .5, .07), (64, 2, 64, .07, .07), (68, 2, 72, .2, .1),
         (101, 2, 40, .1, .07), (132, 2, 8, .2, .07), (129, 2, 136, .5, .5), (48, 3, 96, .07, .07),
         (136, 1, 64, .3, .07), (100, 2, 72, -.5, .07)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MAIN_FAMILIES = ("exact", "norms", "exact_norms")
LABEL_FAMILIES = ("none", "three", "one", "mixed", "wide")


def case_dtypes(case):
    """Negative temperature: fp32 and fp16 only (as oracle.ntxent.case_dtypes)."""
    return DTYPES[:2] if case[3] < 0 else DTYPES


def has_backward(case):
    return (case[0] * case[1]) % 8 == 0


def u_in_of(family, dtype, normalize):
    """Rounding of the rows the MFMA reads, relative to the float64 reference on the rounded inputs: without
    normalize the kernel copies the inputs (none); with it the normalised rows are rounded to the compute dtype,
    except where they are exact in every dtype."""
    if not normalize:
        return 0.0
    return 2.0 ** -24 if family in ("exact", "exact_norms") else U_ROUND[dtype]


def make_features(family: str, b: int, v: int, d: int) -> torch.Tensor:
    """fp32 CPU [B, V, D]: views 0 and 1 are oracle.ntxent.make_inputs(family, b, d), view 2 its z0 at seed 1."""
    z0, z1 = make_inputs(family, b, d)
    views = [z0, z1, make_inputs(family, b, d, seed=1)[0]][:v]
    return torch.stack(views, 1).contiguous()


def make_labels(family: str, b: int) -> Optional[torch.Tensor]:
    """int64 [B] or None.  three: three classes at random;  one: all one class;  mixed: singletons and pairs of
    samples (at V = 1 the singleton rows have no positive);  wide: classes {5, 5 + 2^32, -1}: equal in their low 32
    bits (the first two) and negative."""
    g = torch.Generator().manual_seed(7919 * b + len(family))
    if family == "none":
        return None
    if family == "three":
        return torch.randint(0, 3, (b,), generator=g)
    if family == "one":
        return torch.full((b,), 4, dtype=torch.int64)
    if family == "mixed":   # classes 0 0 1 2 2 3 4 4 5 ... in a random order
        cls = torch.tensor([(2 * (i // 3)) + (1 if i % 3 == 2 else 0) for i in range(b)], dtype=torch.int64)
        return cls[torch.randperm(b, generator=g)]
    if family == "wide":
        vals = torch.tensor([5, 5 + 2 ** 32, -1], dtype=torch.int64)
        return vals[torch.arange(b) % 3][torch.randperm(b, generator=g)]
    raise ValueError(family)


def rows_of(t: torch.Tensor) -> torch.Tensor:
    """[B, V, D] -> [N, D] in the kernels' row order (cat(unbind(t, 1)))."""
    return torch.cat(torch.unbind(t, 1), 0)


def row_labels(labels, b: int, v: int) -> torch.Tensor:
    return (torch.arange(b) if labels is None else labels.reshape(-1).to(torch.int64)).repeat(v)


def positive_mask(y: torch.Tensor) -> torch.Tensor:
    m = y[:, None] == y[None, :]
    m.fill_diagonal_(False)
    return m


class ScRef(NamedTuple):
    """float64 ground truth of one problem."""
    loss: torch.Tensor      # scalar
    row_loss: torch.Tensor  # [N]
    lse: torch.Tensor       # [N]
    npos: torch.Tensor      # [N] int64
    P: torch.Tensor         # [N] sum of the positive logits
    p: torch.Tensor         # [N, N] softmax of the masked logits, diagonal 0
    W: torch.Tensor         # [N, N] G + G^T
    sim: torch.Tensor       # [N, N] logits, diagonal included
    x: torch.Tensor         # [N, D] the rows the logits are taken of (normalised with normalize)
    m: torch.Tensor         # [N, N] bool positives


def _loss_from(sim, m, t, t_base):
    n = sim.shape[0]
    eye = torch.eye(n, dtype=torch.bool)
    lse = torch.logsumexp(sim.masked_fill(eye, float("-inf")), dim=1)
    npos = m.sum(1)
    P = (sim * m).sum(1)
    row_loss = (t / t_base) * (npos > 0).double() * (lse - P / npos.clamp_min(1))
    return row_loss.mean(), row_loss, lse, npos, P


def _rows_x(features, normalize):
    x = rows_of(features.double())
    if normalize:
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return x


def supcon_f64(features, labels, t, t_base, normalize, full: bool = False):
    """float64 loss (full: an ScRef) of [B, V, D] features."""
    b, v, _ = features.shape
    x = _rows_x(features, normalize)
    sim = x @ x.t() / t
    m = positive_mask(row_labels(labels, b, v))
    loss, row_loss, lse, npos, P = _loss_from(sim, m, t, t_base)
    if not full:
        return loss
    eye = torch.eye(b * v, dtype=torch.bool)
    p = torch.exp(sim - lse[:, None]).masked_fill(eye, 0.0)
    G = (npos > 0).double()[:, None] * (p - m.double() / npos.clamp_min(1)[:, None])
    return ScRef(loss, row_loss, lse, npos, P, p, G + G.t(), sim, x, m)


def supcon_grad_f64(features, labels, t, t_base, normalize, grad_out: float = 1.0):
    """d(loss * grad_out)/d features, [B, V, D], by float64 autograd."""
    f = features.detach().double().requires_grad_(True)
    (supcon_f64(f, labels, t, t_base, normalize) * grad_out).backward()
    return f.grad


def closed_form_grad(ref: ScRef, features, t_base, normalize, grad_out: float = 1.0, W=None):
    """The backward the kernels implement, in float64 and row order [N, D]: g = W x, scale, projection."""
    W = ref.W if W is None else W
    n = W.shape[0]
    g = W @ ref.x
    c = grad_out / (t_base * n)
    if not normalize:
        return c * g
    rn = 1.0 / rows_of(features.double()).norm(dim=1, keepdim=True).clamp_min(1e-12)
    return c * rn * (g - (g * ref.x).sum(1, keepdim=True) * ref.x)


# ---------------------------------------------------------------------------------------------------------------------
# Bounds of hcir_supcon_fwd / hcir_supcon_bwd against the float64 reference taken on the inputs the kernel reads
# (already rounded to the tested dtype).
#
#   kap_ij = ||x_i|| ||x_j|| / |T|     the scale of logit ij (1/|T| with normalize)
#   eps_ij = (2 u_in + 2^-20) kap_ij   error of logit ij:  2 u_in : both operands are rows rounded to the compute dtype
#                                      after the normalisation (u_in = 0 without normalize: the rows are copied);
#                                      2^-20 : fp32 MFMA accumulation of the product, the fp32 normalisation, the
#                                      multiply by the fp32 inv_t log2(e) - the allowance oracle.ntxent gives them
#   lse_i   max_{j != i} eps_ij + 2^-19 max(1, |lse_i|)
#             a log-sum-exp moves by at most the largest move of its terms; 2^-19: fp32 exp2 / log2 / online merges and
#             the log2 <-> ln conversions, relative to the lse (absolute below 1)
#   row i   |T/T_base| a_i [ lse_i bound + max_{j in pos(i)} eps_ij                    the mean of the positive logits
#                           + (40 + ceil(N/128)) 2^-24 mean_{pos}|s_ij|               its fp32 summation: a lane adds
#                             at most 32 terms, 4 partials meet in LDS, then one per column tile; + the divide
#                           + 2^-21 (|lse_i| + |P_i / n_i|) ]                         subtract, times ln 2, times T/T_base
#   loss    mean_i row bound + 2^-20 mean_i |row loss_i|   (fp32 fixed-tree mean: at most N/1024 + 10 additions deep)
#   grad    g = W x.  Element error of g:
#             E_ik = (2^-10 + max(u_T, 2^-11)) (|W| |x|)_ik     W rounded to fp16 (2^-11) after an fp32 exp2 pair and
#                                                               the fp32 2/n_i (2^-11 of slack, also the fp32
#                                                               accumulation of hcir_gemm_f16); x copied to fp16
#                  + sum_j [a_i p_ij (eps_ij + lam_i) + a_j p_ji (eps_ij + lam_j)] |x_jk|
#                                                               relative error of p_ij: logit and lse errors, lam_i =
#                                                               lse bound + 2^-22 |lse_i| (the kernel's ln -> log2)
#                  + 2^-24 sum_j |x_jk| + 2^-25 sum_j |W_ij|    fp16 subnormal flush of W and of x
#           normalize = 0: dx = c g, c = |grad_out| / (|T_base| N):  c E + u_T |ref| + q
#           normalize = 1: c rn_i (E_ik + |u_ik| sum_m E_im |u_im| + 4 u_T |g_i.u_i| |u_ik|) + u_T |ref| + q
#           (oracle.ntxent.grad_bound's projection; q the output dtype's subnormal spacing times |grad_out|)
# ---------------------------------------------------------------------------------------------------------------------
def logit_eps(ref: ScRef, t, u_in):
    nx = ref.x.norm(dim=1)
    return (2 * u_in + 2.0 ** -20) * nx[:, None] * nx[None, :] / abs(t)


def lse_bound(ref: ScRef, t, u_in):
    eps = logit_eps(ref, t, u_in)
    eps = eps.masked_fill(torch.eye(eps.shape[0], dtype=torch.bool), 0.0)
    return eps.max(1).values + 2.0 ** -19 * ref.lse.abs().clamp_min(1.0)


def row_loss_bound(ref: ScRef, t, t_base, u_in):
    n = ref.lse.shape[0]
    eps = logit_eps(ref, t, u_in)
    pos_eps = (eps * ref.m).max(1).values
    cnt = ref.npos.clamp_min(1)
    mean_abs = (ref.sim.abs() * ref.m).sum(1) / cnt
    depth = 40 + (n + 127) // 128
    inner = lse_bound(ref, t, u_in) + pos_eps + depth * 2.0 ** -24 * mean_abs \
        + 2.0 ** -21 * (ref.lse.abs() + (ref.P / cnt).abs())
    return abs(t / t_base) * (ref.npos > 0).double() * inner


def loss_bound(ref: ScRef, t, t_base, u_in):
    return row_loss_bound(ref, t, t_base, u_in).mean() + 2.0 ** -20 * ref.row_loss.abs().mean() + 2.0 ** -149


def grad_bound(ref: ScRef, features, d_ref, t, t_base, normalize, grad_out, dtype, u_in):
    """[N, D] bound on |dx - d_ref| in row order; d_ref = rows_of(supcon_grad_f64(...)) at this grad_out."""
    u_t = U_ROUND[dtype]
    n = ref.x.shape[0]
    ax = ref.x.abs()
    a = (ref.npos > 0).double()
    eps = logit_eps(ref, t, u_in)
    lam = lse_bound(ref, t, u_in) + 2.0 ** -22 * ref.lse.abs()
    ep = a[:, None] * ref.p * (eps + lam[:, None])
    e = (2.0 ** -10 + max(u_t, 2.0 ** -11)) * (ref.W.abs() @ ax) + (ep + ep.t()) @ ax \
        + 2.0 ** -24 * ax.sum(0, keepdim=True) + 2.0 ** -25 * ref.W.abs().sum(1, keepdim=True)
    c = abs(grad_out) / (abs(t_base) * n)
    q = (2.0 ** -25 if dtype == torch.float16 else 2.0 ** -30) * abs(grad_out)
    if not normalize:
        return u_t * d_ref.abs() + c * e + q
    gu = ((ref.W @ ref.x) * ref.x).sum(1, keepdim=True)
    rn = 1.0 / rows_of(features.double()).norm(dim=1, keepdim=True).clamp_min(1e-12)
    return u_t * d_ref.abs() + c * rn * (e + ax * (e * ax).sum(1, keepdim=True) + 4 * u_t * gu.abs() * ax) + q


class ScProblem(NamedTuple):
    features: torch.Tensor          # CPU [B, V, D], tested dtype
    labels: Optional[torch.Tensor]  # CPU int64 [B] or None
    ref: ScRef
    dx: Optional[torch.Tensor]      # [N, D] float64 gradient rows at grad_out = 1 (None without a backward)
    u_in: float


@functools.lru_cache(maxsize=None)
def problem(family, label_family, case, dtype, normalize) -> ScProblem:
    """Inputs and float64 reference of one problem, computed once and shared; treat as read-only."""
    b, v, d, t, t_base = case
    f = make_features(family, b, v, d).to(dtype)
    labels = make_labels(label_family, b)
    ref = supcon_f64(f, labels, t, t_base, normalize, full=True)
    dx = rows_of(supcon_grad_f64(f, labels, t, t_base, normalize)) if has_backward(case) else None
    return ScProblem(f, labels, ref, dx, u_in_of(family, dtype, normalize))


# ---------------------------------------------------------------------------------------------------------------------
# Plain-torch emulation of the kernels' arithmetic (CPU): what the bounds must cover.
# ---------------------------------------------------------------------------------------------------------------------
def emulate(features, labels, t, t_base, normalize, grad_out=1.0, backward=True):
    """fp32 normalise -> round to T (or a copy); fp32 logits in the log2 domain; fp32 online-lse values, positive sum
    and count; W and x rounded to fp16; fp32 product; fp32 finish -> round to T.
    Returns (loss, lse, npos, dfeat [B, V, D] in the input dtype or None)."""
    dtype = features.dtype
    b, v, d = features.shape
    n = b * v
    f32 = torch.float32
    x = rows_of(features).float()
    inv = torch.ones(n, dtype=f32)
    xn = x
    if normalize:
        inv = 1.0 / torch.sqrt((x * x).sum(1)).clamp_min(1e-12)
        xn = (x * inv[:, None]).to(dtype).float()
    inv_t = torch.tensor(1.0 / t, dtype=f32)
    scale = inv_t * torch.tensor(_LOG2E, dtype=f32)
    raw = (xn @ xn.t()) * scale
    eye = torch.eye(n, dtype=torch.bool)
    x2 = raw.masked_fill(eye, float("-inf"))
    mx = x2.max(1).values
    lse2 = mx + torch.log2(torch.exp2(x2 - mx[:, None]).sum(1))
    ln2 = torch.tensor(_LN2, dtype=f32)
    lse = lse2 * ln2
    m = positive_mask(row_labels(labels, b, v))
    npos = m.sum(1)
    ps = (raw * m).sum(1)
    tob = torch.tensor(t / t_base, dtype=f32)
    row = torch.where(npos > 0, tob * ((lse2 - ps / npos.clamp_min(1).float()) * ln2), torch.zeros(n, dtype=f32))
    loss = row.sum() / n
    if not backward:
        return loss, lse, npos, None
    l2 = torch.where(npos > 0, lse * torch.tensor(_LOG2E, dtype=f32), torch.full((n,), float("inf"), dtype=f32))
    tw = torch.where(npos > 0, 2.0 / npos.clamp_min(1).float(), torch.zeros(n, dtype=f32))
    w = torch.exp2(raw - l2[:, None]) + torch.exp2(raw - l2[None, :])
    w = torch.where(m, w - tw[:, None], w)
    w = w.masked_fill(eye, 0.0).half().float()
    g = w @ xn.half().float()
    coef = torch.tensor(grad_out, dtype=f32) * torch.tensor(1.0 / t_base, dtype=f32) / torch.tensor(float(n), dtype=f32)
    if normalize:
        gu = (g * xn).sum(1, keepdim=True)
        dx = ((coef * inv)[:, None] * (g - gu * xn)).to(dtype)
    else:
        dx = (coef * g).to(dtype)
    return loss, lse, npos, torch.stack(torch.split(dx, b, 0), 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# Mutations of the float64 reference: the factor by which a kernel that makes a specific mistake (in every row, as a
# mistake in the code would) misses the bound - the loss for the forward's mistakes, the worst gradient element for
# the backward's.  inf = the mistake cannot be made at this shape / with these labels (it changes nothing there).
#   (a) the diagonal counted as a positive            (b) n_i off by one (n_i + 1)
#   (c) labels indexed by row, not by row mod B: other views of a sample belong to no class of the first view, the
#       view partner is not a positive               (d) one 128-wide column tile missing from P_i (least tile)
#   (e) rows with n_i = 0 given the softmax gradient  (f) only the low 32 bits of a label compared
#   (g) the G^T term missing from W
# ---------------------------------------------------------------------------------------------------------------------
def mutation_factors(pr: ScProblem, case, dtype, normalize):
    b, v, d, t, t_base = case
    n = b * v
    ref = pr.ref
    y = row_labels(pr.labels, b, v)
    eye = torch.eye(n, dtype=torch.bool)
    lb = loss_bound(ref, t, t_base, pr.u_in)
    inf = float("inf")

    def loss_factor(P, npos):
        row = (t / t_base) * (npos > 0).double() * (ref.lse - P / npos.clamp_min(1))
        return float((row.mean() - ref.loss).abs() / lb)

    out = {}
    out["a"] = loss_factor(ref.P + ref.sim.diagonal(), ref.npos + 1)
    out["b"] = loss_factor(ref.P, ref.npos + 1) if bool((ref.npos > 0).any()) else inf
    if v > 1 and b > 1:   # b == 1: the only other column is the positive and the loss is 0 either way
        view = torch.arange(n) // b
        mc = ref.m & (view[:, None] == view[None, :]) if pr.labels is not None else torch.zeros_like(ref.m)
        out["c"] = loss_factor((ref.sim * mc).sum(1), mc.sum(1))
    else:
        out["c"] = inf
    worst = inf
    for c0 in range(0, n, 128):
        keep = ref.m.clone()
        keep[:, c0:c0 + 128] = False
        if n > 128 and bool((keep != ref.m).any()):
            worst = min(worst, loss_factor((ref.sim * keep).sum(1), ref.npos))
    out["d"] = worst
    low = y & 0xFFFFFFFF
    mf = (low[:, None] == low[None, :]) & ~eye
    out["f"] = loss_factor((ref.sim * mf).sum(1), mf.sum(1)) if bool((mf != ref.m).any()) else inf
    if pr.dx is not None:
        bound = grad_bound(ref, pr.features, pr.dx, t, t_base, normalize, 1.0, dtype, pr.u_in)

        def grad_factor(W):
            return float(((closed_form_grad(ref, pr.features, t_base, normalize, W=W) - pr.dx).abs() / bound).max())

        G = (ref.npos > 0).double()[:, None] * (ref.p - ref.m.double() / ref.npos.clamp_min(1)[:, None])
        out["e"] = inf
        if bool((ref.npos == 0).any()):
            Ge = torch.where((ref.npos > 0)[:, None], G, ref.p)
            out["e"] = grad_factor(Ge + Ge.t())
        out["g"] = grad_factor(G) if bool(G.any()) else inf
    return out
