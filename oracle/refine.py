"""Host reference, real-number error bound, fp32 emulation and a list of kernel mistakes for hcir_topk_refine_f32
(csrc/refine.hip), the kernel that re-scores, ranks and CERTIFIES the candidates of the filtered search
(hcir/gallery.py).  numpy, no GPU.  tests/test_refine_host.py shows that the case table of tests/_refine_cases.py sees
every mistake below; tests/test_refine_gpu.py and tests/test_gallery_gpu.py hold the kernel to this file.

refine_ref      what the kernel must return, bit for bit.  Scores are oracle.knn.scores (the fp32 fmaf chain of the C
                oracle, (dot * gn) * qn).  A candidate with a negative index or a NaN score is dropped.  Order: score
                descending, index ascending.  Slots past the valid candidates: -inf / -1.  certified = 1 if
                cand_idx[kc-1] < 0 (the filter returned every row it has); otherwise k valid candidates must exist and
                fl32(t + err) < vk, t = cand_val[kc-1], vk = the k-th ranked score, the add in np.float32.
err_bound64     E_i of the hcir/gallery.py docstring as a real number: float64, from the actual fp32 rows and their
                fp16 roundings, no 1.01 and no 1e-7.
ei_kernel32     E_i as the kernel forms it when err_bound is NULL, operation by operation in fp32.

How far the kernel's E_i may lie above 1.01 E64 + 1e-7 (ei_delta).  u = 2^-24.  The kernel has
    s_q = sum x^2, s_d = sum (x - xh)^2, s_h = sum xh^2, xh = fp16(x):  lane l takes elements l + 64 j in a fused
    multiply-add chain of Q = ceil(d / 64) terms, then six butterfly additions.  xh is exact as a value, and x - xh is
    exact in fp32 (xh is within a factor two of x, or x is below the fp16 range and the difference is a multiple of
    ulp(x) no larger than x).  All terms are non-negative, so each sum carries at most Q + 6 relative roundings; the
    root halves that and adds one:                                  (Q + 6) / 2 + 1   on each norm.
    E = (nq eg + nd g16max + gamma (nq g32max + nh g16max)) 1.01f + 1e-7f, all terms non-negative, so the relative
    error of the sum is at most that of its worst path.  The longest is through gamma: two of the four constants as
    fp32 roundings of their float64 values (2), the inner product, the inner sum, the product with gamma, the outer
    sum, the product with 1.01f, the last sum (6), and 1.01f for 1.01 (1).  A compiler that fuses a product into a sum
    only removes roundings.  In all
        E_i <= (1.01 + delta) E64 + 1e-7 + r,   delta = 1.01 ((Q + 6) / 2 + 10) u (1 + 2^-9),
    the last factor for second order, and r = 2 u 1e-7 (1e-7f for 1e-7 and the last sum, 1.2e-14: below every
    resolution) goes into the probe's resolution.  No figure here is set against a result.

The recovery probe (probe_make, probe_bracket).  The kernel does not output E_i.  One launch holds n copies of one
query and its candidates; copy m has cand_val[kc-1] = t_m, fp32, and x_m = vk - t_m is exact in float64.  The kernel
certifies copy m iff fl32(t_m + E_i) < vk.  vk is an fp32 number, so rounding cannot carry a sum at or above vk below
it: certified means E_i < x_m exactly.  Not certified means fl32(t_m + E_i) >= vk, so t_m + E_i >= vk - ulp(vk) / 2.
With x_lo the largest uncertified x_m and x_hi the smallest certified one
        x_lo - ulp(vk) / 2 <= E_i < x_hi.
Soundness is asserted on the lower end (E64 <= x_lo - ulp(vk) / 2, which proves E64 <= E_i), tightness on the upper
(x_hi <= (1.01 + delta) E64 + 1e-7 + resolution, resolution = x_hi - x_lo + ulp(vk) / 2 + r).  The candidate rows are
nearly orthogonal to the query, so |vk| is far below E and ulp(vk) does not limit the grid.

The planted galleries (plant) are described at the function.
"""
from __future__ import annotations

import numpy as np

from oracle import knn as oknn

U32 = 2.0 ** -24
NINF = np.float32(-np.inf)
UNWRITTEN_IDX = -777           # what refine_ref leaves in a slot that a mistaken kernel does not write (value: NaN)

MISTAKES = ("<= for <",
            "k-th score read at rank k",
            "t read at cand_val[k-1]",
            "tie to the larger index",
            "NaN ranks first",
            "empty tail slots unwritten",
            "gn indexed by id",
            "E_i without the ||q - q~|| g16max term",
            "E_i without the ||q|| eg term",
            "E_i without the gamma terms",
            "E_i without the safety factor")
LE, KTH_AT_K, T_AT_K, TIE_LARGER, NAN_FIRST, TAIL_UNWRITTEN, GN_BY_ID, NO_QTERM, NO_GTERM, NO_GAMMA, NO_FACTOR = MISTAKES
E_MISTAKES = (NO_QTERM, NO_GTERM, NO_GAMMA, NO_FACTOR)


def cdiv(a, b):
    return -(-a // b)


def f16(x):
    """round to nearest even to fp16, as float64 values"""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def refine_ref(q, g, cand_idx, cand_val, k, idx_base=0, qn=None, gn=None, err=None, consts=None, mistake=None):
    """-> (out_val fp32 [nq, k], out_idx int64 [nq, k], certified int32 [nq]).  err: fp32 [nq], or None: then E_i is
    ei_kernel32(q, consts).  mistake: one of MISTAKES, the same function with that kernel mistake in it."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    cand_idx = np.asarray(cand_idx, dtype=np.int64)
    cand_val = np.asarray(cand_val, dtype=np.float32)
    nq, kc = cand_idx.shape
    ng = g.shape[0]
    if err is None:
        err = ei_kernel32(q, consts, mistake)
    err = np.asarray(err, dtype=np.float32)
    out_val = np.full((nq, k), NINF, dtype=np.float32)
    out_idx = np.full((nq, k), -1, dtype=np.int64)
    cert = np.zeros(nq, dtype=np.int32)
    for i in range(nq):
        ids = cand_idx[i]
        live = np.nonzero(ids >= 0)[0]
        loc = ids[live] - idx_base
        sc = np.empty(0, dtype=np.float32)
        if live.size:
            gsel = None
            if gn is not None:
                gsel = np.asarray(gn, dtype=np.float32)[(ids[live] % ng) if mistake == GN_BY_ID else loc]
            sc = oknn.scores(q[i:i + 1], g[loc], None if qn is None else np.asarray(qn, dtype=np.float32)[i:i + 1],
                             gsel)[0]
        key = sc.astype(np.float64)
        if mistake == NAN_FIRST:
            key = np.where(np.isnan(key), np.inf, key)
        else:
            keep = ~np.isnan(key)
            live, sc, key = live[keep], sc[keep], key[keep]
        cid = ids[live]
        order = np.lexsort((cid if mistake != TIE_LARGER else -cid, -key))       # score descending, index ascending
        sc, cid = sc[order], cid[order]
        nv = min(sc.size, k)
        out_val[i, :nv], out_idx[i, :nv] = sc[:nv], cid[:nv]
        if mistake == TAIL_UNWRITTEN:
            out_val[i, nv:], out_idx[i, nv:] = np.float32(np.nan), UNWRITTEN_IDX
        if ids[kc - 1] < 0:
            cert[i] = 1
            continue
        kth = k if mistake == KTH_AT_K else k - 1
        if sc.size <= kth:
            continue
        t = cand_val[i, (k - 1) if mistake == T_AT_K else (kc - 1)]
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.float32(t) + np.float32(err[i])
            cert[i] = int(s <= sc[kth]) if mistake == LE else int(s < sc[kth])
    return out_val, out_idx, cert


def brute_force(q, g, cand_idx, cand_val, k, idx_base=0, qn=None, gn=None, err=None):
    """refine_ref again with nothing shared but the C oracle's scalar chain: every score of the gallery, python
    tuples, sorted()"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    full = oknn.scores(q, g, qn, gn, mode=oknn.MODE_CHAIN32_SCALAR)
    nq, kc = np.asarray(cand_idx).shape
    out_val = np.full((nq, k), NINF, dtype=np.float32)
    out_idx = np.full((nq, k), -1, dtype=np.int64)
    cert = np.zeros(nq, dtype=np.int32)
    for i in range(nq):
        rows = []
        for c in range(kc):
            j = int(cand_idx[i][c])
            if j >= 0 and full[i, j - idx_base] == full[i, j - idx_base]:
                rows.append((-float(full[i, j - idx_base]), j, full[i, j - idx_base]))
        rows.sort(key=lambda r: (r[0], r[1]))
        for p, r in enumerate(rows[:k]):
            out_val[i, p], out_idx[i, p] = r[2], r[1]
        if cand_idx[i][kc - 1] < 0:
            cert[i] = 1
        elif len(rows) >= k:
            with np.errstate(invalid="ignore", over="ignore"):
                cert[i] = int(np.float32(cand_val[i][kc - 1]) + np.float32(err[i]) < rows[k - 1][2])
    return out_val, out_idx, cert


def same_bits(a, b):
    """(val, idx, cert) triples equal bit for bit (NaN included)"""
    return (np.array_equal(np.asarray(a[0], dtype=np.float32).view(np.int32),
                           np.asarray(b[0], dtype=np.float32).view(np.int32))
            and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


def e_star(t, vk):
    """the smallest fp32 e with fl32(t + e) >= vk, elementwise (t < vk, both finite fp32) -> (e*, the fp32 below it)"""
    t = np.asarray(t, dtype=np.float32)
    vk = np.asarray(vk, dtype=np.float32)
    assert (t < vk).all()
    lo = np.zeros(t.shape, dtype=np.int32)                         # bits of +0: fl32(t + 0) < vk
    hi = np.full(t.shape, np.float32(np.inf).view(np.int32))       # bits of +inf: holds.  Positive floats order as ints
    with np.errstate(over="ignore"):
        while (hi - lo > 1).any():                                 # fl32(t + e) is monotone in e: bisection
            mid = lo + (hi - lo) // 2
            ok = (t + mid.view(np.float32)) >= vk
            hi, lo = np.where(ok, mid, hi), np.where(ok, lo, mid)
    e, below = hi.view(np.float32), lo.view(np.float32)
    assert ((t + e) >= vk).all() and ((t + below) < vk).all()
    return e, below


# ---------------------------------------------------------------------------------------------------------------
# E_i
# ---------------------------------------------------------------------------------------------------------------
def gamma_d(d):
    return d * U32 / (1.0 - d * U32)


def mirror_consts64(g, mirror=None):
    """(eg, g16max, g32max, gamma) in float64 from the fp32 rows g and their fp16 mirror (made here if None)"""
    g64 = np.asarray(g, dtype=np.float32).astype(np.float64)
    m64 = f16(g) if mirror is None else np.asarray(mirror).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (float(np.linalg.norm(g64 - m64, axis=1).max()), float(np.linalg.norm(m64, axis=1).max()),
                float(np.linalg.norm(g64, axis=1).max()), gamma_d(g64.shape[1]))


def e64_from(q, consts, drop=None):
    """E_i [nq] in float64 from float64 constants; drop: one of E_MISTAKES' terms left out (never the factor: there
    is none here)"""
    eg, g16max, g32max, gamma = (float(c) for c in consts)
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    qh = f16(q)
    nq_, nd_, nh_ = (np.linalg.norm(v, axis=1) for v in (q64, q64 - qh, qh))
    t_g = 0.0 if drop == NO_GTERM else nq_ * eg
    t_q = 0.0 if drop == NO_QTERM else nd_ * g16max
    t_r = 0.0 if drop == NO_GAMMA else gamma * (nq_ * g32max + nh_ * g16max)
    return t_g + t_q + t_r


def err_bound64(q, g, mirror=None):
    """-> (E [nq] float64, (eg, g16max, g32max, gamma) float64)"""
    consts = mirror_consts64(g, mirror)
    return e64_from(q, consts), consts


def consts32(consts):
    return np.asarray(consts, dtype=np.float32)


def ei_delta(d):
    return 1.01 * ((cdiv(d, 64) + 6) / 2 + 10) * U32 * (1 + 2.0 ** -9)


def ei_upper(e64, d):
    """the upper bound on the kernel's E_i, the probe's resolution not included"""
    return (1.01 + ei_delta(d)) * e64 + 1e-7


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ei_kernel32(q, consts, mistake=None):
    """the kernel's own evaluation, fp32 [nq]: lane chains, butterfly, three roots, the sum (no fusing: one rounding
    per operation)"""
    q = np.asarray(q, dtype=np.float32)
    n, d = q.shape
    eg, g16max, g32max, gamma = (np.float32(c) for c in consts32(consts))
    chunks = cdiv(d, 64)
    x = np.zeros((n, chunks * 64), dtype=np.float32)
    x[:, :d] = q
    x = x.reshape(n, chunks, 64)
    with np.errstate(over="ignore"):
        xh = x.astype(np.float16).astype(np.float32)
    dl = x - xh
    s = [np.zeros((n, 64), dtype=np.float32) for _ in range(3)]
    for j in range(chunks):
        for m, v in enumerate((x[:, j], dl[:, j], xh[:, j])):
            s[m] = _fma32(v, v, s[m])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = [v + v[:, lanes ^ o] for v in s]
    nq_, nd_, nh_ = (np.sqrt(v[:, 0]) for v in s)
    zero = np.zeros(n, dtype=np.float32)
    t_g = zero if mistake == NO_GTERM else nq_ * eg
    t_q = zero if mistake == NO_QTERM else nd_ * g16max
    t_r = zero if mistake == NO_GAMMA else gamma * (nq_ * g32max + nh_ * g16max)
    e = t_g + t_q + t_r
    if mistake != NO_FACTOR:
        e = e * np.float32(1.01) + np.float32(1e-7)
    return e.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# the recovery probe
# ---------------------------------------------------------------------------------------------------------------
PROBE_COPIES = 1024
PROBE_KC, PROBE_K = 3, 2
PROBE_FAMILIES = ("norm 1e-3", "norm 1", "norm 50", "fp16 exact", "below fp16", "d 8", "d 2048")


def probe_query(family, seed=0):
    """-> (q fp32 [d], g fp32 [ng, d]): the gallery gives the mirror constants; rows 0 .. 2, the candidates, are
    nearly orthogonal to q"""
    rng = np.random.default_rng(1000 + seed)
    d = {"d 8": 8, "d 2048": 2048}.get(family, 200)               # 200: a ragged last trip of the lane loop
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    if family == "norm 1e-3":
        q *= 1e-3
    elif family == "norm 50":
        q *= 50.0
    elif family == "below fp16":
        q *= 1e-8 * np.sqrt(d)                                    # elements near 1e-8 < 2^-25: fp16(x) = 0
    q = q.astype(np.float32)
    if family == "fp16 exact":
        q = q.astype(np.float16).astype(np.float32)
    g = rng.standard_normal((40, d)) * 10.0 ** rng.uniform(-1, 1, (40, 1))
    q64 = q.astype(np.float64)
    for j in range(PROBE_KC):                                     # candidates: the component along q removed
        g[j] -= (g[j] @ q64) / (q64 @ q64) * q64
    return q, g.astype(np.float32)


def probe_make(q, g, copies=PROBE_COPIES):
    """-> dict of the launch's inputs: `copies` rows of the same query and candidates 0 .. PROBE_KC-1 (mirror-style
    values), cand_val[:, kc-1] = t_m on a grid of x = vk - t around 1.01 E64 + 1e-7 with step E64 2^-22, and what
    probe_bracket needs"""
    e64, c64 = err_bound64(q[None], g)
    e64 = float(e64[0])
    consts = consts32(c64)
    cand_idx = np.tile(np.arange(PROBE_KC, dtype=np.int64), (copies, 1))
    sc = oknn.scores(q[None], g[:PROBE_KC])[0]
    vk = np.sort(sc)[::-1][PROBE_K - 1]
    centre = 1.01 * e64 + 1e-7
    x = centre + (np.arange(copies) - copies // 2) * (e64 * 2.0 ** -22)
    t = (np.float64(vk) - x).astype(np.float32)
    cand_val = np.tile(np.float32([1.0, 0.5, 0.0]), (copies, 1))
    cand_val[:, PROBE_KC - 1] = t
    return dict(q=np.tile(q, (copies, 1)), g=g, cand_idx=cand_idx, cand_val=cand_val, consts=consts, e64=e64,
                vk=np.float32(vk), x=np.float64(vk) - t.astype(np.float64), d=q.shape[0])


def probe_bracket(p, certified):
    """-> dict(lo, hi, resolution, sound, tight, monotone): lo <= E_i < hi as derived at the top of the file"""
    cert = np.asarray(certified).astype(bool)
    x = p["x"]
    half_ulp = float(np.spacing(np.abs(p["vk"]))) / 2 if p["vk"] != 0 else 2.0 ** -150
    if cert.all() or not cert.any():
        return dict(lo=-np.inf if cert.all() else x.max(), hi=x.min() if cert.all() else np.inf, resolution=np.inf,
                    sound=not cert.any(), tight=not cert.all(), monotone=True, inside=False)
    x_lo, x_hi = x[~cert].max(), x[cert].min()
    res = (x_hi - x_lo) + half_ulp + 2 * U32 * 1e-7
    return dict(lo=x_lo - half_ulp, hi=x_hi, resolution=res, inside=True,
                monotone=bool(x_lo < x_hi), sound=bool(p["e64"] <= x_lo - half_ulp),
                tight=bool(x_hi <= ei_upper(p["e64"], p["d"]) + res))


# ---------------------------------------------------------------------------------------------------------------
# planted galleries: a too-small E_i returns a wrong top-k
# ---------------------------------------------------------------------------------------------------------------
PLANT_D, PLANT_K, PLANT_KC = 64, 5, 16
PLANT_POOL = 200000
PLANT_MARGIN = 5e-6            # every strict inequality below holds by this much in float64; the chain's error is 1e-7
PLANTED_QUERY = 1              # the row of the query batch that is planted; the others are ordinary


def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def plant(kind, seed=0):
    """kind "query": the ||q - q~|| g16max term is what keeps the search exact.  Gallery rows are exactly
    fp16-representable (eg = 0), the query is not.  kind "gallery": the ||q|| eg term.  The query is
    fp16-representable, and row A carries an offset of 0.9 of half an fp16 ulp in the direction sign(q), which the
    mirror rounds away.  Both, at d = 64, k = 5, 16 filter candidates:
        four rows well above everything;  a neutral row N with exact score c and a mirror score next to it;
        the hidden row A: exact score in (c, c + 3e-5), mirror score about 1e-4 lower;
        eleven fillers: exact score below c, mirror score strictly between s16(A) and c - E_mutant;
        a hundred rows far below.
    The exact top-5 is the four and A.  The filter's 16 are the four, N and the fillers: A is 17th.  Among the 16 the
    fifth exact score is vk = c, and the 16th mirror score t is a filler's, so t + E_mutant < vk, and the mutant
    certifies a list without A.  The real bound has t + E64 > s16(A) + err(A) = exact(A) > vk.
    Rows are taken by rejection from a pool of unit vectors, by float64 scores.
    -> dict(q [3, d], g [ng, d], a, n: gallery indices of A and N, filter16: the indices the filter must return for the
    planted query, drop: the E_i mistake this gallery exposes)"""
    rng = np.random.default_rng(77 + seed + (0 if kind == "query" else 500))
    d = PLANT_D
    q = _unit_rows(rng, 1, d)[0].astype(np.float32)
    pool = _unit_rows(rng, PLANT_POOL, d).astype(np.float32)
    if kind == "query":
        pool = pool.astype(np.float16).astype(np.float32)
        delta = q.astype(np.float64) - f16(q)
        lean = 0.45 * delta / np.linalg.norm(delta) + 0.89 * _unit_rows(rng, 4000, d)
        cands = lean.astype(np.float16).astype(np.float32)
        drop = NO_QTERM
    else:
        q = q.astype(np.float16).astype(np.float32)
        base = _unit_rows(rng, 4000, d).astype(np.float16)
        ulp = np.spacing(np.abs(base)).astype(np.float64)         # of the fp16 value
        cands = (base.astype(np.float64) + 0.9 * 0.5 * ulp * np.sign(q.astype(np.float64))).astype(np.float32)
        drop = NO_GTERM
    q64, qh = q.astype(np.float64), f16(q)

    def both(rows):
        return rows.astype(np.float64) @ q64, f16(rows) @ qh

    m = PLANT_MARGIN
    ex_c, s_c = both(cands)
    ok = np.nonzero((ex_c - s_c > 0.8e-4) & (ex_c - s_c < 1.6e-4) & (np.abs(ex_c) < 0.1))[0]
    assert ok.size, "no hidden row"
    ex, s16 = both(pool)
    e_mut = 1.02 * gamma_d(d) * 2.2 * 1.01 + 2e-7                # above what a mutant forms here: norms of 1 to 1.1
    for a in ok:
        hi_a, lo_a = ex_c[a], s_c[a]
        near = np.nonzero((ex > hi_a - 3e-5) & (ex < hi_a - m) & (s16 > lo_a + m))[0]
        if not near.size:
            continue
        n = near[np.argmin(np.abs(ex[near] - s16[near]))]
        c = ex[n]
        fill = np.nonzero((s16 > lo_a + m) & (s16 < c - e_mut - m) & (ex < c - m))[0]
        fill = fill[fill != n]
        if fill.size >= 11 and s16[n] > s16[fill].min():
            break
    else:
        raise AssertionError("no planted gallery in the pool")
    fill = fill[:11]
    high = np.argsort(-ex)[:4]
    low = np.nonzero((ex < c - 0.05) & (s16 < lo_a - 0.05))[0][:100]
    assert ex[high].min() > c + 0.2 and s16[high].min() > c + 0.2 and low.size == 100
    rows = np.concatenate([pool[high], pool[n][None], cands[a][None], pool[fill], pool[low]])
    perm = rng.permutation(rows.shape[0])
    where = np.empty_like(perm)
    where[perm] = np.arange(perm.size)                            # old position -> gallery index
    queries = np.stack([_unit_rows(rng, 1, d)[0].astype(np.float32), q, _unit_rows(rng, 1, d)[0].astype(np.float32)])
    return dict(q=queries, g=np.ascontiguousarray(rows[perm]), a=int(where[5]), n=int(where[4]), drop=drop,
                filter16=np.sort(np.concatenate([where[:5], where[6:17]])))


def plant_facts(p):
    """the preconditions of a planted gallery from float64 scores (and the oracle's chain for vk) -> dict; every
    entry of `holds` must be True"""
    q, g = p["q"][PLANTED_QUERY], p["g"]
    m = PLANT_MARGIN
    s16 = f16(g) @ f16(q)
    order = np.argsort(-s16, kind="stable")
    filt = order[:PLANT_KC]
    t = s16[filt[-1]]
    chain = oknn.scores(q[None], g)[0]
    _, top = oknn.cosine_topk(q[None], g, PLANT_K)
    vk = np.sort(chain[filt])[::-1][PLANT_K - 1]
    e64, c64 = err_bound64(q[None], g)
    e_mut = float(ei_kernel32(q[None], c64, p["drop"])[0])
    ex = g.astype(np.float64) @ q.astype(np.float64)
    holds = {
        "the filter's 16 are the planted ones": np.array_equal(np.sort(filt), p["filter16"]),
        "A is 17th in the mirror, clear of both neighbours": order[16] == p["a"] and s16[order[15]] - s16[p["a"]] > m
                                                              and s16[p["a"]] - s16[order[17]] > m,
        "A is the exact 5th": top[0, PLANT_K - 1] == p["a"],
        "A is not among the 16": p["a"] not in filt,
        "the exact 5th and 6th are clear of each other": ex[p["a"]] - ex[p["n"]] > m,
        "vk is N's score": vk == chain[p["n"]],
        "t + E_mutant < vk": t + e_mut + m < vk,
        "vk <= t + E64": vk + m <= t + e64[0],
        "E_mutant is the smaller by far": e_mut * 4 < e64[0],
    }
    return dict(holds=holds, t=float(t), vk=float(vk), e64=float(e64[0]), e_mut=e_mut, err_a=float(ex[p["a"]] - s16[p["a"]]),
                window=float(vk - e_mut - s16[p["a"]]), top=top[0], filt=filt)
