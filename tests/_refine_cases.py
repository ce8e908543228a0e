"""The case table of hcir_topk_refine_f32 that tests/test_refine_host.py (no GPU: the table can see every mistake of
oracle.refine.MISTAKES) and tests/test_refine_gpu.py (the kernel, bit for bit) both read.

A case is a dict of numpy inputs made by build(spec).  Candidates are the kc best rows under a NOISY score (the exact
float64 score plus noise as large as the gaps between neighbours), given in that order with those values: the kernel
must really permute them.  Gallery rows and queries have norms from 1e-2 to 1e2, the inverse norms are those of the
rows, so scores with both are cosines and scores with one or none are far from 1.  err_bound alternates between e*
(the smallest fp32 that must NOT certify) and the fp32 below it (must certify), so every case holds both flags."""
import numpy as np

from oracle import refine as orf

NG = 300
IDX_BASES = (0, 7, 1 << 33)
NORMS = ((False, False), (True, False), (False, True), (True, True))            # (q_inv_norm, g_inv_norm)
COMBOS = [(b, n) for b in IDX_BASES for n in NORMS]
SHAPES = [(1, 8, 1, 1), (3, 24, 2, 1), (4, 40, 2, 2), (5, 72, 16, 5), (130, 256, 16, 14), (5, 768, 17, 9),
          (3, 2048, 63, 1), (4, 2048, 64, 64), (5, 8, 64, 30), (130, 24, 63, 63), (4, 768, 16, 16), (3, 256, 17, 1)]


def _spec(name, nq, d, kc, k, combo, **kw):
    s = dict(name=name, nq=nq, d=d, kc=kc, k=k, idx_base=combo[0], use_qn=combo[1][0], use_gn=combo[1][1], ng=NG,
             empty=0, nan=None, dup=False, seed=0)
    s.update(kw)
    return s


def specs():
    out = []
    for n, (shape, combo) in enumerate(zip(SHAPES, COMBOS)):                     # every shape, each with one combination
        out.append(_spec("shape", *shape, combo, seed=n, ng=4096 if n == 4 else NG))
    for n, combo in enumerate(COMBOS):                                           # every combination on one shape
        out.append(_spec("combo", 5, 72, 16, 5, combo, seed=20 + n, dup=n % 2 == 0))
    c = COMBOS[7]                                                                # idx_base 7, both norms
    out += [
        _spec("duplicates", 5, 40, 17, 9, c, dup=True, seed=40),
        _spec("duplicates k=kc", 3, 24, 2, 2, COMBOS[4], dup=True, seed=41),
        _spec("some empty", 5, 72, 16, 5, c, empty=4, seed=42),
        _spec("fewer than k valid", 5, 72, 16, 9, c, empty=11, seed=43),         # 5 valid: slots [5, 9) are filled
        _spec("fewer than k valid, kc 64", 3, 40, 64, 64, COMBOS[9], empty=41, seed=44),
        _spec("all empty", 5, 72, 16, 5, c, empty=16, seed=45),
        _spec("all empty kc 1", 4, 8, 1, 1, COMBOS[0], empty=1, seed=46),
        _spec("NaN row, k reachable", 5, 72, 16, 5, c, nan="reachable", seed=47),
        _spec("NaN row, fewer than k valid", 5, 72, 16, 16, c, nan="short", seed=48),   # 15 valid, cand_idx[kc-1] >= 0
        _spec("NaN row and empty", 5, 40, 17, 9, COMBOS[10], nan="reachable", empty=3, dup=True, seed=49),
    ]
    return out


def spec_id(s):
    return (f"{s['name']}-nq{s['nq']}-d{s['d']}-kc{s['kc']}-k{s['k']}-base{s['idx_base']}"
            f"-{'qn' if s['use_qn'] else ''}{'gn' if s['use_gn'] else ''}")


def build(s):
    rng = np.random.default_rng(s["seed"] + 31 * s["d"] + s["kc"])
    nq, d, kc, k, ng = s["nq"], s["d"], s["kc"], s["k"], s["ng"]
    g = (rng.standard_normal((ng, d)) * 10.0 ** rng.uniform(-2, 2, (ng, 1))).astype(np.float32)
    q = (rng.standard_normal((nq, d)) * 10.0 ** rng.uniform(-2, 2, (nq, 1))).astype(np.float32)
    dup = None
    if s["dup"]:
        dup = (11, 200)                                                          # equal rows, two indices
        g[dup[1]] = g[dup[0]]
    nan_row = None
    if s["nan"]:
        nan_row = 123
        g[nan_row, d // 2] = np.nan
    with np.errstate(invalid="ignore"):
        gn = (1.0 / np.linalg.norm(g.astype(np.float64), axis=1)).astype(np.float32)
    gn[~np.isfinite(gn)] = 1.0
    qn = (1.0 / np.linalg.norm(q.astype(np.float64), axis=1)).astype(np.float32)
    exact = np.nan_to_num(q.astype(np.float64) @ np.nan_to_num(g.astype(np.float64)).T)
    if s["use_gn"]:
        exact = exact * gn
    if s["use_qn"]:
        exact = exact * qn[:, None]
    spread = np.sort(exact, axis=1)[:, ::-1]
    gap = (spread[:, 0] - spread[:, min(kc, ng - 1)]) / max(kc, 1)               # the mean gap among the best kc
    noisy = exact + 2.0 * gap[:, None] * rng.standard_normal(exact.shape)
    cand_idx = np.empty((nq, kc), dtype=np.int64)
    cand_val = np.empty((nq, kc), dtype=np.float32)
    for i in range(nq):
        order = list(np.argsort(-noisy[i], kind="stable")[:kc])
        forced = []
        if dup is not None and kc >= 2:
            forced += [dup[1], dup[0]]                                           # the larger index first
        if nan_row is not None:
            forced.insert(1 if forced else 0, nan_row)
        forced = forced[:kc]
        rest = [j for j in order if j not in forced]
        order = rest[:kc - len(forced)]
        for p, j in enumerate(forced):                                           # spread over the list, in this order
            order.insert(min(len(order), (p * kc) // max(len(forced), 1)), j)
        cand_idx[i] = order
        cand_val[i] = np.sort(noisy[i, order])[::-1]
    valid = kc - s["empty"]
    if s["nan"] == "short":
        assert valid - 1 < k <= valid
    cand_idx += s["idx_base"]
    cand_idx[:, valid:] = -1
    cand_val[:, valid:] = -np.inf
    case = dict(q=q, g=g, cand_idx=cand_idx, cand_val=cand_val, k=k, idx_base=s["idx_base"],
                qn=qn if s["use_qn"] else None, gn=gn if s["use_gn"] else None, dup=dup, nan_row=nan_row)
    # err_bound at the decision: with err = 0 the reference gives vk; e* and the number below it alternate
    case["err"] = np.full(nq, 0.5, dtype=np.float32)
    val, _, _ = orf.refine_ref(err=case["err"], **ref_args(case))
    vk, t = val[:, k - 1], cand_val[:, kc - 1]
    ok = np.isfinite(vk) & np.isfinite(t)
    if ok.any():
        t_ok = np.where(t < vk, t, vk - np.abs(vk) - 1).astype(np.float32)       # the list's tail is noisy: put t below vk
        case["cand_val"][ok, kc - 1] = t_ok[ok]
        e, below = orf.e_star(t_ok[ok], vk[ok])
        case["err"][ok] = np.where(np.arange(int(ok.sum())) % 2 == 0, e, below)
    case["decided"] = ok
    # every third query: t + err == vk exactly, in real numbers (must not certify: the inequality is strict)
    case["equal"] = np.zeros(nq, dtype=bool)
    for i in np.nonzero(ok)[0][2::3]:
        v = np.float64(vk[i])
        if v == 0:
            continue
        e = 2.0 ** (np.floor(np.log2(abs(v))) - 6)
        t_eq = v - e
        if np.float64(np.float32(t_eq)) == t_eq:
            case["cand_val"][i, :kc - 1] = np.maximum(case["cand_val"][i, :kc - 1], np.float32(t_eq))   # still sorted
            case["cand_val"][i, kc - 1], case["err"][i], case["equal"][i] = t_eq, e, True
    return case


def decision_runs(case):
    """-> [(err array, expected certified)] over the decided queries of a case: all at e*, all at the number below"""
    ok = case["decided"]
    t = case["cand_val"][ok, -1]
    val, _, _ = orf.refine_ref(err=case["err"], **ref_args(case))
    e, below = orf.e_star(t, val[ok, case["k"] - 1])
    runs = []
    for arr, want in ((e, 0), (below, 1)):
        err = case["err"].copy()
        err[ok] = arr
        runs.append((err, np.where(ok, want, -1)))
    return runs


def ref_args(case):
    return {k: case[k] for k in ("q", "g", "cand_idx", "cand_val", "k", "idx_base", "qn", "gn")}
