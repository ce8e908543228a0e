"""CPU-only: the error bounds of oracle.rowops are honest and sharp.

Honest: the plain-torch emulations of the kernels' arithmetic (element 4 (lane + 64 j) + e per lane, the xor-butterfly
wave_sum, fma where the kernel has one, the wave-order LDS combination and the 16-lane finalize tree) stay inside the
bounds (max err / bound <= 1) on every input family at every width of tests/test_rowops_gpu.py.  Sharp: each listed
kernel mistake, applied to the float64 reference, exceeds the bound at least 10-fold on at least one family, over the
elements the mistake touches.  The tables are printed (pytest -s; profiles/rowops_bounds.txt keeps a copy).

A mistake is restated on every output it reaches (the fp16 LayerNorm rows, the fp32 CLS embedding with and without
the L2 normalisation, the patch mean) and the largest factor counts: a relative mistake of the size of h (the
normalised value rounded to fp16, the unbiased variance at d ~ 1000) is 1 - 4 x the bound of an fp16 row whose |y| is
ordinary and shows on the `cancel` row (y ~ 0) and on the fp32 outputs.

Families that cannot show a mistake, by construction:
  constant  x - mean = 0 in float64: whatever only changes rstd or the divisor of the variance leaves y = beta;
  marker    one-hot rows: the statistics are those of a single value, |c| ~ |x|, nothing cancels; the last column
            group holds the one-hot column of few rows or none (d = 1028: 1.3 x for the group left out).
No listed mistake stays below the 10 x bar (BELOW_BAR is empty; the mechanism of tests/test_gemm_host.py is kept).
"""
import functools

import pytest
import torch

from oracle import rowops as ro

FWD_D = (4, 260, 768, 1024, 1028, 1280, 1284, 2048)
BWD_D = (4, 256, 260, 768, 1024, 1028, 2048, 2052, 4096)
COLSUM_SHAPES = ((1, 8), (7, 8), (13, 264), (513, 8), (1025, 256), (131073, 8))
BELOW_BAR = ()
ROWS = 30                  # [15, 2, d], [10, 3, d] and [5, 6, d] token views; row 6 is a class token in each
CANCEL = 6
DT = {"f32": torch.float32, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def problem(family, rows, d, xdt, cancel_row=None):
    p = ro.make_problem(family, rows, d, cancel_row=cancel_row)
    p["x"] = p["x"].to(DT[xdt])
    if family == "cancel":
        p = ro.apply_cancel(p, p["x"])
    return p


def _print(tag, worst):
    print(f"\nrowops-emu {tag}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------
# (a) the emulations stay inside the bounds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", FWD_D)
@pytest.mark.parametrize("family", ro.FAMILIES)
def test_forward_emulations_within_bounds(family, d, xdt):
    p = problem(family, ROWS, d, xdt, CANCEL)
    x, ga, be = p["x"], p["gamma"], p["beta"]
    worst = {"ln": ro.ratio(ro.emulate_layernorm(x, ga, be), *ro.layernorm_f64(x, ga, be))}
    tok = x.view(10, 3, d)
    for g, b in ((ga, be), (None, None)):
        for l2 in (0, 1):
            o32, o16 = ro.emulate_cls_head(tok, g, b, l2=l2)
            ref, b32, b16 = ro.cls_head_f64(tok, g, b, l2=l2)
            name = "cls" + ("+ln" if g is not None else "") + ("+l2" if l2 else "")
            worst[name + "/f32"], worst[name + "/f16"] = ro.ratio(o32, ref, b32), ro.ratio(o16, ref, b16)
            if l2:
                worst[name + "/norm32"] = float(((o32.double().norm(dim=1) - 1).abs() / ro.norm_bound(d, False)).max())
                worst[name + "/norm16"] = float(((o16.double().norm(dim=1) - 1).abs() / ro.norm_bound(d, True)).max())
        for t in (2, 3, 6):
            tk = x.view(ROWS // t, t, d)
            worst[f"pm{'+ln' if g is not None else ''}/t{t}"] = ro.ratio(ro.emulate_patch_mean(tk, g, b),
                                                                          *ro.patch_mean_f64(tk, g, b))
    _print(f"fwd {family:8s} d {d:4d} {xdt}", worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def _bwd_ratios(p, rows, accumulate, with_dres):
    x, dy, ga = p["x"][:rows], p["dy"][:rows], p["gamma"]
    dres_in = p["dres_in"][:rows] if with_dres else None
    old = (p["old_dgamma"], p["old_dbeta"])
    ref = ro.layernorm_bwd_f64(x, dy, ga, dres_in=dres_in, old=old, accumulate=accumulate)
    emu = ro.emulate_layernorm_bwd(x, dy, ga, dres_in=dres_in, old=old, accumulate=accumulate, fused=True)
    worst = {k: ro.ratio(emu[k], *ref[k]) for k in ("dres", "dgamma", "dbeta")}
    assert torch.equal(emu["dres16"], emu["dres"].half())
    worst["dres_colsum"] = ro.ratio(emu["dres_colsum"], *ro.dres_colsum_f64(emu["dres16"]))
    return worst


@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", BWD_D)
@pytest.mark.parametrize("family", ro.FAMILIES)
def test_backward_emulations_within_bounds(family, d, xdt):
    p = problem(family, 65, d, xdt, 2)
    for rows in (1, 5, 65):
        for accumulate, with_dres in ((0, True), (1, False)):
            if family == "cancel" and not with_dres:
                continue
            worst = _bwd_ratios(p, rows, accumulate, with_dres)
            _print(f"bwd {family:8s} d {d:4d} rows {rows:2d} {xdt} acc {accumulate}", worst)
            assert all(v <= 1.0 for v in worst.values()), worst


def test_backward_row_loop_emulation_within_bounds():
    """65606 rows at d = 4: 1024 workgroups, 16 or 17 rows per wave"""
    rows = 65606
    assert ro.ln_bwd_blocks(rows) == 1024 and ro.cdiv(rows, 4096) == 17 and ro.ln_bwd_depth(rows) == 17 + 64 + 18
    worst = _bwd_ratios(problem("plain", rows, 4, "f32"), rows, 1, True)
    _print("bwd plain d 4 rows 65606", worst)
    assert all(v <= 1.0 for v in worst.values()), worst


DH_PATTERNS, dh_pattern = ro.DH_PATTERNS, ro.dh_pattern


def test_gelu_emulations_within_bounds():
    u = ro.all_finite_f16()
    assert u.numel() == 65536 and torch.isfinite(u).all() and u.unique().numel() >= 65536 - 2048 - 1      # +0 == -0
    worst = {"fwd": ro.ratio(ro.emulate_gelu_fwd(u), *ro.gelu_fwd_f64(u))}
    for name in DH_PATTERNS:
        dh = dh_pattern(name)
        assert torch.isfinite(ro.gelu_bwd_f64(u, dh)[0].half()).all()
        worst["bwd/" + name] = ro.ratio(ro.emulate_gelu_bwd(u, dh), *ro.gelu_bwd_f64(u, dh))
    x = u.float()
    worst["grad"] = ro.ratio(ro.emulate_gelu_grad(x), ro.gelu_grad_f64(x.double()), ro.SECOND * ro.gelu_grad_err(x.double()))
    _print("gelu every finite fp16", worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    far = x.abs() >= 16.0                                     # the exact tails
    assert torch.equal(ro.emulate_gelu_fwd(u)[far].float(), x[far].clamp_min(0.0))
    assert torch.equal(ro.emulate_gelu_grad(x)[far], (x[far] > 0).float())


MAT_FAMILIES = ro.MAT_FAMILIES
matrix = functools.lru_cache(maxsize=None)(ro.make_matrix)


@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=str)
def test_colsum_emulation_within_bounds(shape):
    m, n = shape
    want = {1: (1, 1), 7: (1, 7), 13: (1, 13), 513: (2, 257), 1025: (3, 342), 131073: (256, 513)}[m]
    assert (ro.colsum_chunks(m), ro.cdiv(m, ro.colsum_chunks(m))) == want
    worst = {}
    for fam in MAT_FAMILIES:
        x, old = matrix(fam, m, n)
        for acc in (0, 1):
            worst[f"{fam}/acc{acc}"] = ro.ratio(ro.emulate_colsum(x, old, acc), *ro.colsum_f64(x, old, acc))
    _print(f"colsum {shape}", worst)
    assert all(v <= 1.0 for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------
# (b) mistakes, applied to the float64 reference
# ---------------------------------------------------------------------------------------------------------------
def forward_mistakes(p, d, t=6):
    """name -> [(mistaken output, reference, bound)] over the outputs the mistake reaches"""
    x, ga, be = p["x"], p["gamma"], p["beta"]
    xd = x.double()
    rows = x.shape[0]
    tok = x.view(rows // t, t, d)
    st = ro.Stats(x)
    grp, padded = ro.groups(d), 256 * ro.nv_of(d)
    ln_ref = ro.layernorm_f64(x, ga, be)
    cls_ref = {l2: ro.cls_head_f64(tok, ga, be, l2=l2) for l2 in (0, 1)}
    pm_ref = ro.patch_mean_f64(tok, ga, be)

    def l2n(y):
        return y / y.norm(dim=1, keepdim=True).clamp_min(1e-12)

    def everywhere(y):
        """a mistaken [rows, d] float64 LayerNorm output, carried to all four outputs"""
        yt = y.view(rows // t, t, d)
        return [(y,) + ln_ref, (yt[:, 0],) + cls_ref[0][:2], (l2n(yt[:, 0]),) + cls_ref[1][:2],
                (yt[:, 1:].mean(1),) + pm_ref]

    out = {}
    rs = lambda var, eps=ro.LN_EPS: (var + eps).rsqrt()
    out["unbiased variance"] = everywhere(ro.ln_apply(x, st.mean, rs(st.var * d / max(d - 1, 1)), ga, be))
    out["eps 1e-5 in place of 1e-6"] = everywhere(ro.ln_apply(x, st.mean, rs(st.var, 1e-5), ga, be))
    mp = xd.sum(1, keepdim=True) / padded
    out["mean and variance over the padded width 256 NV"] = everywhere(
        ro.ln_apply(x, mp, rs(((xd - mp) ** 2).sum(1, keepdim=True) / padded), ga, be))
    if grp > 1:
        head = xd[:, :256 * (grp - 1)]
        mh = head.sum(1, keepdim=True) / d
        out["the last column group left out of the statistics"] = everywhere(
            ro.ln_apply(x, mh, rs(((head - mh) ** 2).sum(1, keepdim=True) / d), ga, be))
        out["gamma / beta read one column group off"] = everywhere(
            ro.ln_apply(x, st.mean, st.rstd, ga.roll(-256), be.roll(-256)))
    out["the normalised value rounded to fp16 before the affine"] = everywhere(
        st.xhat.half().double() * ga.double() + be.double())
    y = ro.ln_apply(x, st.mean, st.rstd, ga, be).view(rows // t, t, d)
    out["token 1 read in place of token 0"] = [(y[:, 1],) + cls_ref[0][:2], (l2n(y[:, 1]),) + cls_ref[1][:2]]
    xh0 = st.xhat.view(rows // t, t, d)[:, 0]
    out["the L2 norm taken before the affine"] = [(y[:, 0] / xh0.norm(dim=1, keepdim=True),) + cls_ref[1][:2]]
    out["patch mean including the class token"] = [(ro.patch_mean_f64(tok, ga, be, first=0)[0],) + pm_ref]
    out["patch mean dividing by t"] = [(ro.patch_mean_f64(tok, ga, be, div=t)[0],) + pm_ref]
    keep = [i for i in range(1, t) if (i - 1) % 4 != 1]
    out["patch mean losing the rows of one wave"] = [(ro.patch_mean_f64(tok, ga, be, rows=keep)[0],) + pm_ref]
    return out


def backward_mistakes(p, rows):
    x, dy, ga, dres_in = p["x"][:rows], p["dy"][:rows], p["gamma"], p["dres_in"][:rows]
    r = ro.layernorm_bwd_f64(x, dy, ga, dres_in=dres_in)
    st, g, mg, mgx, xh, dyd = r["st"], r["g"], r["mg"], r["mgx"], r["xh"], dy.double()
    rin = dres_in.double()
    blocks = ro.ln_bwd_blocks(rows)
    idx = torch.arange(rows)
    wave_rows = lambda blk, w: idx[(idx % (4 * blocks)) == 4 * blk + w]
    out = {}
    out["the xhat mean(g xhat) term dropped"] = [(st.rstd * (g - mg) + rin,) + r["dres"]]
    out["mean(dy) in place of mean(dy gamma)"] = [(st.rstd * (g - dyd.mean(1, keepdim=True) - xh * mgx) + rin,) + r["dres"]]
    out["dgamma built from g, not from dy"] = [((g * xh).sum(0),) + r["dgamma"]]

    def without(drop):
        keep = torch.ones(rows, dtype=torch.bool)
        keep[drop] = False
        return [((dyd * xh)[keep].sum(0),) + r["dgamma"], (dyd[keep].sum(0),) + r["dbeta"]]

    out["the last row of a wave missing from dgamma / dbeta"] = without(wave_rows(0, 0)[-1:])
    out["one wave's partial missing"] = without(wave_rows(0, min(1, rows - 1)))
    out["one workgroup's partial missing"] = without(idx[(idx % (4 * blocks)) // 4 == blocks - 1])
    out["dres_in not added"] = [(r["dx"],) + r["dres"]]
    stored = r["dres"][0].float().half()
    out["dres_colsum of the fp32 values, not of the stored fp16"] = [(r["dres"][0].sum(0),) + ro.dres_colsum_f64(stored)]
    return out


def gelu_mistakes():
    u = ro.all_finite_f16()
    x = u.double()
    fwd = ro.gelu_fwd_f64(u)
    out = {"the tanh form": [(ro.gelu_tanh_f64(x),) + fwd]}
    flush = lambda v: torch.where(v.abs() < 2.0 ** -14, torch.zeros_like(v), v)
    out["tails flushed to zero below |g| < 2^-14"] = [(flush(fwd[0]),) + fwd]
    q = 0.5 * torch.special.erfc(x.abs() * ro.SQRT1_2)
    wrong = torch.where(x > 0, 1.0 - q, -q) + x * torch.exp(-0.5 * x * x) * ro.INV_SQRT_2PI
    for name in DH_PATTERNS:
        dh = dh_pattern(name)
        bwd = ro.gelu_bwd_f64(u, dh)
        out["tails flushed to zero below |g| < 2^-14"].append((flush(bwd[0]),) + bwd)
        out.setdefault("the gradient's cdf select by x > 0 with q mis-signed", []).append((dh.double() * wrong,) + bwd)
    return out


def colsum_mistakes(fam, m, n):
    x, old = matrix(fam, m, n)
    chunks = ro.colsum_chunks(m)
    rows_per = ro.cdiv(m, chunks)
    ref0, ref1 = ro.colsum_f64(x), ro.colsum_f64(x, old, 1)
    idx = torch.arange(m)
    return {"the last row chunk dropped": [(ro.colsum_f64(x, rows=idx[idx < (chunks - 1) * rows_per])[0],) + ref0],
            "the rows r % 8 == 7 dropped": [(ro.colsum_f64(x, rows=idx[(idx % rows_per) % 8 != 7])[0],) + ref0],
            "accumulate ignoring the old value": [(ref0[0],) + ref1]}


def _factor(triples):
    return max(ro.ratio(mut, ref, bound) for mut, ref, bound in triples)


def _table(title, rows):
    print(f"\n{title}")
    for name, per in rows.items():
        print(f"rowops-mut  {name:58s} " + "  ".join(f"{fam} {val:.3g}" for fam, val in per.items()) +
              (f"   BELOW THE 10x BAR (best {max(per.values()):.3g})" if name in BELOW_BAR else ""))


def _check(rows):
    assert all(max(per.values()) >= 10.0 for name, per in rows.items() if name not in BELOW_BAR), rows
    assert all(max(rows[name].values()) > 1.0 for name in BELOW_BAR if name in rows), rows


@pytest.mark.parametrize("d", [260, 1028])
def test_forward_mistakes_exceed_bounds_tenfold(d):
    rows = {}
    for fam in ro.FAMILIES:
        for name, triples in forward_mistakes(problem(fam, ROWS, d, "f32", CANCEL), d).items():
            rows.setdefault(name, {})[fam] = _factor(triples)
    _table(f"LayerNorm forward / CLS head / patch mean mistakes, max err / bound, d {d}", rows)
    assert len(rows) == 11
    _check(rows)


@pytest.mark.parametrize("n_rows", [5, 65])
def test_backward_mistakes_exceed_bounds_tenfold(n_rows):
    rows = {}
    for fam in ro.FAMILIES:
        for name, triples in backward_mistakes(problem(fam, 65, 260, "f32", 2), n_rows).items():
            rows.setdefault(name, {})[fam] = _factor(triples)
    _table(f"LayerNorm backward mistakes, max err / bound, d 260 rows {n_rows}", rows)
    assert len(rows) == 8
    _check(rows)


def test_gelu_mistakes_exceed_bounds_tenfold():
    rows = {name: {"every fp16": _factor(triples)} for name, triples in gelu_mistakes().items()}
    _table("GELU mistakes, max err / bound over every finite fp16 value", rows)
    assert len(rows) == 3
    _check(rows)


@pytest.mark.parametrize("shape", [(13, 264), (1025, 256), (131073, 8)], ids=str)
def test_colsum_mistakes_exceed_bounds_tenfold(shape):
    rows = {}
    for fam in MAT_FAMILIES:
        for name, triples in colsum_mistakes(fam, *shape).items():
            rows.setdefault(name, {})[fam] = _factor(triples)
    _table(f"column-sum mistakes, max err / bound, {shape}", rows)
    _check(rows)


def test_reference_pieces_are_consistent():
    """the float64 pieces against torch's own float64 LayerNorm / GELU autograd; the marker family's single products;
    the dispatch tables against the widths the tests name."""
    F = torch.nn.functional
    p = problem("plain", 65, 260, "f32", 2)
    x = p["x"].double().requires_grad_(True)
    ga = p["gamma"].double().requires_grad_(True)
    be = p["beta"].double().requires_grad_(True)
    y = F.layer_norm(x, (260,), ga, be, ro.LN_EPS)
    assert (y.detach() - ro.layernorm_f64(p["x"], p["gamma"], p["beta"])[0]).abs().max() <= 1e-12
    y.backward(p["dy"].double())
    r = ro.layernorm_bwd_f64(p["x"], p["dy"], p["gamma"])
    assert (x.grad - r["dres"][0]).abs().max() <= 1e-11
    assert (ga.grad - r["dgamma"][0]).abs().max() <= 1e-11 and (be.grad - r["dbeta"][0]).abs().max() <= 1e-12
    v = torch.linspace(-8, 8, 3201, dtype=torch.float64)
    assert (torch.autograd.functional.jacobian(ro.gelu_f64, v).diagonal() - ro.gelu_grad_f64(v)).abs().max() <= 1e-14
    m = problem("marker", 65, 260, "f32", 2)
    nz = m["dy"].double() != 0
    assert (nz.sum(0) <= 1).all() and (nz.sum(1) == 1).all() and ((m["x"] != 0).sum(1) == 1).all()
    rm = ro.layernorm_bwd_f64(m["x"], m["dy"], m["gamma"])
    assert torch.equal(rm["dbeta"][0], m["dy"].double().sum(0)) and (rm["dbeta"][0] != 0).sum() == 65
    cols = nz.double().argmax(1)                                  # the one dy column of each row
    assert torch.equal(rm["dgamma"][0][cols], (m["dy"].double() * rm["xh"])[torch.arange(65), cols])
    assert [ro.nv_of(d) for d in FWD_D] == [2, 2, 3, 4, 5, 5, 8, 8]
    assert [ro.nj_of(d) for d in BWD_D] == [1, 1, 2, 3, 4, 8, 8, 16, 16]
    assert ro.ln_bwd_blocks(65) == 2 and ro.ln_bwd_blocks(5) == 1 and ro.ln_bwd_blocks(65606) == 1024
    for fam in ro.FAMILIES:
        c = problem(fam, ROWS, 260, "f32", CANCEL)
        assert not torch.equal(c["x"], c["x"].flip(0)) and not torch.equal(c["gamma"], c["gamma"].flip(0))
    c = problem("cancel", ROWS, 260, "f32", CANCEL)
    y = ro.layernorm_f64(c["x"], c["gamma"], c["beta"])[0]
    assert y[CANCEL].abs().max() <= 1e-6 and y[CANCEL + 1].abs().max() > 0.1
