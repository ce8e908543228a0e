"""GPU: every element of every GEMM kernel's outputs against oracle.gemm's float64 reference, through the per-element
bounds derived there (err / bound <= 1; tests/test_gemm_host.py shows the bounds are honest and sharp).

Every case: the route (128 x 128 kernel, 128 x 192 kernel, 256 x 256 kernel, tail split) is ASKED of the library
(hcir_gemm_route) and asserted, with the number of 256 x 256 tiles against the 256 workgroups where that matters, so
that a changed dispatch threshold fails here instead of silently moving a shape to another kernel.  Every output
element is compared (a non-finite value is an infinite error); outputs that are not read are prefilled with NaN; pad
columns (ldo > n) and three rows past m hold a pattern that must come back bit-equal.  Operands and their float64 S
and A are made once per (shape, family).  K = 192 on the persistent routes: three k-steps, both LDS slots reused.
hcir_gemm_f16_gelu_dual stays on the 256 x 256 kernel at every shape (gemm_plan.h): the query says so and the test
asserts it, at the shapes that send the other epilogues to the 128 x 192 kernel and to the split.

The worst err / bound per (route, epilogue, family) is printed at the end of the module (profiles/gemm_bounds.txt).
On an MI355X (no bound was changed after the first GPU run): fp16 outputs 0.985 - 0.996 on every route (the bound is
little more than the store's half ulp, which a correctly rounded store reaches); fp32 outputs 0.92 - 0.99 on marker rows
(a single product: the bound is the one rounding of the bias add) and 0.01 - 0.03 otherwise; slice mean 0.09, slice
M2 0.31, combined mean 0.27 and rstd 0.20; hcir_gemm_f16_tn 0.04.
"""
import pytest
import torch

from oracle import gemm as og

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
NAN = float("nan")
EXTRA_ROWS = 3
WORST = {}

# name -> ((m, n, k), route, tiles of 256 x 256 per workgroup: None (not that kernel), "one", "two")
SHAPES = {
    "small-5x8x8": ((5, 8, 8), og.ROUTE_SMALL, None),
    "small-129x136x72": ((129, 136, 72), og.ROUTE_SMALL, None),
    "small-1x128x120": ((1, 128, 120), og.ROUTE_SMALL, None),
    "small-1100x384x192": ((1100, 384, 192), og.ROUTE_SMALL, None),      # m >= 1024 but n % 256 != 0
    "mid-1030x256x192": ((1030, 256, 192), og.ROUTE_MID, None),          # 6 row tiles of 192, the last ragged  
    "big1-11517x1024x192": ((11517, 1024, 192), og.ROUTE_BIG, "one"),    # 180 tiles
    "big2-25381x1024x192": ((25381, 1024, 192), og.ROUTE_BIG, "two"),    # 400 tiles; last wave tiles wholly past m
    "split-17923x1024x192": ((17923, 1024, 192), og.ROUTE_SPLIT, "one"),  # 256 tiles + 1539 rows on 128 x 192
}
PERSISTENT = [s for s in SHAPES if not s.startswith("small")]
# (kind, with scale)
VARIANTS = [("bias_f16", False), ("gelu_f16", False), ("resid_f32", True), ("resid_f32", False), ("bias_f32", False),
            ("affine_relu_f16", True), ("affine_f32", True), ("resid_f16", True), ("resid_f16", False)]
FUSED = ("dual", "ln_bias_f16", "ln_gelu_f16", "stats")


def families_of(kind):
    fams = ["plain", "marker"]
    if kind in ("gelu_f16", "dual", "ln_gelu_f16"):
        fams.append("tail")
    if kind in ("bias_f16", "bias_f32", "gelu_f16", "dual"):
        fams.append("cancel")
    if kind in ("ln_bias_f16", "ln_gelu_f16", "stats"):
        fams.append("offset")
    return fams


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\ngemm worst err / bound per route, epilogue and family:")
    for key, val in sorted(WORST.items()):
        print("gemm-worst " + " ".join(f"{k:20s}" for k in key) + f" {val:.3f}")


@pytest.fixture(scope="module")
def problems():
    """(shape name, family) -> operands on the device with their float64 S and A, made on first use"""
    cache = {}

    def get(shape, family):
        if (shape, family) not in cache:
            m, n, k = SHAPES[shape][0]
            p = {key: v.cuda() for key, v in og.make_problem(family, m, n, k).items()}
            p["acc"] = og.acc_f64(p["a"], p["w"])
            p["m"], p["n"], p["k"] = m, n, k
            cache[(shape, family)] = p
        return cache[(shape, family)]
    return get


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _note(shape, kind, family, ratios):
    for name, val in ratios.items():
        key = (shape.split("-")[0], kind, name, family)
        WORST[key] = max(WORST.get(key, 0.0), val)
    print(f"\ngemm-err {shape} {kind} {family}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def assert_route(L, shape, epi):
    """The library's own answer for this shape and epilogue; the 256 x 256 tile count against the 256 workgroups."""
    (m, n, k), want, per_wg = SHAPES[shape]
    if epi == og.ROUTE_EPI_DUAL and want != og.ROUTE_SMALL:
        want = og.ROUTE_BIG
    rows = torch.full((1,), -1, dtype=torch.int64)
    assert L.hcir_gemm_route(m, n, k, epi, rows.data_ptr()) == want, (shape, epi)
    m1 = int(rows[0])
    tiles = -(-n // 256) * -(-m // 256)
    if want == og.ROUTE_BIG:
        assert m1 == m
        if epi != og.ROUTE_EPI_DUAL:
            assert (tiles <= 256) == (per_wg == "one") and tiles <= 512, (shape, tiles)
    elif want == og.ROUTE_SPLIT:
        assert 0 < m1 < m and m1 % 256 == 0 and (m1 // 256) * (n // 256) == 256, (shape, m1)
        assert m - m1 == 1539
    else:
        assert m1 == 0
    return m1


class Out:
    """[m + 3, ld] buffer: a pattern everywhere, then NaN (or `init`) in [:m, :n]; check() wants the pattern back."""

    def __init__(self, m, n, ld, dtype, init=None):
        numel = (m + EXTRA_ROWS) * ld
        self.buf = ((torch.arange(numel, device="cuda") % 251) - 125).to(dtype).view(m + EXTRA_ROWS, ld)
        self.t = self.buf[:m, :n]
        self.t[...] = NAN if init is None else init
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr()

    def check(self):
        m, n = self.t.shape
        assert torch.equal(self.buf[:m, n:], self.before[:m, n:]), "pad columns written"
        assert torch.equal(self.buf[m:], self.before[m:]), "rows past m written"
        return self.t

    def untouched(self):
        as_int = torch.int32 if self.buf.dtype == torch.float32 else torch.int16
        return torch.equal(self.buf.view(as_int), self.before.view(as_int))


def pitched(t, ld):
    """a copy of t [r, c] with row pitch ld, the pad columns holding 77 (finite: a read of them is a wrong value)"""
    buf = torch.full((t.shape[0], ld), 77.0, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def run_epilogue(L, p, kind, scaled, pad=False, resid_separate=False):
    """One launch of hcir_gemm_f16 / _resid / _gelu_dual / _fused -> {output name: err / bound}, every element."""
    m, n, k = p["m"], p["n"], p["k"]
    lda, ldw, ldo = (k + 64, k + 8, n + 8) if pad else (k, k, n)
    a, w = (pitched(p["a"], lda), pitched(p["w"], ldw)) if pad else (p["a"], p["w"])
    f32 = kind in og.F32_KINDS
    dt = torch.float32 if f32 else torch.float16
    is_resid = kind in ("resid_f32", "resid_f16", "stats")
    resid = p["resid"].to(dt) if is_resid else None
    scale = p["scale"] if scaled else None
    out = Out(m, n, ldo, dt, None if (not is_resid or resid_separate) else resid)
    rbuf = Out(m, n, ldo, dt, resid) if resid_separate else None
    ratios = {}
    if kind == "dual":
        out2 = Out(m, n, ldo, dt)
        assert L.hcir_gemm_f16_gelu_dual(a.data_ptr(), lda, w.data_ptr(), ldw, p["bias"].data_ptr(), m, n, k, out.ptr(),
                                         out2.ptr(), ldo, _st()) == 0
        refs = og.epilogue_f64("dual", p["acc"], bias=p["bias"])
        ratios = {"pre": og.ratio(out.check(), *refs[0]), "act": og.ratio(out2.check(), *refs[1])}
    elif kind in ("ln_bias_f16", "ln_gelu_f16"):
        assert L.hcir_gemm_f16_fused(a.data_ptr(), lda, w.data_ptr(), ldw, p["bias"].data_ptr(), None, m, n, k,
                                     0 if kind == "ln_bias_f16" else 1, out.ptr(), ldo, p["stats"].data_ptr(),
                                     p["c1"].data_ptr(), None, _st()) == 0
        (ref, bound), = og.epilogue_f64(kind, p["acc"], bias=p["bias"], stats=p["stats"], c1=p["c1"])
        ratios = {"out": og.ratio(out.check(), ref, bound)}
    elif kind == "stats":
        nsl = L.hcir_gemm_stats_slices(n)
        assert nsl == n // 64
        part = Out(nsl * m, 2, 2, torch.float32)
        stats = Out(m, 2, 2, torch.float32)
        assert L.hcir_gemm_f16_fused(a.data_ptr(), lda, w.data_ptr(), ldw, p["bias"].data_ptr(), _ptr(scale), m, n, k, 6,
                                     out.ptr(), ldo, None, None, part.ptr(), _st()) == 0
        assert L.hcir_ln_stats_finalize(part.ptr(), nsl, m, n, og.LN_EPS, stats.ptr(), _st()) == 0
        (ref, bound), = og.epilogue_f64("resid_f16", p["acc"], bias=p["bias"], scale=scale, resid=resid)
        rows = out.check()
        sl = part.check().view(nsl, m, 2)
        st = stats.check()
        # the statistics are those of the fp16 rows the kernel stored
        mean_p, m2_p, d_mean_p, d_m2_p = og.slice_stats_f64(rows)
        mean, rstd, d_mean, d_rstd = og.finalize_f64(mean_p, m2_p, og.LN_EPS, d_mean_p, d_m2_p)
        given = og.finalize_f64(sl[..., 0], sl[..., 1], og.LN_EPS)       # hcir_ln_stats_finalize on the producer's slices
        ratios = {"out": og.ratio(rows, ref, bound), "slice_mean": og.ratio(sl[..., 0], mean_p, d_mean_p),
                  "slice_m2": og.ratio(sl[..., 1], m2_p, d_m2_p), "mean": og.ratio(st[:, 0], mean, d_mean),
                  "rstd": og.ratio(st[:, 1], rstd, d_rstd), "fin_mean": og.ratio(st[:, 0], given[0], given[2]),
                  "fin_rstd": og.ratio(st[:, 1], given[1], given[3])}
    else:
        args = (a.data_ptr(), lda, w.data_ptr(), ldw, p["bias"].data_ptr(), _ptr(scale), m, n, k, og.EPI[kind])
        if resid_separate:
            assert L.hcir_gemm_f16_resid(*args, rbuf.ptr(), out.ptr(), ldo, _st()) == 0
        else:
            assert L.hcir_gemm_f16(*args, out.ptr(), ldo, _st()) == 0
        (ref, bound), = og.epilogue_f64(kind, p["acc"], bias=p["bias"], scale=scale, resid=resid)
        ratios = {"out": og.ratio(out.check(), ref, bound)}
    if rbuf is not None:
        assert rbuf.untouched(), "resid changed"
    return ratios


def _label(kind, scaled, extra=""):
    return kind + ("+scale" if scaled and kind.startswith("resid") else "") + extra


# ---------------------------------------------------------------------------------------------------------------
# hcir_gemm_f16: every epilogue on every route
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,scaled", VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_epilogues_on_every_route(L, problems, shape, kind, scaled):
    assert_route(L, shape, og.EPI[kind])
    for family in families_of(kind):
        r = run_epilogue(L, problems(shape, family), kind, scaled)
        _note(shape, _label(kind, scaled), family, r)
        assert all(v <= 1.0 for v in r.values()), (shape, kind, family, r)


@pytest.mark.parametrize("kind", FUSED)
@pytest.mark.parametrize("shape", PERSISTENT)
def test_fused_epilogues_on_persistent_routes(L, problems, shape, kind):
    """dual output, both LayerNorm-fold epilogues and the statistics producer (with hcir_ln_stats_finalize behind it):
    on the split the slices and the fold's (mean, rstd) of the rows behind rows_on_big are compared like all others."""
    assert_route(L, shape, {"dual": og.ROUTE_EPI_DUAL, "ln_bias_f16": 0, "ln_gelu_f16": 1, "stats": 6}[kind])
    for family in families_of(kind):
        r = run_epilogue(L, problems(shape, family), kind, scaled=(kind == "stats" and family == "plain"))
        _note(shape, kind, family, r)
        assert all(v <= 1.0 for v in r.values()), (shape, kind, family, r)


def test_fused_epilogues_refused_on_small(L, problems):
    p = problems("small-1100x384x192", "plain")
    m, n, k = p["m"], p["n"], p["k"]
    assert_route(L, "small-1100x384x192", og.ROUTE_EPI_DUAL)
    assert L.hcir_gemm_fused_supported(m, n, k) == 0
    out, out2 = Out(m, n, n, torch.float16), Out(m, n, n, torch.float16)
    part = Out(n // 64 * m, 2, 2, torch.float32)
    a, w, b = p["a"].data_ptr(), p["w"].data_ptr(), p["bias"].data_ptr()
    assert L.hcir_gemm_f16_gelu_dual(a, k, w, k, b, m, n, k, out.ptr(), out2.ptr(), n, _st()) == UNSUPPORTED
    for epi in (0, 1):
        assert L.hcir_gemm_f16_fused(a, k, w, k, b, None, m, n, k, epi, out.ptr(), n, p["stats"].data_ptr(),
                                     p["c1"].data_ptr(), None, _st()) == UNSUPPORTED
    assert L.hcir_gemm_f16_fused(a, k, w, k, b, None, m, n, k, 6, out.ptr(), n, None, None, part.ptr(), _st()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched() and out2.untouched() and part.untouched()       # nothing was launched


@pytest.mark.parametrize("kind,scaled", [("resid_f32", True), ("resid_f16", True), ("resid_f16", False)], ids=str)
@pytest.mark.parametrize("shape", ["big2-25381x1024x192", "split-17923x1024x192"])
def test_residual_out_of_place(L, problems, shape, kind, scaled):
    """hcir_gemm_f16_resid on the several-tiles route and on the split (the second launch reads resid behind
    rows_on_big): out = resid + ..., resid bit-unchanged, out's own NaN prefill never read."""
    assert_route(L, shape, og.EPI[kind])
    for family in ("plain", "marker"):
        r = run_epilogue(L, problems(shape, family), kind, scaled, resid_separate=True)
        _note(shape, _label(kind, scaled, "/resid"), family, r)
        assert all(v <= 1.0 for v in r.values()), (shape, kind, family, r)


@pytest.mark.parametrize("kind", ["bias_f16", "gelu_f16", "affine_relu_f16", "resid_f16", "bias_f32", "affine_f32",
                                  "resid_f32", "dual", "ln_bias_f16", "ln_gelu_f16", "stats"])
@pytest.mark.parametrize("shape", ["big2-25381x1024x192", "split-17923x1024x192"])
def test_row_pitches(L, problems, shape, kind):
    """lda = k + 64, ldw = k + 8, ldo = n + 8 for every epilogue class, fp16 and fp32 outputs, the fold, the dual and
    the statistics: the split advances A, out, resid by pitched rows."""
    epi = {"dual": og.ROUTE_EPI_DUAL, "ln_bias_f16": 0, "ln_gelu_f16": 1, "stats": 6}.get(kind)
    assert_route(L, shape, og.EPI[kind] if epi is None else epi)
    for family in ("plain", "marker"):
        r = run_epilogue(L, problems(shape, family), kind, scaled=kind in ("resid_f16", "resid_f32", "affine_relu_f16",
                                                                          "affine_f32"), pad=True)
        _note(shape, kind + "/pitched", family, r)
        assert all(v <= 1.0 for v in r.values()), (shape, kind, family, r)


def test_fp16_output_pitch_refused_on_persistent_routes(L, problems):
    """The persistent epilogue stores 16-byte pieces of a row: ldo % 8 != 0 is refused for fp16 outputs before any
    launch (the fused and dual calls always did)."""
    p = problems("mid-1030x256x192", "plain")
    m, n, k = p["m"], p["n"], p["k"]
    for epi, dt in ((0, torch.float16), (1, torch.float16), (4, torch.float16), (6, torch.float16)):
        out = Out(m, n, n + 4, dt, 0.5)
        assert L.hcir_gemm_f16_resid(p["a"].data_ptr(), k, p["w"].data_ptr(), k, p["bias"].data_ptr(),
                                     p["scale"].data_ptr(), m, n, k, epi, None, out.ptr(), n + 4, _st()) == INVALID
        torch.cuda.synchronize()
        assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------
# hcir_ln_stats_finalize alone, on slices of known float64 form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,parts", [(1, 1), (257, 4), (1000, 16), (300, 48)])
def test_ln_stats_finalize_alone(L, m, parts):
    """Slices written by the test (fp32 values, so their float64 form is known exactly): rows with |mean| >> spread,
    rows whose slices disagree strongly (the slice_n dm^2 term is most of the variance), zero M2."""
    g = torch.Generator().manual_seed(m + parts)
    mean_p = torch.randn(parts, m, generator=g) + 40.0 * (torch.arange(m) % 4 == 0) + \
        5.0 * torch.randn(parts, 1, generator=g) * (torch.arange(m) % 3 == 0)
    m2_p = torch.rand(parts, m, generator=g) * 64.0 * (torch.arange(m) % 5 != 0)
    part = torch.stack([mean_p, m2_p], -1).contiguous().cuda()
    stats = Out(m, 2, 2, torch.float32)
    assert L.hcir_ln_stats_finalize(part.data_ptr(), parts, m, 64 * parts, og.LN_EPS, stats.ptr(), _st()) == 0
    st = stats.check()
    mean, rstd, d_mean, d_rstd = og.finalize_f64(part[..., 0], part[..., 1], og.LN_EPS)
    r = {"mean": og.ratio(st[:, 0], mean, d_mean), "rstd": og.ratio(st[:, 1], rstd, d_rstd)}
    _note(f"finalize-{m}x{parts}", "finalize", "written", r)
    assert all(v <= 1.0 for v in r.values()), r
    assert L.hcir_ln_stats_finalize(part.data_ptr(), parts, m, 64 * parts + 8, og.LN_EPS, stats.ptr(), _st()) == INVALID


# ---------------------------------------------------------------------------------------------------------------
# hcir_gemm_f16_tn
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("shape", og.TN_SHAPES, ids=str)
def test_gemm_tn(L, shape, pad):
    """dW (+)= A^T B, every element, accumulate 0 and 1; the split count the bound assumes is the one the library's
    workspace size implies; lda > n, ldb > k, lddw > k with dW's pad columns untouched."""
    m, n, k = shape
    splits, rows = og.tn_plan(m, n, k)
    ws_bytes = L.hcir_gemm_f16_tn_workspace_bytes(m, n, k)
    assert ws_bytes == splits * n * k * 4, (ws_bytes, splits)
    tiles, steps = (n // 256) * (k // 256), m // 64
    want = {64: dict(splits=1), 100 * 64: dict(splits=100, rows=64), 301 * 64: dict(rows=128, last=64),
            256 * 64: dict(splits=256, rows=64), 64 * 64: dict(splits=64, rows=64), 130 * 64: dict(rows=192, last=64),
            128 * 64: dict(splits=64, rows=128)}[m]
    assert splits == want.get("splits", splits) and rows == want.get("rows", rows)
    assert m - (splits - 1) * rows == want.get("last", rows)
    if m in (256 * 64, 64 * 64, 128 * 64):
        assert tiles * splits == 256
    a, b, old = (t.cuda() for t in og.make_tn(m, n, k))
    lda, ldb, lddw = (n + 8, k + 8, k + 4) if pad else (n, k, k)
    ab, bb = (pitched(a, lda), pitched(b, ldb)) if pad else (a, b)
    ws = torch.full((ws_bytes // 4,), NAN, device="cuda")
    for accumulate in (0, 1):
        dw = Out(n, k, lddw, torch.float32, old if accumulate else None)
        assert L.hcir_gemm_f16_tn(ab.data_ptr(), lda, bb.data_ptr(), ldb, m, n, k, dw.ptr(), lddw, accumulate,
                                  ws.data_ptr(), ws_bytes, _st()) == 0
        ref, bound, _ = og.tn_f64(a, b, old, accumulate)
        r = {"dw": og.ratio(dw.check(), ref, bound)}
        _note(f"tn-{m}x{n}x{k}", f"tn/acc{accumulate}" + ("/pitched" if pad else ""), "plain", r)
        assert r["dw"] <= 1.0, (shape, accumulate, r)
    assert L.hcir_gemm_f16_tn(ab.data_ptr(), lda, bb.data_ptr(), ldb, m, n, k, dw.ptr(), lddw, 0, ws.data_ptr(),
                              ws_bytes - 4, _st()) == WORKSPACE
