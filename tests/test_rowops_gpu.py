"""GPU: every element of the row-wise ViT kernels' outputs against oracle.rowops's float64 references, through the
per-element bounds derived there (err / bound <= 1; tests/test_rowops_host.py shows the bounds are honest and sharp).

hcir_layernorm_f16, hcir_cls_head, hcir_patch_mean (csrc/norm.hip: NV 2, 3, 4, 5, 8), hcir_layernorm_bwd / _fused
(csrc/train.hip: NJ 1, 2, 3, 4, 8, 16), hcir_gelu_fwd_f16 / _bwd_f16 on every finite fp16 value, hcir_add_f32_f16 bit
for bit, hcir_colsum_f16 and hcir_gelu_bwd_colsum_f16, all through the C ABI so that every pitch and optional pointer
is passed.  Every case: each written buffer lies between canary rows, pad columns (ld > d) hold a pattern that must
come back bit-equal, outputs are prefilled with NaN (a non-finite value is an infinite error), and the case runs twice
with bit-equal results.  The two grid-stride cases assert the launch geometry they rely on
(hcir_layernorm_bwd_blocks(rows) == 1024; n > 8192 workgroups x the elements of one).

The worst err / bound per (kernel, family, shape) is printed at the end of the module (profiles/rowops_bounds.txt).
On an MI355X (no bound was changed after the first GPU run): fp16 outputs 0.98 - 1.00 (the bound is little more than
the store's half ulp) except on `constant` rows (0.68 - 0.86: the bound there is the error of the mean); fp32 CLS
embedding 0.08 - 0.74, row norms 0.08 - 0.71, patch mean 0.11 - 0.52; dres_out 0.15 - 0.91, dgamma 0.23 - 0.91, dbeta
0.16 - 0.94 (one row added to an old value: a single rounding), dres_colsum 0.03 - 0.06, column sums 0.01 - 0.17.
hcir_add_f32_f16 is bit-equal to the CPU's fp32 add and round-to-nearest-even conversion.
"""
import pytest
import torch

from oracle import rowops as ro
from oracle.attention import f32

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
NAN = float("nan")
CANARY = 2
EPS = f32(1e-6)
WORST = {}
DT = {"f32": torch.float32, "f16": torch.float16}
CODE = {torch.float32: ro.F32, torch.float16: ro.F16}
FWD_D = (4, 260, 768, 1024, 1028, 1280, 1284, 2048)
BWD_D = (4, 256, 260, 768, 1024, 1028, 2048, 2052, 4096)
COLSUM_SHAPES = {(1, 8): 1, (7, 8): 1, (13, 264): 1, (513, 8): 2, (1025, 256): 3, (131073, 8): 256}   # -> chunks


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\nrowops worst err / bound per kernel, family and shape:")
    for key, val in sorted(WORST.items()):
        print("rowops-worst " + " ".join(f"{k:18s}" for k in key) + f" {val:.3f}")


@pytest.fixture(scope="module")
def problems():
    """(family, rows, d, x dtype, cancel row) -> tensors on the device, made on first use"""
    cache = {}

    def get(family, rows, d, xdt, cancel_row=None):
        key = (family, rows, d, xdt, cancel_row)
        if key not in cache:
            p = ro.make_problem(family, rows, d, cancel_row=cancel_row)
            p["x"] = p["x"].to(DT[xdt])
            if family == "cancel":
                p = ro.apply_cancel(p, p["x"])
            cache[key] = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in p.items()}
        return cache[key]
    return get


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _note(kernel, family, shape, ratios):
    for name, val in ratios.items():
        key = (kernel, name, family, shape)
        WORST[key] = max(WORST.get(key, 0.0), val)
    assert all(v <= 1.0 for v in ratios.values()), (kernel, family, shape, ratios)


class Buf:
    """[CANARY + rows + CANARY, ld] buffer: a pattern everywhere, then NaN (or `init`) in the live [rows, cols];
    check() wants the canary rows and the pad columns back bit-equal."""

    def __init__(self, rows, cols, ld, dtype, init=None):
        assert ld >= cols
        total = (rows + 2 * CANARY) * ld
        self.buf = ((torch.arange(total, device="cuda") % 251) - 125).to(dtype).view(rows + 2 * CANARY, ld)
        self.t = self.buf[CANARY:CANARY + rows, :cols]
        self.t[...] = NAN if init is None else init
        self.before = self.buf.clone()

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        rows, cols = self.t.shape
        live = slice(CANARY, CANARY + rows)
        assert torch.equal(self.buf[live, cols:], self.before[live, cols:]), "pad columns written"
        assert torch.equal(self.buf[:CANARY], self.before[:CANARY]), "rows before the buffer written"
        assert torch.equal(self.buf[CANARY + rows:], self.before[CANARY + rows:]), "rows past the buffer written"
        return self.t

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def vec(n, init=None):
    return Buf(1, n, n, torch.float32, init)


def pitched(t, ld):
    """a copy of t [r, c] with row pitch ld, the pad columns holding 77 (finite: a read of them is a wrong value)"""
    if ld == t.shape[1]:
        return t.contiguous()
    buf = torch.full((t.shape[0], ld), 77.0, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def twice(run):
    """run() -> tuple of output tensors; two runs, bit-equal"""
    a = run()
    b = run()
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v)), "two runs differ"
    return a


# ---------------------------------------------------------------------------------------------------------------
# hcir_layernorm_f16
# ---------------------------------------------------------------------------------------------------------------
def run_layernorm(L, x, ga, be, ldx=None, ldy=None):
    rows, d = x.shape
    ldx, ldy = ldx or d, ldy or d
    xb = pitched(x, ldx)
    y = Buf(rows, d, ldy, torch.float16)
    assert L.hcir_layernorm_f16(xb.data_ptr(), CODE[x.dtype], rows, d, ldx, ga.data_ptr(), be.data_ptr(), EPS, y.ptr(),
                                ldy, _st()) == 0
    return (y.check().clone(),)


@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", FWD_D, ids=lambda d: f"NV{ro.nv_of(d)}-d{d}")
def test_layernorm_forward(L, problems, d, xdt):
    for family in ro.FAMILIES:
        p = problems(family, 5, d, xdt, 2)
        for rows in (1, 5):                           # one live wave in the last (second) workgroup
            x = p["x"][:rows]
            y, = twice(lambda: run_layernorm(L, x, p["gamma"], p["beta"]))
            ref = ro.layernorm_f64(x, p["gamma"], p["beta"], EPS)
            _note("layernorm_f16", family, f"d{d}-{xdt}", {"y": ro.ratio(y, *ref)})


@pytest.mark.parametrize("xdt", list(DT))
def test_layernorm_forward_pitched(L, problems, xdt):
    d = 1028
    for family in ("plain", "marker"):
        p = problems(family, 5, d, xdt, 2)
        y, = twice(lambda: run_layernorm(L, p["x"], p["gamma"], p["beta"], ldx=d + 8, ldy=d + 4))
        ref = ro.layernorm_f64(p["x"], p["gamma"], p["beta"], EPS)
        _note("layernorm_f16", family, f"d{d}-{xdt}-pitched", {"y": ro.ratio(y, *ref)})


# ---------------------------------------------------------------------------------------------------------------
# hcir_cls_head
# ---------------------------------------------------------------------------------------------------------------
def run_cls_head(L, tok, ga, be, l2, want32, want16):
    b, t, d = tok.shape
    e32 = Buf(b, d, d, torch.float32) if want32 else None
    e16 = Buf(b, d, d, torch.float16) if want16 else None
    assert L.hcir_cls_head(tok.data_ptr(), CODE[tok.dtype], b, t, d, _ptr(ga), _ptr(be), EPS, l2,
                           e32.ptr() if e32 else None, e16.ptr() if e16 else None, _st()) == 0
    return tuple(o.check().clone() for o in (e32, e16) if o is not None)


@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", FWD_D, ids=lambda d: f"NV{ro.nv_of(d)}-d{d}")
def test_cls_head(L, problems, d, xdt):
    b, t = 5, 3
    for family in ro.FAMILIES:
        p = problems(family, b * t, d, xdt, 6)       # row 6: the class token of image 2
        tok = p["x"].view(b, t, d)
        for with_ln in (True, False):
            ga, be = (p["gamma"], p["beta"]) if with_ln else (None, None)
            for l2 in (0, 1):
                ref, b32, b16 = ro.cls_head_f64(tok, ga, be, EPS, l2)
                name = ("ln" if with_ln else "raw") + ("+l2" if l2 else "")
                for want32, want16 in ((True, True), (True, False), (False, True)):
                    outs = list(twice(lambda: run_cls_head(L, tok, ga, be, l2, want32, want16)))
                    r = {}
                    if want32:
                        o = outs.pop(0)
                        r[name + "/f32"] = ro.ratio(o, ref, b32)
                        if l2:
                            r[name + "/norm32"] = float(((o.double().norm(dim=1) - 1).abs() / ro.norm_bound(d, False)).max())
                        if not with_ln and not l2:
                            assert torch.equal(o, tok[:, 0].float())
                    if want16:
                        o = outs.pop(0)
                        r[name + "/f16"] = ro.ratio(o, ref, b16)
                        if l2:
                            r[name + "/norm16"] = float(((o.double().norm(dim=1) - 1).abs() / ro.norm_bound(d, True)).max())
                    _note("cls_head", family, f"d{d}-{xdt}", r)


# ---------------------------------------------------------------------------------------------------------------
# hcir_patch_mean
# ---------------------------------------------------------------------------------------------------------------
def run_patch_mean(L, tok, ga, be):
    b, t, d = tok.shape
    out = Buf(b, d, d, torch.float32)
    assert L.hcir_patch_mean(tok.data_ptr(), CODE[tok.dtype], b, t, d, _ptr(ga), _ptr(be), EPS, out.ptr(), _st()) == 0
    return (out.check().clone(),)


@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", (4, 768, 1024, 1028, 2048), ids=lambda d: f"NV{ro.nv_of(d)}-d{d}")
@pytest.mark.parametrize("t", (2, 3, 6))     # one, two and five patch rows: at 2 and 3 some of the four waves own no row
def test_patch_mean(L, problems, t, d, xdt):
    b = 3
    for family in ro.FAMILIES:
        p = problems(family, b * t, d, xdt, 1)
        tok = p["x"].view(b, t, d)
        for with_ln in (True, False):
            ga, be = (p["gamma"], p["beta"]) if with_ln else (None, None)
            o, = twice(lambda: run_patch_mean(L, tok, ga, be))
            _note("patch_mean", family, f"t{t}-d{d}-{xdt}",
                  {"ln" if with_ln else "raw": ro.ratio(o, *ro.patch_mean_f64(tok, ga, be, EPS))})


# ---------------------------------------------------------------------------------------------------------------
# hcir_layernorm_bwd / hcir_layernorm_bwd_fused
# ---------------------------------------------------------------------------------------------------------------
def run_ln_bwd(L, p, rows, accumulate, dres, mode, pitch=False):
    """dres: "none", "sep" (a separate dres_in) or "alias" (dres_in == dres_out); mode: "plain" (hcir_layernorm_bwd),
    "copy" (fused with dres_f16) or "colsum" (fused with dres_f16 and dres_colsum).  -> (ratios, outputs)"""
    x, dy, ga = p["x"][:rows], p["dy"][:rows], p["gamma"]
    d = x.shape[1]
    ldx, lddy, ldr, ldh = (d + 8, d + 4, d + 4, d + 12) if pitch else (d, d, d, d)
    xb, dyb = pitched(x, ldx), pitched(dy, lddy)
    dres_in = None if dres == "none" else p["dres_in"][:rows]
    old = (p["old_dgamma"], p["old_dbeta"])
    out = Buf(rows, d, ldr, torch.float32, dres_in if dres == "alias" else None)
    rin = Buf(rows, d, ldr, torch.float32, dres_in) if dres == "sep" else None
    rin_ptr = out.ptr() if dres == "alias" else (rin.ptr() if rin else None)
    dg, db = vec(d, old[0] if accumulate else None), vec(d, old[1] if accumulate else None)
    h16 = Buf(rows, d, ldh, torch.float16) if mode != "plain" else None
    cs = vec(d, 5.0 if accumulate else None) if mode == "colsum" else None       # assigned, never accumulated
    blocks = L.hcir_layernorm_bwd_blocks(rows)
    assert blocks == ro.ln_bwd_blocks(rows)
    ws = torch.full((blocks * d * (3 if cs else 2),), NAN, device="cuda")
    head = (xb.data_ptr(), CODE[x.dtype], rows, d, ldx, dyb.data_ptr(), lddy, ga.data_ptr(), EPS, rin_ptr, out.ptr(), ldr,
            dg.ptr(), db.ptr(), accumulate)
    if mode == "plain":
        assert L.hcir_layernorm_bwd(*head, ws.data_ptr(), ws.numel() * 4, _st()) == 0
    else:
        assert L.hcir_layernorm_bwd_fused(*head, h16.ptr(), ldh, cs.ptr() if cs else None, ws.data_ptr(), ws.numel() * 4,
                                          _st()) == 0
    ref = ro.layernorm_bwd_f64(x, dy, ga, EPS, dres_in, old, accumulate)
    o = out.check()
    r = {"dres": ro.ratio(o, *ref["dres"]), "dgamma": ro.ratio(dg.check()[0], *ref["dgamma"]),
         "dbeta": ro.ratio(db.check()[0], *ref["dbeta"])}
    outs = [o.clone(), dg.t.clone(), db.t.clone()]
    if rin is not None:
        assert rin.untouched(), "dres_in changed"
    if h16 is not None:
        h = h16.check()
        assert torch.equal(_bits(h), _bits(o.half())), "dres_f16 is not the fp16 rounding of the returned dres_out"
        outs.append(h.clone())
    if cs is not None:
        r["dres_colsum"] = ro.ratio(cs.check()[0], *ro.dres_colsum_f64(h16.t))
        outs.append(cs.t.clone())
    return r, tuple(outs)


BWD_CONFIGS = ((0, "sep", "colsum"), (1, "none", "plain"), (1, "sep", "copy"), (1, "alias", "copy"), (1, "sep", "colsum"),
               (0, "none", "copy"))


def _bwd_case(L, p, rows, family, shape, pitch=False):
    kept = {}
    for accumulate, dres, mode in BWD_CONFIGS:
        ratios = []
        outs = twice(lambda: ratios.append(run_ln_bwd(L, p, rows, accumulate, dres, mode, pitch)) or ratios[-1][1])
        _note("layernorm_bwd", family, shape, ratios[0][0])
        kept[(accumulate, dres, mode)] = outs
    for a, b in zip(kept[(1, "sep", "copy")], kept[(1, "alias", "copy")]):      # in place == out of place
        assert torch.equal(_bits(a), _bits(b)), "dres_out aliasing dres_in changes the result"
    for a, b in zip(kept[(1, "sep", "copy")][:3], kept[(1, "sep", "colsum")][:3]):   # fused outputs do not depend on colsum
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", BWD_D, ids=lambda d: f"NJ{ro.nj_of(d)}-d{d}")
def test_layernorm_backward(L, problems, d, xdt):
    for family in ro.FAMILIES:
        p = problems(family, 65, d, xdt, 2)
        for rows in (1, 5, 65):                       # at 65 the second workgroup has one row and three idle waves
            _bwd_case(L, p, rows, family, f"d{d}-{xdt}")


@pytest.mark.parametrize("xdt", list(DT))
@pytest.mark.parametrize("d", (260, 2052), ids=lambda d: f"NJ{ro.nj_of(d)}-d{d}")
def test_layernorm_backward_pitched(L, problems, d, xdt):
    """ldx = d + 8, lddy = d + 4, ldr = d + 4, ldh = d + 12"""
    for family in ("plain", "marker"):
        _bwd_case(L, problems(family, 65, d, xdt, 2), 65, family, f"d{d}-{xdt}-pitched", pitch=True)


@pytest.mark.parametrize("xdt", list(DT))
def test_layernorm_backward_row_loop(L, problems, xdt):
    """65606 rows at d = 4: the grid is capped at 1024 workgroups, every wave loops over 16 or 17 rows"""
    rows = 65606
    assert L.hcir_layernorm_bwd_blocks(rows) == 1024 and rows > 1024 * 4 * 16
    for family in ("plain", "marker"):
        p = problems(family, rows, 4, xdt)
        for accumulate, dres, mode in ((1, "sep", "colsum"), (0, "none", "plain")):
            ratios = []
            twice(lambda: ratios.append(run_ln_bwd(L, p, rows, accumulate, dres, mode)) or ratios[-1][1])
            _note("layernorm_bwd", family, f"rows{rows}-d4-{xdt}", ratios[0][0])


# ---------------------------------------------------------------------------------------------------------------
# GELU forward / backward, hcir_add_f32_f16: every finite fp16 value, and the grid-stride loops' second trip
# ---------------------------------------------------------------------------------------------------------------
TILES = 257          # 65536 * 257 = 8192 * 2048 + 65536 elements


def run_gelu_fwd(L, u):
    h = Buf(1, u.numel(), u.numel(), torch.float16)
    assert L.hcir_gelu_fwd_f16(u.data_ptr(), u.numel(), h.ptr(), _st()) == 0
    return (h.check()[0].clone(),)


def run_gelu_bwd(L, u, dh):
    du = Buf(1, u.numel(), u.numel(), torch.float16)
    assert L.hcir_gelu_bwd_f16(u.data_ptr(), dh.data_ptr(), u.numel(), du.ptr(), _st()) == 0
    return (du.check()[0].clone(),)


def test_gelu_forward_every_fp16(L):
    u = ro.all_finite_f16().cuda()
    h, = twice(lambda: run_gelu_fwd(L, u))
    _note("gelu_fwd", "every fp16", "n65536", {"h": ro.ratio(h, *ro.gelu_fwd_f64(u))})
    far = u.float().abs() >= 16.0                    # act.h: exact 0 / x in the tails
    assert torch.equal(h[far].float(), u[far].float().clamp_min(0.0))
    big = u.repeat(TILES)
    assert big.numel() == 8192 * 2048 + 65536 and big.numel() > 8192 * 256 * 8       # a second trip of the loop
    hb, = twice(lambda: run_gelu_fwd(L, big))
    assert torch.equal(_bits(hb), _bits(h.repeat(TILES)))


@pytest.mark.parametrize("pattern", ro.DH_PATTERNS)
def test_gelu_backward_every_fp16(L, pattern):
    u, dh = ro.all_finite_f16().cuda(), ro.dh_pattern(pattern).cuda()
    du, = twice(lambda: run_gelu_bwd(L, u, dh))
    _note("gelu_bwd", "every fp16", f"dh-{pattern}", {"du": ro.ratio(du, *ro.gelu_bwd_f64(u, dh))})
    far = u.float().abs() >= 16.0
    assert torch.equal(du[far].float(), (dh[far].float() * (u[far].float() > 0)))
    big, dhb = u.repeat(TILES), dh.repeat(TILES)
    assert big.numel() > 8192 * 256 * 8
    dub, = twice(lambda: run_gelu_bwd(L, big, dhb))
    assert torch.equal(_bits(dub), _bits(du.repeat(TILES)))


def add_inputs(n):
    """fp32 a, b [n]: the fp16 overflow threshold (65504 is the largest finite value, 65520 the tie to infinity), the
    subnormal range (2^-25 is the tie to zero, 3 * 2^-25 a tie between subnormals), ties of the normal range
    (1 + 2^-11, 1 + 3 * 2^-11), fp32 subnormals, and sums a + b that are ties or cross the threshold."""
    i = torch.arange(n)
    pa = torch.tensor([65504.0, 65519.0, 65519.996, 65520.0, 65536.0, 7e4, 3e38, 2.0 ** -24, 2.0 ** -25,
                       2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 1 + 2.0 ** -11,
                       1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1e-40, 0.0, 1.0, 0.1, 1000.3, 2.0 ** -24 * 2.5])
    pb = torch.tensor([0.0, 2.0 ** -11, 16.0, 15.996, 2.0 ** -25, -2.0 ** -25, 1.0, -1.0, 3e-8, 2.0 ** -12, 65504.0, -65504.0,
                       1e-40, 0.25, -0.1, 2.0 ** -24, 3 * 2.0 ** -11])          # 22 and 17 values: coprime periods
    sign = torch.where((i // 374) % 2 == 1, -1.0, 1.0)
    jitter = 1.0 + ((i // 748) % 64).float() * 2.0 ** -13 * ((i // 748) % 3 == 2)
    return (pa[i % 22] * sign * jitter).float(), (pb[i % 17] * jitter).float()


def run_add(L, a, b):
    y = Buf(1, a.numel(), a.numel(), torch.float16)
    assert L.hcir_add_f32_f16(a.data_ptr(), _ptr(b), a.numel(), y.ptr(), _st()) == 0
    return (y.check()[0].clone(),)


def test_add_f32_f16_bit_exact(L):
    """fp16(a + b): one IEEE fp32 add, one round-to-nearest-even conversion - the bits of torch's CPU (a + b).half()"""
    n = 8192 * 1024 + 4
    assert n > 8192 * 256 * 4 and n % 4 == 0         # a second trip of the loop
    a, b = add_inputs(n)
    want_ab, want_a = (a + b).half(), a.half()
    assert torch.isinf(want_ab).any() and (want_ab == 65504.0).any() and (want_ab.float().abs() == 2.0 ** -24).any()
    ad, bd = a.cuda(), b.cuda()
    y, = twice(lambda: run_add(L, ad, bd))
    assert torch.equal(_bits(y.cpu()), _bits(want_ab))
    y, = twice(lambda: run_add(L, ad, None))
    assert torch.equal(_bits(y.cpu()), _bits(want_a))


# ---------------------------------------------------------------------------------------------------------------
# hcir_colsum_f16, hcir_gelu_bwd_colsum_f16
# ---------------------------------------------------------------------------------------------------------------
def run_colsum(L, x, old, accumulate, ld=None):
    m, n = x.shape
    ld = ld or n
    xb = pitched(x, ld)
    out = vec(n, old if accumulate else None)
    chunks = L.hcir_colsum_chunks(m)
    ws = torch.full((chunks * n,), NAN, device="cuda")
    assert L.hcir_colsum_f16(xb.data_ptr(), m, n, ld, out.ptr(), accumulate, ws.data_ptr(), ws.numel() * 4, _st()) == 0
    return (out.check()[0].clone(),)


def run_gelu_bwd_colsum(L, u, dh, old, accumulate, ld=None):
    m, n = u.shape
    ld = ld or n
    ub, dhb = pitched(u, ld), pitched(dh, ld)
    du = Buf(m, n, ld, torch.float16)
    out = vec(n, old if accumulate else None)
    chunks = L.hcir_colsum_chunks(m)
    ws = torch.full((chunks * n,), NAN, device="cuda")
    assert L.hcir_gelu_bwd_colsum_f16(ub.data_ptr(), dhb.data_ptr(), m, n, ld, du.ptr(), out.ptr(), accumulate,
                                      ws.data_ptr(), ws.numel() * 4, _st()) == 0
    return du.check().clone(), out.check()[0].clone()


@pytest.mark.parametrize("shape", list(COLSUM_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_colsum_and_gelu_bwd_colsum(L, shape):
    m, n = shape
    assert L.hcir_colsum_chunks(m) == COLSUM_SHAPES[shape] == ro.colsum_chunks(m)
    g = torch.Generator().manual_seed(m + n)
    u = (torch.randn(m, n, generator=g) * 2.0).half().cuda()
    for family in ro.MAT_FAMILIES:
        x, old = (t.cuda() for t in ro.make_matrix(family, m, n))
        for ld in ((n, n + 8) if shape in ((13, 264), (1025, 256)) else (n,)):
            tag = f"{m}x{n}" + ("-pitched" if ld != n else "")
            for accumulate in (0, 1):
                out, = twice(lambda: run_colsum(L, x, old, accumulate, ld))
                _note("colsum_f16", family, tag, {f"acc{accumulate}": ro.ratio(out, *ro.colsum_f64(x, old, accumulate))})
                du, cs = twice(lambda: run_gelu_bwd_colsum(L, u, x, old, accumulate, ld))
                _note("gelu_bwd_colsum", family, tag,
                      {f"du/acc{accumulate}": ro.ratio(du, *ro.gelu_bwd_f64(u, x)),
                       f"colsum/acc{accumulate}": ro.ratio(cs, *ro.colsum_f64(du, old, accumulate))})
                # the fused kernel against the two separate ones, bit for bit
                du_sep, = run_gelu_bwd(L, u.reshape(-1), x.reshape(-1))
                cs_sep, = run_colsum(L, du_sep.view(m, n), old, accumulate)
                assert torch.equal(_bits(du), _bits(du_sep.view(m, n))) and torch.equal(_bits(cs), _bits(cs_sep))


# ---------------------------------------------------------------------------------------------------------------
# rejections: host-side returns, nothing is launched
# ---------------------------------------------------------------------------------------------------------------
def test_rejections(L):
    rows, d, wide = 4, 8, 4200
    x32 = torch.randn(rows * 3, wide, device="cuda")
    x16, dy = x32.half(), torch.randn(rows * 3, wide, device="cuda").half()
    ga, be = torch.ones(wide, device="cuda"), torch.zeros(wide, device="cuda")
    y16, o32 = Buf(rows * 3, wide, wide, torch.float16), Buf(rows * 3, wide, wide, torch.float32)
    dg, db, cs = vec(wide), vec(wide), vec(wide)
    ws = torch.full((4 * wide * 3,), NAN, device="cuda")
    st, X, G, B = _st(), x32.data_ptr(), ga.data_ptr(), be.data_ptr()

    def ln(d=d, ldx=wide, ldy=wide, dt=ro.F32, x=X, g=G, b=B):
        return L.hcir_layernorm_f16(x, dt, rows, d, ldx, g, b, EPS, y16.ptr(), ldy, st)

    assert ln(d=6) == INVALID and ln(d=2052) == INVALID and ln(ldx=4) == INVALID and ln(ldy=4) == INVALID
    assert ln(ldx=wide + 2) == INVALID and ln(ldy=wide + 2) == INVALID and ln(dt=2) == UNSUPPORTED
    assert ln(g=None) == INVALID and ln(b=None) == INVALID

    def head(d=d, t=3, dt=ro.F32, g=G, b=B, e32=o32.ptr(), e16=y16.ptr()):
        return L.hcir_cls_head(X, dt, rows, t, d, g, b, EPS, 1, e32, e16, st)

    assert head(d=6) == INVALID and head(d=2052) == INVALID and head(dt=2) == UNSUPPORTED
    assert head(g=None) == INVALID and head(b=None) == INVALID and head(e32=None, e16=None) == INVALID

    def pmean(d=d, t=3, dt=ro.F32, g=G, b=B):
        return L.hcir_patch_mean(X, dt, rows, t, d, g, b, EPS, o32.ptr(), st)

    assert pmean(d=6) == INVALID and pmean(d=2052) == INVALID and pmean(t=1) == INVALID and pmean(t=0) == INVALID
    assert pmean(dt=2) == UNSUPPORTED and pmean(g=None) == INVALID and pmean(b=None) == INVALID

    need = L.hcir_layernorm_bwd_blocks(rows) * d * 4

    def bwd(d=d, ldx=wide, lddy=wide, ldr=wide, ldh=wide, dt=ro.F32, h=y16.ptr(), c=None, ws_bytes=None, fused=True):
        nbytes = need * (3 if c else 2) if ws_bytes is None else ws_bytes
        args = (X, dt, rows, d, ldx, dy.data_ptr(), lddy, G, EPS, None, o32.ptr(), ldr, dg.ptr(), db.ptr(), 0)
        if fused:
            return L.hcir_layernorm_bwd_fused(*args, h, ldh, c, ws.data_ptr(), nbytes, st)
        return L.hcir_layernorm_bwd(*args, ws.data_ptr(), nbytes, st)

    for fused in (True, False):
        assert bwd(d=6, fused=fused) == INVALID and bwd(d=4100, fused=fused) == INVALID
        assert bwd(ldx=4, fused=fused) == INVALID and bwd(lddy=4, fused=fused) == INVALID and bwd(ldr=4, fused=fused) == INVALID
        assert bwd(ldr=wide + 2, fused=fused) == INVALID
        assert bwd(ldx=wide + 2, fused=fused) == INVALID and bwd(lddy=wide + 2, fused=fused) == INVALID    # four-element loads
        assert bwd(ldx=wide + 1, fused=fused) == INVALID and bwd(lddy=wide + 3, fused=fused) == INVALID
        assert bwd(dt=2, fused=fused) == UNSUPPORTED
        assert bwd(ws_bytes=need * 2 - 4, fused=fused) == WORKSPACE
    assert bwd(ldh=4) == INVALID and bwd(ldh=wide + 2) == INVALID
    assert bwd(h=None, c=cs.ptr()) == INVALID
    assert bwd(c=cs.ptr(), ws_bytes=need * 3 - 4) == WORKSPACE

    U, DH = x16.data_ptr(), dy.data_ptr()
    assert L.hcir_gelu_fwd_f16(U, 12, y16.ptr(), st) == INVALID and L.hcir_gelu_bwd_f16(U, DH, 12, y16.ptr(), st) == INVALID
    assert L.hcir_add_f32_f16(X, None, 6, y16.ptr(), st) == INVALID
    cneed = L.hcir_colsum_chunks(rows) * 16 * 4
    assert L.hcir_colsum_f16(U, rows, 12, wide, dg.ptr(), 0, ws.data_ptr(), cneed, st) == INVALID
    assert L.hcir_colsum_f16(U, rows, 16, 20, dg.ptr(), 0, ws.data_ptr(), cneed, st) == INVALID
    assert L.hcir_colsum_f16(U, rows, 16, 8, dg.ptr(), 0, ws.data_ptr(), cneed, st) == INVALID
    assert L.hcir_colsum_f16(U, rows, 16, wide, dg.ptr(), 0, ws.data_ptr(), cneed - 4, st) == WORKSPACE
    for n, ld, nbytes, want in ((12, wide, cneed, INVALID), (16, 20, cneed, INVALID), (16, 8, cneed, INVALID),
                                (16, wide, cneed - 4, WORKSPACE)):
        assert L.hcir_gelu_bwd_colsum_f16(U, DH, rows, n, ld, y16.ptr(), dg.ptr(), 0, ws.data_ptr(), nbytes, st) == want
    torch.cuda.synchronize()
    for buf in (y16, o32, dg, db, cs):
        assert buf.untouched()
    assert torch.isnan(ws).all()
