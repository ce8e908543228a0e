"""GPU: every element of the outputs of the kernels that close the HSimCLR step and finish an embedding, against
oracle.head_loss's float64 references through the bounds derived there (err / bound <= 1; tests/test_head_loss_host.py
shows the bounds honest and sharp):

  hcir_bn1d_fwd / _bwd           (rows, f) of oracle.head_loss.BN_SHAPES: one column, exactly one workgroup, one live
                                 column in the last workgroup, a ragged last workgroup, three workgroups, the head's
                                 width; rows 1 .. 1023 with every rows % 4; the four output modes; the three dy_scale
                                 values; with and without the ReLU mask; all six pitches distinct and above f
  hcir_triplet_margin_fwd / _bwd d below, at and off the 64 lanes, b off the 4 rows of a workgroup, b = 1, two margins
  hcir_mse_fwd / _bwd            one element to two grid-stride trips with a ragged tail; dx only, dy only, both
  hcir_l2_normalize              d off 256, n off 4; a zero row, a row below eps, rows scaled by 1e-15 and 1e15
  hcir_convert_f32               the scalar tail and the second grid-stride trip; special values, bit for bit

The kernels are called through the C ABI into buffers between canaries, live elements prefilled with NaN (an unwritten
element is an infinite error), the gap columns of a pitched buffer holding a sentinel that must come back, every case
twice with bit-equal results.  Every buffer is 16-byte aligned at its first live element.  References and bounds are
torch float64 on the device.  The worst err / bound per kernel, shape and family is printed at the end of the module
(profiles/head_loss_bounds.txt)."""
import pytest
import torch

from oracle import head_loss as oh

pytestmark = pytest.mark.gpu

NAN = float("nan")
CANARY = 64                       # elements before and after, rounded up so the live part starts 16-byte aligned
SENTINEL = -77.0
WORST = {}
HCIR_F16, HCIR_BF16 = 1, 2


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\nhead-loss worst err / bound per kernel, shape and family (all modes), check by check:")
    for (kernel, shape, family), per in sorted(WORST.items()):
        figures = "  ".join(f"{k} {v:.3f}" for k, v in per.items() if "=" not in k)           # equalities: 0 or a failure
        print(f"head-loss-worst {kernel:8s} {shape:14s} {family:14s} {figures}")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Buf:
    """rows x cols live elements at pitch ld inside one flat allocation: canary | rows * ld | canary.  The canaries hold a
    pattern, the live elements NaN (or `init`), the gap columns [cols, ld) SENTINEL; check() wants canaries and gaps
    back bit-equal and returns the live view."""

    def __init__(self, rows, cols, dtype=torch.float32, ld=None, init=None):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        n = rows * ld
        self.flat = torch.empty(2 * CANARY + n, dtype=dtype, device="cuda")
        self.edge = ((torch.arange(2 * CANARY, device="cuda") % 251) - 125).to(dtype)
        self.flat[:CANARY], self.flat[CANARY + n:] = self.edge[:CANARY], self.edge[CANARY:]
        self.grid = self.flat[CANARY:CANARY + n].view(rows, ld)
        self.grid[...] = SENTINEL
        self.t = self.grid[:, :cols]
        self.t[...] = NAN if init is None else init
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        n = self.rows * self.ld
        got = torch.cat([self.flat[:CANARY], self.flat[CANARY + n:]])
        assert torch.equal(_bits(got), _bits(self.edge)), "elements before or past the buffer written"
        gap = self.grid[:, self.cols:]
        assert torch.equal(_bits(gap), _bits(torch.full_like(gap, SENTINEL))), "gap columns of a pitched buffer written"
        return self.t


def vec(n, init=None):
    return Buf(1, n, torch.float32, None, init)


def scalar(v):
    return Buf(1, 1, torch.float32, None, v)


def twice(fn):
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), f"two runs differ in {k}"
    return a


def _note(kernel, shape, family, tag, ratios):
    per = WORST.setdefault((kernel, str(shape), family), {})
    for name, val in ratios.items():
        per[name] = max(per.get(name, 0.0), val)
    assert all(v <= 1.0 for v in ratios.values()), (kernel, shape, family, tag, ratios)


# ---------------------------------------------------------------------------------------------------------------
# bn1d
# ---------------------------------------------------------------------------------------------------------------
#            relu  y32    y16    running scale      mask
BN_MODES = [(True, False, True, True, None, True),            # ReLU + y_f16 only, the mask from the forward's output
            (False, True, False, True, 3.0, False),           # no ReLU + y_f32 only
            (True, True, True, False, 2.0 ** -7, True),       # both outputs, running pointers NULL
            (True, True, True, True, 2.0 ** -7, False)]       # ReLU in the forward, relu_out_f16 NULL in the backward


def pitches(f):
    """ldx, ldy32, ldy16, lddy, ldr, lddx: distinct, above f, multiples of 8 elements (16 bytes in fp16)"""
    base = (f // 8 + 1) * 8
    return [base + 8 * i for i in (3, 1, 4, 0, 5, 2)]


def bn_forward(L, prob, relu, want32, want16, running, ld):
    rows, f = prob["x"].shape
    ldx, ldy32, ldy16 = ld[:3]
    x = Buf(rows, f, torch.float32, ldx, prob["x"])
    y32 = Buf(rows, f, torch.float32, ldy32) if want32 else None
    y16 = Buf(rows, f, torch.float16, ldy16) if want16 else None
    mean, rstd = vec(f), vec(f)
    rm, rv = vec(f, prob["rm"]), vec(f, prob["rv"])
    gamma, beta = vec(f, prob["gamma"]), vec(f, prob["beta"])
    assert L.hcir_bn1d_fwd(x.ptr(), ldx, rows, f, gamma.ptr(), beta.ptr(), oh.EPS, oh.MOMENTUM, int(relu),
                           rm.ptr() if running else None, rv.ptr() if running else None, mean.ptr(), rstd.ptr(),
                           y32.ptr() if want32 else None, ldy32, y16.ptr() if want16 else None, ldy16, _st()) == 0
    out = {"save_mean": mean.check()[0], "save_rstd": rstd.check()[0], "y32": y32.check() if want32 else None,
           "y16": y16.check() if want16 else None, "running_mean": rm.check()[0], "running_var": rv.check()[0]}
    for b, src in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
        assert torch.equal(_bits(b.check()), _bits(prob[src].reshape(b.t.shape))), f"the forward wrote its input {src}"
    return out


def bn_backward(L, prob, mean, rstd, y16, scale, ld):
    rows, f = prob["x"].shape
    ldx, _, _, lddy, ldr, lddx = ld
    x, dy = Buf(rows, f, torch.float32, ldx, prob["x"]), Buf(rows, f, torch.float32, lddy, prob["dy"])
    mask = Buf(rows, f, torch.float16, ldr, y16) if y16 is not None else None
    dx = Buf(rows, f, torch.float16, lddx)
    dgamma, dbeta = vec(f), vec(f)
    gamma, km, kr = vec(f, prob["gamma"]), vec(f, mean), vec(f, rstd)
    sc = scalar(scale) if scale is not None else None
    assert L.hcir_bn1d_bwd(dy.ptr(), lddy, x.ptr(), ldx, rows, f, gamma.ptr(), km.ptr(), kr.ptr(),
                           mask.ptr() if mask else None, ldr, sc.ptr() if sc else None, dx.ptr(), lddx, dgamma.ptr(),
                           dbeta.ptr(), _st()) == 0
    for b in (x, dy, gamma, km, kr) + ((mask,) if mask else ()) + ((sc,) if sc else ()):
        b.check()
    return {"dx": dx.check(), "dgamma": dgamma.check()[0], "dbeta": dbeta.check()[0]}


def bn_run(L, prob, mode, pitched=False):
    relu, want32, want16, running, scale, use_mask = mode
    f = prob["x"].shape[1]
    ld = pitches(f) if pitched else [f] * 6
    out = bn_forward(L, prob, relu, want32, want16, running, ld)
    if not running:
        assert torch.equal(_bits(out["running_mean"]), _bits(prob["rm"])), "running_mean written through a NULL"
        assert torch.equal(_bits(out["running_var"]), _bits(prob["rv"])), "running_var written through a NULL"
        out["running_mean"] = out["running_var"] = None
    out.update(bn_backward(L, prob, out["save_mean"], out["save_rstd"], out["y16"] if use_mask else None, scale, ld))
    return out


@pytest.mark.parametrize("shape", oh.BN_SHAPES, ids=str)
def test_bn1d_every_element_and_column_within_its_bound(L, shape):
    rows, f = shape
    for family in oh.FAMILIES:
        prob = oh.make_bn1d(family, rows, f, seed=rows + f, device="cuda")
        outs = []
        for mode in BN_MODES:
            relu, _, _, _, scale, use_mask = mode
            out = twice(lambda: bn_run(L, prob, mode))
            outs.append(out)
            if relu and rows * f >= 64:
                y = out["y16"]
                assert (y == 0).any() and (y > 0).any()
            _note("bn1d", shape, family, str(mode), oh.check_bn1d(prob, relu, out, scale, use_mask))
        # NULL running pointers change nothing else: the statistics and y of the ReLU modes are the same bits
        for name in ("save_mean", "save_rstd", "y16"):
            assert torch.equal(_bits(outs[0][name]), _bits(outs[2][name])), name
            assert torch.equal(_bits(outs[3][name]), _bits(outs[2][name])), name
        assert torch.equal(_bits(outs[3]["y32"]), _bits(outs[2]["y32"]))


@pytest.mark.parametrize("shape", oh.BN_SHAPES, ids=str)
def test_bn1d_six_distinct_pitches_give_the_same_bits(L, shape):
    """all six leading dimensions distinct and above f: every output bit-equal to the run at pitch f (held to the
    bounds above), the gap columns untouched"""
    rows, f = shape
    assert len(set(pitches(f))) == 6 and min(pitches(f)) > f and {m[4] for m in BN_MODES} == set(oh.BN_SCALES)
    prob = oh.make_bn1d("random_buffers", rows, f, seed=rows + f + 1, device="cuda")
    for mode in BN_MODES:
        want, got = bn_run(L, prob, mode), bn_run(L, prob, mode, pitched=True)
        for k in want:
            assert (want[k] is None and got[k] is None) or torch.equal(_bits(want[k]), _bits(got[k])), (mode, k)
    _note("bn1d", shape, "pitched", "", oh.check_bn1d(prob, mode[0], got, mode[4], mode[5]))


@pytest.mark.parametrize("shape", [(1023, 100), (258, 768), (5, 65), (9, 1), (4, 64)], ids=str)
def test_bn1d_integer_sums_and_hot_rows_bit_for_bit(L, shape):
    """mean 0, rstd 1, gamma 1, |dy| <= 2, |x| <= 3: every partial sum is an integer below 2^24, whatever the order; then
    dy hot in one row (0, 3, 4, rows - 1): dbeta = dy[r], dgamma = dy[r] x[r].  A row lost when rows % 4 != 0 shows."""
    rows, f = shape
    assert 6 * rows < 2 ** 24
    base = oh.exact_bn1d(rows, f, device="cuda")
    ld = [f] * 6
    for y16 in (None, base["y16"]):
        g = base["dy"].double() * (1 if y16 is None else (y16 > 0))
        out = twice(lambda: bn_backward(L, base, base["mean"], base["rstd"], y16, None, ld))
        assert torch.equal(out["dbeta"].double(), g.sum(0)), f"dbeta, mask {y16 is not None}"
        assert torch.equal(out["dgamma"].double(), (g * base["x"].double()).sum(0)), f"dgamma, mask {y16 is not None}"
        _note("bn1d", shape, "integers", "", {"dx": oh.ratio(out["dx"], *oh.dx_f64(
            base["dy"], base["x"], base["mean"], base["rstd"], base["gamma"], out["dgamma"], out["dbeta"], None, y16))})
    assert set(oh.hot_rows(rows)) == {r for r in (0, 3, 4, rows - 1) if r < rows}
    for r in oh.hot_rows(rows):
        dy = torch.zeros(rows, f, device="cuda")
        dy[r] = base["dy"][r]
        out = bn_backward(L, dict(base, dy=dy), base["mean"], base["rstd"], None, None, ld)
        assert torch.equal(out["dbeta"], dy[r]), f"dbeta, row {r}"
        assert torch.equal(out["dgamma"], dy[r] * base["x"][r]), f"dgamma, row {r}"


# ---------------------------------------------------------------------------------------------------------------
# triplet
# ---------------------------------------------------------------------------------------------------------------
def triplet_run(L, a, p, n, margin):
    b, d = a.shape
    A, P, N = (Buf(b, d, init=t) for t in (a, p, n))
    loss, row_loss, dist = scalar(None), vec(b), Buf(2, b)
    assert L.hcir_triplet_margin_fwd(A.ptr(), P.ptr(), N.ptr(), b, d, margin, oh.TRIPLET_EPS, loss.ptr(), row_loss.ptr(),
                                     dist.ptr(), _st()) == 0
    out = {"loss": loss.check()[0, 0], "row_loss": row_loss.check()[0], "dist": dist.check()}
    go = scalar(oh.TRIPLET_GRAD)
    da, dp, dn = Buf(b, d), Buf(b, d), Buf(b, d)
    assert L.hcir_triplet_margin_bwd(A.ptr(), P.ptr(), N.ptr(), b, d, oh.TRIPLET_EPS, row_loss.ptr(), dist.ptr(), go.ptr(),
                                     da.ptr(), dp.ptr(), dn.ptr(), _st()) == 0
    for buf, src in ((A, a), (P, p), (N, n)):
        assert torch.equal(_bits(buf.check()), _bits(src))
    go.check(), row_loss.check(), dist.check()
    out.update(da=da.check(), dp=dp.check(), dn=dn.check())
    return out


@pytest.mark.parametrize("shape", oh.TRIPLET_SHAPES, ids=str)
def test_triplet_every_row_and_element_within_its_bound(L, shape):
    b, d = shape
    for family in ("normal", "large_mean", "scaled"):
        a, p, n = oh.make_triplet(family, b, d, seed=b + d, device="cuda")
        for margin in oh.MARGINS:
            out = twice(lambda: triplet_run(L, a, p, n, margin))
            active = out["row_loss"] > 0
            assert bool(active[0])                                # the p == a row: its gradient is looked at
            if b >= 4:
                assert active.any() and (~active).any()
            w = oh.check_triplet(a, p, n, margin, out)
            # p == a exactly: dist = eps sqrt(d), every element of up = 1 / sqrt(d)
            tol = ((oh.cdiv(d, 64) + 6) / 2 + 4) * oh.U32 * oh.SECOND
            up = out["dp"][0].double() * (-b / oh.TRIPLET_GRAD)
            w["dist (p is a)"] = abs(float(out["dist"][0, 0]) / (oh.TRIPLET_EPS * d ** 0.5) - 1.0) / tol
            w["up (p is a)"] = float((up * d ** 0.5 - 1.0).abs().max()) / tol
            _note("triplet", shape, family, f"margin {margin}", w)


# ---------------------------------------------------------------------------------------------------------------
# mse
# ---------------------------------------------------------------------------------------------------------------
def mse_run(L, x, y, want_dx, want_dy):
    n = x.numel()
    X, Y = Buf(1, n, init=x), Buf(1, n, init=y)
    loss, ws = scalar(None), vec(256)
    assert L.hcir_mse_fwd(X.ptr(), Y.ptr(), n, loss.ptr(), ws.ptr(), _st()) == 0
    assert torch.isnan(ws.check()[0, oh.mse_blocks(n):]).all(), "the workspace written past its partial sums"
    go = scalar(oh.MSE_GRAD)
    dx, dy = (Buf(1, n) if want_dx else None), (Buf(1, n) if want_dy else None)
    assert L.hcir_mse_bwd(X.ptr(), Y.ptr(), n, go.ptr(), dx.ptr() if dx else None, dy.ptr() if dy else None, _st()) == 0
    assert torch.equal(_bits(X.check()[0]), _bits(x)) and torch.equal(_bits(Y.check()[0]), _bits(y))
    go.check()
    return {"loss": loss.check()[0, 0], "dx": dx.check()[0] if dx else None, "dy": dy.check()[0] if dy else None}


@pytest.mark.parametrize("n", oh.MSE_SIZES)
def test_mse_loss_and_every_element_within_its_bound(L, n):
    assert oh.mse_trips(n) == (17 if n > 256 * 4096 else oh.cdiv(n, 256 * oh.mse_blocks(n)))
    for family in ("normal", "large_mean", "scaled"):
        x, y = (t.flatten() for t in oh.make_rows(family, 1, n, seed=n % 977, device="cuda", count=2))
        for want_dx, want_dy in ((True, False), (False, True), (True, True)):
            out = twice(lambda: mse_run(L, x, y, want_dx, want_dy))
            _note("mse", n, family, f"dx {want_dx} dy {want_dy}", oh.check_mse(x, y, out))


# ---------------------------------------------------------------------------------------------------------------
# l2_normalize, convert
# ---------------------------------------------------------------------------------------------------------------
def l2_run(L, x, want32, want16):
    n, d = x.shape
    X = Buf(n, d, init=x)
    y32 = Buf(n, d) if want32 else None
    y16 = Buf(n, d, torch.float16) if want16 else None
    assert L.hcir_l2_normalize(X.ptr(), n, d, oh.L2_EPS, y32.ptr() if y32 else None, y16.ptr() if y16 else None,
                               _st()) == 0
    assert torch.equal(_bits(X.check()), _bits(x))
    return {"y32": y32.check() if y32 else None, "y16": y16.check() if y16 else None}


@pytest.mark.parametrize("shape", oh.L2_SHAPES, ids=str)
def test_l2_normalize_every_element_within_its_bound(L, shape):
    x = oh.make_l2(*shape, seed=shape[1], device="cuda")
    got = {}
    for want32, want16 in ((True, False), (False, True), (True, True)):
        out = twice(lambda: l2_run(L, x, want32, want16))
        _note("l2", shape, "special rows", f"y32 {want32} y16 {want16}", oh.check_l2(x, out))
        for k, v in out.items():
            if v is not None:
                assert k not in got or torch.equal(_bits(got[k]), _bits(v)), f"{k} depends on the other output"
                got[k] = v
    if shape[0] >= 2:                                                                 # the zero row
        assert (x[-1] == 0).all() and (got["y32"][-1] == 0).all() and (got["y16"][-1] == 0).all()
    if shape[0] >= 3:                                                                 # the row below eps: x / eps
        assert oh.ratio(got["y32"][-2], x[-2].double() / oh.L2_EPS, 2 * oh.U32 * x[-2].double().abs() / oh.L2_EPS) <= 1.0


@pytest.mark.parametrize("n", oh.CONVERT_SIZES)
def test_convert_bit_equal_to_round_to_nearest_even(L, n):
    x = oh.convert_input(n, device="cuda")
    for dtype, code in ((torch.float16, HCIR_F16), (torch.bfloat16, HCIR_BF16)):
        def run():
            X, y = Buf(1, n, init=x), Buf(1, n, dtype)
            assert L.hcir_convert_f32(X.ptr(), n, code, y.ptr(), _st()) == 0
            got = X.check()[0]
            assert torch.equal(torch.isnan(got), torch.isnan(x)) and torch.equal(got[~torch.isnan(x)], x[~torch.isnan(x)])
            return {"y": y.check()[0]}
        _note("convert", n, str(dtype).split(".")[1], "", oh.check_convert(x, twice(run)["y"], dtype))
