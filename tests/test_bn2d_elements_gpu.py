"""GPU: every element and every channel of the batch-statistics BatchNorm2d kernels' outputs (csrc/bn2d.hip) against
oracle.bn2d's float64 references through the bounds derived there (err / bound <= 1; tests/test_bn2d_host.py shows
the bounds honest and sharp), at the plans a training batch runs:

  CAPPED   about 21 M elements: the chunk count clamped by the grid cap, 6 passes per chunk (the 4-row unrolled body of
           the statistics kernel plus a tail row, three trips of the backward's 2-row body), 6 trips of the elementwise
           kernels' grid stride, 7 - 27 chunks per finalize lane, a last chunk of 1 - 21 rows;
  STRIDED  about 4.5 M elements: 2 apply trips, 2 - 10 chunks per finalize lane, C = 192, 320, 384 with 3 and 5 slabs;
  the small maps of tests/test_bn2d_gpu.py (one trip, one chunk per lane) as well.

Each case asserts through oracle.bn2d.plan and hcir_bn2d_chunks that it reaches the branch it is there for.  The
kernels are called through the C ABI into buffers between canary rows, outputs prefilled with NaN (an unwritten
element is an infinite error), the workspace followed by NaN that must stay, every case twice with bit-equal results.
References and bounds are torch float64 on the device: independent of the HIP kernels.

Besides the bounds: small-integer maps whose sums are exact in fp32 (dbeta, dgamma bit for bit), one hot row at every
boundary of the plan (closed-form mean and rstd; dbeta, dgamma equal to the row), and the shared workspace reused
across plans.  The worst err / bound per shape, family and check is printed at the end of the module
(profiles/bn2d_bounds.txt)."""
import pytest
import torch

from oracle import bn2d as ob

pytestmark = pytest.mark.gpu

NAN = float("nan")
CANARY = 2
WORST = {}
OUTPUTS = ("y", "save_mean", "save_rstd", "running_mean", "running_var", "dx", "dresid", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\nbn2d worst err / bound per shape and family (both switch combinations), check by check:")
    for (shape, family), per in sorted(WORST.items()):
        print(f"bn2d-worst {shape:22s} {family:14s} " + "  ".join(f"{k} {v:.3f}" for k, v in per.items()))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Buf:
    """[CANARY + rows + CANARY, cols]: a pattern in the canary rows, NaN (or `init`) in the live rows; check() wants the
    canary rows back bit-equal."""

    def __init__(self, rows, cols, dtype, init=None):
        self.rows = rows
        self.buf = torch.empty(rows + 2 * CANARY, cols, dtype=dtype, device="cuda")
        edge = ((torch.arange(2 * CANARY * cols, device="cuda") % 251) - 125).to(dtype).view(2 * CANARY, cols)
        self.buf[:CANARY], self.buf[CANARY + rows:] = edge[:CANARY], edge[CANARY:]
        self.t = self.buf[CANARY:CANARY + rows]
        self.t[...] = NAN if init is None else init
        self.edge = edge

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        got = torch.cat([self.buf[:CANARY], self.buf[CANARY + self.rows:]])
        assert torch.equal(_bits(got), _bits(self.edge)), "rows before or past the buffer written"
        return self.t


def vec(c, init=None):
    return Buf(1, c, torch.float32, init)


def run(L, prob, relu, resid):
    """one forward and one backward through the C ABI -> {name: tensor}"""
    x, dy, gamma, beta = prob["x"], prob["dy"], prob["gamma"], prob["beta"]
    m, c = x.shape
    need = L.hcir_bn2d_workspace_bytes(m, c)
    assert need == ob.plan(m, c).chunks * c * 8
    ws = torch.full((need // 4 + 64,), NAN, device="cuda")
    y, dx = Buf(m, c, torch.float16), Buf(m, c, torch.float16)
    dresid = Buf(m, c, torch.float16) if resid else None
    mean, rstd, dgamma, dbeta = vec(c), vec(c), vec(c), vec(c)
    rm, rv = vec(c, prob["rm"]), vec(c, prob["rv"])
    assert L.hcir_bn2d_fwd_nhwc_f16(x.data_ptr(), m, c, gamma.data_ptr(), beta.data_ptr(), ob.EPS, ob.MOMENTUM,
                                    prob["resid"].data_ptr() if resid else None, int(relu), rm.ptr(), rv.ptr(),
                                    mean.ptr(), rstd.ptr(), y.ptr(), ws.data_ptr(), need, _st()) == 0
    assert torch.isnan(ws[need // 4:]).all(), "the forward wrote past its workspace"
    ws.fill_(NAN)
    assert L.hcir_bn2d_bwd_nhwc_f16(dy.data_ptr(), x.data_ptr(), y.ptr() if relu else None, m, c, gamma.data_ptr(),
                                    mean.ptr(), rstd.ptr(), dx.ptr(), dresid.ptr() if resid else None, dgamma.ptr(),
                                    dbeta.ptr(), ws.data_ptr(), need, _st()) == 0
    assert torch.isnan(ws[need // 4:]).all(), "the backward wrote past its workspace"
    out = dict(y=y.check(), dx=dx.check(), dresid=dresid.check() if resid else None)
    for name, b in (("save_mean", mean), ("save_rstd", rstd), ("running_mean", rm), ("running_var", rv),
                    ("dgamma", dgamma), ("dbeta", dbeta)):
        out[name] = b.check()[0]
    return out


def twice(fn):
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), f"two runs differ in {k}"
    return a


def _note(shape, family, tag, ratios):
    per = WORST.setdefault((str(shape), family), {})
    for name, val in ratios.items():
        per[name] = max(per.get(name, 0.0), val)
    assert all(v <= 1.0 for v in ratios.values()), (shape, family, tag, ratios)


def _branch(L, shape):
    """the plan the kernels run the shape with, and the branch the shape is in the suite for"""
    from hcir import ops
    m, c = ob.rows_of(shape), shape[3]
    p = ob.plan(m, c)
    assert ops.bn2d_chunks(m, c) == p.chunks == L.hcir_bn2d_chunks(m, c)
    if shape in ob.CAPPED_SHAPES:
        assert p.clamped and p.chunks * p.slabs <= ob.GRID_CAP < ob.cdiv(ob.cdiv(m, p.rpp), ob.MIN_PASSES) * p.slabs
        assert p.chunk_passes == 6 and p.trips == 6 and p.per >= 7 and p.last_rows < p.rows_per_chunk
    elif shape in ob.STRIDED_SHAPES:
        assert p.chunk_passes == 4 and p.trips == 2 and p.per >= 2 and p.last_rows < p.rows_per_chunk
        assert p.slabs == {128: 1, 192: 3, 320: 5, 384: 3}[c]
    else:
        assert p.chunk_passes <= 4 and p.trips == 1 and p.per == 1
    return m, c, p


@pytest.mark.parametrize("shape", ob.SMALL_SHAPES + ob.STRIDED_SHAPES + ob.CAPPED_SHAPES, ids=str)
def test_every_element_and_channel_within_its_bound(L, shape):
    m, c, p = _branch(L, shape)
    for family in ob.FAMILIES:
        prob = ob.make_problem(family, m, c, seed=c + shape[0], device="cuda")
        for relu, resid in ((True, True), (False, False)):
            out = twice(lambda: run(L, prob, relu, resid))
            if relu:
                assert (out["y"] == 0).any() and (out["y"] > 0).any()
            _note(shape, family, f"relu{int(relu)} resid{int(resid)}", ob.check_outputs(prob, p, relu, resid, out))
        del prob, out


@pytest.mark.parametrize("shape", ob.STRIDED_SHAPES + ob.CAPPED_SHAPES, ids=str)
def test_integer_sums_bit_for_bit(L, shape):
    """mean 0, rstd 1, gamma 1, |dy| <= 2, |x| <= 3: every partial sum is an integer below 2^24, whatever the order"""
    from hcir import ops
    m, c, p = _branch(L, shape)
    assert 6 * m < 2 ** 24
    for with_mask in (False, True):
        prob = ob.exact_problem(m, c, with_mask, device="cuda")
        dbeta, dgamma = ob.exact_sums(prob)
        y = prob["y"].view(shape) if with_mask else None
        for _ in range(2):
            dx, _, got_dgamma, got_dbeta = ops.bn2d_bwd(prob["dy"].view(shape), prob["x"].view(shape), y, prob["gamma"],
                                                        prob["mean"], prob["rstd"])
            assert torch.equal(got_dbeta.double(), dbeta.double()), f"dbeta, mask {with_mask}"
            assert torch.equal(got_dgamma.double(), dgamma.double()), f"dgamma, mask {with_mask}"
        g = ob.masked(prob["dy"], prob["y"])
        ratio = ob.ratio(dx.view(m, c), *ob.dx_f64(g, prob["x"], prob["mean"], prob["rstd"], prob["gamma"], got_dgamma,
                                                   got_dbeta, m))
        _note(shape, "integers", f"mask{int(with_mask)}", {"dx": ratio})


@pytest.mark.parametrize("shape", ob.PROBE_SHAPES, ids=str)
def test_one_hot_row_at_every_boundary_of_the_plan(L, shape):
    """x = 1024 in one row, 0 elsewhere: mean = 1024 / M and rstd in closed form; dy hot instead: dbeta = dy[r] and
    dgamma = dy[r] x[r] exactly.  A row that a chunk, pass or trip boundary loses or counts twice shows in full."""
    from hcir import ops
    m, c, p = _branch(L, shape)
    rows = ob.probe_rows(m, p)
    last0 = (p.chunks - 1) * p.rows_per_chunk
    assert {0, p.rpp - 1, p.rpp, p.rows_per_chunk - 1, p.rows_per_chunk, last0, m - 1, p.apply_blocks * p.rpp - 1,
            p.apply_blocks * p.rpp} == set(rows) and last0 < m - 1
    mean, rstd = ob.hot_stats(m)
    base = ob.exact_problem(m, c, False, device="cuda")
    x = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    dy = torch.zeros(m, c, dtype=torch.float16, device="cuda")
    hot = ob.hot_dy(m, c, 0, device="cuda")[0]
    worst = {"save_mean": 0.0, "save_rstd": 0.0}
    for r in rows:
        x[r] = ob.HOT
        got_mean, got_rstd = ops.bn2d_stats(x.view(shape), ob.EPS, ob.MOMENTUM)
        x[r] = 0.0
        worst["save_mean"] = max(worst["save_mean"], float((got_mean.double() - mean).abs().max() / (ob.HOT_TOL * mean)))
        worst["save_rstd"] = max(worst["save_rstd"], float((got_rstd.double() - rstd).abs().max() / (ob.HOT_TOL * rstd)))
        assert worst["save_mean"] <= 1.0 and worst["save_rstd"] <= 1.0, (r, worst)
        dy[r] = hot
        _, _, got_dgamma, got_dbeta = ops.bn2d_bwd(dy.view(shape), base["x"].view(shape), None, base["gamma"],
                                                   base["mean"], base["rstd"])
        dy[r] = 0.0
        assert torch.equal(got_dbeta, hot.float()), f"dbeta, row {r}"
        assert torch.equal(got_dgamma, hot.float() * base["x"][r].float()), f"dgamma, row {r}"
    _note(shape, "hot row", "", worst)


def test_shared_workspace_reused_across_plans(L):
    """a CAPPED plan, a one-chunk plan and the CAPPED plan again on hcir.ops' shared workspace: each bit-equal to a
    run on a workspace of its own"""
    from hcir import ops
    big, small = (61, 13, 13, 2048), (3, 5, 5, 64)
    probs, own = {}, {}
    for shape in (big, small):
        m, c, _ = _branch(L, shape)
        probs[shape] = ob.make_problem("random_buffers", m, c, seed=5, device="cuda")
        own[shape] = run(L, probs[shape], True, True)
    for shape in (big, small, big):
        prob = probs[shape]
        rm, rv = prob["rm"].clone(), prob["rv"].clone()
        y, mean, rstd = ops.bn2d_fwd(prob["x"].view(shape), prob["gamma"], prob["beta"], ob.EPS, ob.MOMENTUM,
                                     prob["resid"].view(shape), True, rm, rv)
        dx, dresid, dgamma, dbeta = ops.bn2d_bwd(prob["dy"].view(shape), prob["x"].view(shape), y, prob["gamma"], mean,
                                                 rstd, want_dresid=True)
        got = dict(zip(OUTPUTS, (y, mean, rstd, rm, rv, dx, dresid, dgamma, dbeta)))
        for name in OUTPUTS:
            assert torch.equal(_bits(got[name].reshape(own[shape][name].shape)), _bits(own[shape][name])), (shape, name)
