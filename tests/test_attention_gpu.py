"""GPU: every element of every attention kernel's outputs against oracle.attention's float64 reference, through the
per-element bounds derived there (err / bound <= 1; tests/test_attention_host.py shows the bounds are honest and sharp).

Every case: outputs prefilled with NaN and required finite; every output buffer between canary blocks; two runs,
bit-equal; the float64 reference computed on the device in chunks of images.  Shapes are the smallest that reach each
path (key-tile counts 1..9 with ragged and exact last tiles, one live row / key in the last tile, partial last
workgroups, the persistent kernels' second and third items), not the workload's.

Worst err / bound per kernel and output on an MI355X (profiles/attention_errors.txt has every case and every kernel
instantiation; no bound was changed after the first GPU run):
  attn_fwd_kernel<1..9>        O 0.644   lse 0.077      attn_fwd2_kernel (persistent)   O 0.425   lse 0.048
  attn_fwd_generic_kernel      O 0.563 (hd 32 / 48 / 80 / 96 / 128 at 1, 2, 5 or 7, 9 key tiles)
  attn_bwd2_kernel (T <= 224)  dQ 0.675  dK 0.167  dV 0.529     attn_bwd_kernel (T <= 256)  dQ 0.721  dK 0.122  dV 0.229
  attn_cls_fwd_kernel          O 0.962   lse 0.062      attn_cls_bwd_kernel   dQ 0.751  dK 0.801  dV 0.972
(the class-token kernels keep P in fp32, so their bound is little more than the fp16 store's half ulp, which a
correctly rounded store reaches.)
"""
import pytest
import torch

from oracle import attention as oa

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
CANARY, PAD = 1234.0, 4096
WORST = {}


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\nattention worst err / bound per kernel and output:")
    for (kern, name), val in sorted(WORST.items()):
        print(f"attn-worst {kern:16s} {name:4s} {val:.3f}")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _note(kern, ratios, case):
    for name, val in ratios.items():
        WORST[(kern, name)] = max(WORST.get((kern, name), 0.0), val)
    print(f"\nattn-err {kern} {case}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def _scale(hd):
    return oa.f32(hd ** -0.5)


class Guarded:
    """An output buffer prefilled with NaN between two canary blocks."""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device="cuda")
        self.t = self.buf[PAD:PAD + n].view(shape)
        self.t.fill_(float("nan"))

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[-PAD:] == CANARY).all()), "canary overwritten"
        assert bool(torch.isfinite(self.t).all()), "an output element was not written"
        return self.t


def _twice(fn):
    """Run fn() -> tuple of tensors twice and require bit-equal results."""
    first, second = fn(), fn()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "two runs differ"
    return first


def run_fwd(L, qd, b, t, h, hd, scale, nq, with_lse=False):
    def once():
        out = Guarded((b, nq, h * hd), torch.float16)
        if with_lse:
            lse = Guarded((b, h, t), torch.float32)
            assert L.hcir_attn_fwd_lse(qd.data_ptr(), b, t, h, hd, scale, out.ptr(), lse.ptr(), _st()) == 0
            return out.check(), lse.check()
        assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, scale, nq, out.ptr(), _st()) == 0
        return (out.check(),)
    return _twice(once)


def run_bwd(L, qd, out, dout, lse, b, t, h, scale):
    def once():
        dqkv = Guarded((b, t, 3, h, 64), torch.float16)
        assert L.hcir_attn_bwd(qd.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), b, t, h, 64, scale,
                               dqkv.ptr(), _st()) == 0
        return (dqkv.check(),)
    return _twice(once)[0]


def _chunks(b, h, t):
    cb = max(1, (1 << 22) // (h * t * t))     # at most 32 MB per float64 [cb, h, t, t] matrix
    return [(i, min(b, i + cb)) for i in range(0, b, cb)]


def fwd_ratios(qd, out, lse, b, t, h, hd, scale, nq):
    r = {"o": 0.0}
    for lo, hi in _chunks(b, h, t):
        ref = oa.attention_f64(qd[lo:hi], hi - lo, t, h, hd, scale, nq=nq)
        bo, bl = oa.fwd_bounds(ref)
        r["o"] = max(r["o"], oa.ratio(oa.heads_of(out[lo:hi], hi - lo, nq, h, hd), ref.o, bo))
        if lse is not None:
            r["lse"] = max(r.get("lse", 0.0), oa.ratio(lse[lo:hi], ref.lse2, bl))
    return r


def bwd_ratios(qd, out, lse, dout, dqkv, b, t, h, scale):
    """The backward is fed the forward kernel's own out and lse; their bounds are the backward bound's o_err, lse_err."""
    r = {"o": 0.0, "lse": 0.0, "dq": 0.0, "dk": 0.0, "dv": 0.0}
    for lo, hi in _chunks(b, h, t):
        n = hi - lo
        ref = oa.attention_f64(qd[lo:hi], n, t, h, 64, scale, dout[lo:hi])
        bo, bl = oa.fwd_bounds(ref)
        bdq, bdk, bdv = oa.bwd_bounds(ref, bo, bl)
        d = dqkv[lo:hi].double().permute(2, 0, 3, 1, 4)
        for k, v in (("o", oa.ratio(oa.heads_of(out[lo:hi], n, t, h, 64), ref.o, bo)),
                     ("lse", oa.ratio(lse[lo:hi], ref.lse2, bl)), ("dq", oa.ratio(d[0], ref.dq, bdq)),
                     ("dk", oa.ratio(d[1], ref.dk, bdk)), ("dv", oa.ratio(d[2], ref.dv, bdv))):
            r[k] = max(r[k], v)
    return r


def fwd_kernel(b, t, h, hd, nq):
    nkt = (t + 31) // 32
    if hd != 64:
        return f"generic<{hd},{nkt}>"
    return "fwd2" if nkt == 7 and nq == t and b * h >= 512 else f"fwd<{nkt}>"


def _assert_within(r, case):
    assert all(v <= 1.0 for v in r.values()), (case, r)


# ---------------------------------------------------------------------------------------------------------------
# hcir_attn_fwd, head_dim 64
# ---------------------------------------------------------------------------------------------------------------
FWD_T = [1, 17, 32, 33, 65, 97, 129, 161, 193, 197, 224, 225, 256, 257, 288]


@pytest.mark.parametrize("b,h", [(1, 1), (2, 3), (3, 4)])
@pytest.mark.parametrize("t", FWD_T)
def test_fwd_every_key_tile_count(L, t, b, h):
    for fam in ("flat", "marker_last"):
        qd = oa.make_qkv(fam, b, t, h, 64).cuda()
        (out,) = run_fwd(L, qd, b, t, h, 64, _scale(64), t)
        r = fwd_ratios(qd, out, None, b, t, h, 64, _scale(64), t)
        _note(fwd_kernel(b, t, h, 64, t), r, f"{fam} b{b} t{t} h{h}")
        _assert_within(r, fam)


@pytest.mark.parametrize("t", [197, 17])
@pytest.mark.parametrize("fam", oa.FAMILIES)
def test_fwd_families(L, fam, t):
    b, h = 2, 3
    qd = oa.make_qkv(fam, b, t, h, 64).cuda()
    (out,) = run_fwd(L, qd, b, t, h, 64, _scale(64), t)
    r = fwd_ratios(qd, out, None, b, t, h, 64, _scale(64), t)
    _note(fwd_kernel(b, t, h, 64, t), r, f"{fam} b{b} t{t} h{h}")
    _assert_within(r, fam)


@pytest.mark.parametrize("t", [197, 225])      # seven key tiles (rows leave through the LDS transposition), eight (direct)
def test_fwd_query_row_limit(L, t):
    b, h = 2, 3
    for fam in ("marker_last", "sharp"):
        qd = oa.make_qkv(fam, b, t, h, 64).cuda()
        (full,) = run_fwd(L, qd, b, t, h, 64, _scale(64), t)
        for nq in (1, 31, 32, 33, 40, t):
            (part,) = run_fwd(L, qd, b, t, h, 64, _scale(64), nq)
            assert torch.equal(part, full[:, :nq]), (fam, nq)
            r = fwd_ratios(qd, part, None, b, t, h, 64, _scale(64), nq)
            _note(fwd_kernel(b, t, h, 64, nq), r, f"{fam} b{b} t{t} h{h} nq{nq}")
            _assert_within(r, (fam, nq))


@pytest.mark.parametrize("t", [x for x in FWD_T if x <= 256])
def test_fwd_lse(L, t):
    b, h = 2, 3
    for fam in ("marker_last", "sharp", "negdom"):
        qd = oa.make_qkv(fam, b, t, h, 64).cuda()
        out, lse = run_fwd(L, qd, b, t, h, 64, _scale(64), t, with_lse=True)
        (plain,) = run_fwd(L, qd, b, t, h, 64, _scale(64), t)
        assert torch.equal(out, plain), "hcir_attn_fwd_lse and hcir_attn_fwd differ"
        r = fwd_ratios(qd, out, lse, b, t, h, 64, _scale(64), t)
        _note(fwd_kernel(b, t, h, 64, t) + "+lse", r, f"{fam} b{b} t{t} h{h}")
        _assert_within(r, fam)


@pytest.mark.parametrize("b", [32, 33])        # h = 16: 512 items (two per workgroup exactly) and 528 (an uneven walk)
@pytest.mark.parametrize("t", [193, 197, 224])
def test_fwd_persistent(L, t, b):
    """b * h >= 512 at seven key tiles: the persistent double-buffered kernel.  Every image carries the marker, so the
    images a workgroup reaches as its second and third item (items >= 256: images 16 and up) do too.  Bit-equal to the
    same images in calls of fewer than 512 items (attn_fwd_kernel<7>): the two kernels share the code of the query
    tile, so this checks what they do not share - the double-buffered staging, the item walk, the barrier and the
    waits."""
    h = 16
    for fam in ("flat", "marker_last"):
        qd = oa.make_qkv(fam, b, t, h, 64).cuda()
        out, lse = run_fwd(L, qd, b, t, h, 64, _scale(64), t, with_lse=True)
        (plain,) = run_fwd(L, qd, b, t, h, 64, _scale(64), t)
        assert torch.equal(out, plain)
        for lo in range(0, b, 11):
            n = min(11, b - lo)
            po, pl = run_fwd(L, qd[lo:lo + n], n, t, h, 64, _scale(64), t, with_lse=True)
            assert torch.equal(po, out[lo:lo + n]) and torch.equal(pl, lse[lo:lo + n]), (fam, lo)
        r = fwd_ratios(qd, out, lse, b, t, h, 64, _scale(64), t)
        _note("fwd2+lse", r, f"{fam} b{b} t{t} h{h}")
        _assert_within(r, fam)


# every head_dim meets 1, 2 and 9 key tiles, a ragged and an exact last tile; 129 / 197 alternate
GENERIC = [(hd, t) for i, hd in enumerate((32, 48, 80, 96, 128)) for t in (1, 17, 50, 257, 288, (129, 197)[i % 2])]


@pytest.mark.parametrize("hd,t", GENERIC)
def test_fwd_generic_head_dims(L, hd, t):
    b, h = 2, 3
    for fam in ("flat", "uniform"):
        qd = oa.make_qkv(fam, b, t, h, hd).cuda()
        (full,) = run_fwd(L, qd, b, t, h, hd, _scale(hd), t)
        (one,) = run_fwd(L, qd, b, t, h, hd, _scale(hd), 1)
        assert torch.equal(one, full[:, :1])
        r = fwd_ratios(qd, full, None, b, t, h, hd, _scale(hd), t)
        _note(fwd_kernel(b, t, h, hd, t), r, f"{fam} b{b} t{t} h{h}")
        _assert_within(r, fam)


# ---------------------------------------------------------------------------------------------------------------
# hcir_attn_bwd
# ---------------------------------------------------------------------------------------------------------------
def _bwd_case(L, fam, b, t, h, dout=None):
    qd = oa.make_qkv(fam, b, t, h, 64).cuda()
    dout = (oa.make_dout(b, t, h, 64) if dout is None else dout).cuda()
    out, lse = run_fwd(L, qd, b, t, h, 64, _scale(64), t, with_lse=True)
    dqkv = run_bwd(L, qd, out, dout, lse, b, t, h, _scale(64))
    r = bwd_ratios(qd, out, lse, dout, dqkv, b, t, h, _scale(64))
    _note("bwd2" if t <= 224 else "bwd", {k: r[k] for k in ("dq", "dk", "dv")}, f"{fam} b{b} t{t} h{h}")
    _assert_within(r, fam)
    return qd, dout, out, lse, dqkv


@pytest.mark.parametrize("b,h", [(1, 1), (2, 3)])
@pytest.mark.parametrize("t", [1, 17, 32, 33, 65, 129, 193, 197, 225, 256])
def test_bwd_token_counts(L, t, b, h):
    for fam in ("flat", "marker_last"):
        _bwd_case(L, fam, b, t, h)


@pytest.mark.parametrize("fam", oa.FAMILIES)
def test_bwd_families(L, fam):
    _bwd_case(L, fam, 2, 197, 3)


def test_bwd_more_items_than_workgroups(L):
    """264 items on 256 persistent workgroups: eight of them carry a second item.  Bit-equal to one image per call."""
    b, t, h = 22, 197, 12
    qd, dout, out, lse, dqkv = _bwd_case(L, "marker_first", b, t, h)
    for i in range(b):
        one = run_bwd(L, qd[i:i + 1], out[i:i + 1], dout[i:i + 1], lse[i:i + 1], 1, t, h, _scale(64))
        assert torch.equal(one, dqkv[i:i + 1]), i


@pytest.mark.parametrize("t", [197, 256])
def test_bwd_exact_zero_ds(L, t):
    """uniform family, dout constant along the queries and confined to V's key-constant dims 0..3: dP does not depend
    on the key, so dS = 0, dQ = dK = 0 and dV_j = sum_i dout_i / t = dout in exact arithmetic.  The bounds' relative
    terms vanish with the reference; what is left are their absolute terms."""
    b, h = 2, 3
    dout = torch.zeros(b, t, h, 64)
    dout[..., :4] = torch.tensor([0.5, -0.25, 1.0, 0.125])
    dout = dout.reshape(b, t, h * 64).half()
    qd, doutd, out, lse, dqkv = _bwd_case(L, "uniform", b, t, h, dout)
    ref = oa.attention_f64(qd, b, t, h, 64, _scale(64), doutd)
    assert float(ref.dq.abs().max()) <= 1e-14 and float(ref.dk.abs().max()) <= 1e-14
    assert float((ref.dv - oa.heads_of(doutd, b, t, h, 64)).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------
# hcir_attn_cls_fwd_lse / hcir_attn_cls_bwd: one wave per (image, head), four per workgroup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h", [(1, 1), (1, 2), (3, 1), (5, 1), (26, 12)])   # 1, 2, 3, 1 live waves in the last workgroup; 312
@pytest.mark.parametrize("t", [1, 5, 63, 64, 65, 193, 197, 256])
def test_cls_fwd_bwd(L, t, b, h):
    """Contract of hcir_attn_cls_bwd (include/hcir.h): dK and dV of every token, dQ of token 0, and ZERO written to the
    dQ of tokens 1 .. T-1."""
    scale = _scale(64)
    for fam in ("flat", "marker_last", "negdom"):
        qd = oa.make_qkv(fam, b, t, h, 64).cuda()
        dout = oa.make_dout(b, 1, h, 64).cuda()

        def fwd():
            out, lse = Guarded((b, h * 64), torch.float16), Guarded((b, h), torch.float32)
            assert L.hcir_attn_cls_fwd_lse(qd.data_ptr(), b, t, h, 64, scale, out.ptr(), lse.ptr(), _st()) == 0
            return out.check(), lse.check()
        out, lse = _twice(fwd)

        def bwd():
            dqkv = Guarded((b, t, 3, h, 64), torch.float16)
            assert L.hcir_attn_cls_bwd(qd.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), b, t, h, 64,
                                       scale, dqkv.ptr(), _st()) == 0
            return (dqkv.check(),)
        (dqkv,) = _twice(bwd)
        ref = oa.attention_f64(qd, b, t, h, 64, scale, dout, nq=1)
        bo, bl = oa.fwd_bounds(ref, "cls")
        bdq, bdk, bdv = oa.bwd_bounds(ref, bo, bl, "cls")
        d = dqkv.double().permute(2, 0, 3, 1, 4)
        o4 = oa.heads_of(out, b, 1, h, 64)
        r = {"o": oa.ratio(o4, ref.o, bo), "lse": oa.ratio(lse[..., None], ref.lse2, bl),
             "dq": oa.ratio(d[0][:, :, :1], ref.dq, bdq), "dk": oa.ratio(d[1], ref.dk, bdk),
             "dv": oa.ratio(d[2], ref.dv, bdv)}
        _note("cls", r, f"{fam} b{b} t{t} h{h}")
        _assert_within(r, fam)
        assert not bool(dqkv[:, 1:, 0].any()), "dQ of tokens 1 .. T-1 must be written as zero"
        # row 0 of the MFMA forward: other arithmetic, so not bit-equal; within the sum of the two bounds
        mo, ml = run_fwd(L, qd, b, t, h, 64, scale, t, with_lse=True)
        fo, fl = oa.fwd_bounds(ref, "mfma")
        assert oa.ratio(oa.heads_of(mo[:, :1], b, 1, h, 64), o4, bo + fo) <= 1.0
        assert oa.ratio(ml[:, :, :1], lse[..., None].double(), bl + fl) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# every status an entry point can return before it launches anything
# ---------------------------------------------------------------------------------------------------------------
_FWD_BAD = [("qkv", 0, INVALID), ("out", 0, INVALID), ("b", 0, INVALID), ("h", 0, INVALID), ("t", 0, INVALID),
            ("t", 289, UNSUPPORTED), ("hd", 72, UNSUPPORTED), ("b", 1 << 31, INVALID)]
_TRAIN_BAD = [("qkv", 0, INVALID), ("out", 0, INVALID), ("lse", 0, INVALID), ("b", 0, INVALID), ("h", 0, INVALID),
              ("t", 0, INVALID), ("t", 257, UNSUPPORTED), ("hd", 72, UNSUPPORTED), ("hd", 80, UNSUPPORTED),
              ("b", 1 << 31, INVALID)]
STATUS = ([("fwd", *c) for c in _FWD_BAD + [("nq", 0, INVALID), ("nq", 18, INVALID)]]
          + [("fwd_lse", *c) for c in _TRAIN_BAD if c[:2] != ("t", 257)] + [("fwd_lse", "t", 289, UNSUPPORTED)]
          + [("bwd", *c) for c in _TRAIN_BAD + [("dout", 0, INVALID), ("dqkv", 0, INVALID)]]
          + [("cls_fwd", *c) for c in _TRAIN_BAD]
          + [("cls_bwd", *c) for c in _TRAIN_BAD + [("dout", 0, INVALID), ("dqkv", 0, INVALID)]])


@pytest.mark.parametrize("entry,field,value,status", STATUS, ids=lambda v: str(v))
def test_status_before_launch(L, entry, field, value, status):
    """One bad argument at a time, all others valid (real buffers of a b = 1, t = 17, h = 1 problem).  Every call
    returns before a launch: the outputs keep their NaN prefill."""
    bufs = {"qkv": torch.zeros(17 * 3 * 64, dtype=torch.float16, device="cuda"),
            "out": torch.full((17 * 64,), float("nan"), dtype=torch.float16, device="cuda"),
            "dout": torch.zeros(17 * 64, dtype=torch.float16, device="cuda"),
            "lse": torch.full((17,), float("nan"), dtype=torch.float32, device="cuda"),
            "dqkv": torch.full((17 * 3 * 64,), float("nan"), dtype=torch.float16, device="cuda")}
    a = {k: v.data_ptr() for k, v in bufs.items()}
    a.update(b=1, t=17, h=1, hd=64, nq=17)
    a[field] = value
    sc = _scale(64)
    if entry == "fwd":
        got = L.hcir_attn_fwd(a["qkv"], a["b"], a["t"], a["h"], a["hd"], sc, a["nq"], a["out"], _st())
    elif entry == "fwd_lse":
        got = L.hcir_attn_fwd_lse(a["qkv"], a["b"], a["t"], a["h"], a["hd"], sc, a["out"], a["lse"], _st())
    elif entry == "cls_fwd":
        got = L.hcir_attn_cls_fwd_lse(a["qkv"], a["b"], a["t"], a["h"], a["hd"], sc, a["out"], a["lse"], _st())
    else:
        fn = L.hcir_attn_bwd if entry == "bwd" else L.hcir_attn_cls_bwd
        got = fn(a["qkv"], a["out"], a["dout"], a["lse"], a["b"], a["t"], a["h"], a["hd"], sc, a["dqkv"], _st())
    assert got == status
    torch.cuda.synchronize()
    writes = ("out", "lse") if entry in ("fwd", "fwd_lse", "cls_fwd") else ("dqkv",)
    assert all(bool(torch.isnan(bufs[k]).all()) for k in writes)
