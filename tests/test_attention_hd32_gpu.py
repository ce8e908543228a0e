"""GPU: hcir_attn_fwd_lse and hcir_attn_bwd at head_dim 32 (the MAE decoder: 512 / 16 heads), every element against
oracle.attention's float64 reference through the per-element bounds derived there, which are parametric in the head
dim.  The forward is attn_fwd_generic_kernel<32, NKT> (now also writing the log2-sum-exp), the backward is
attn_bwd32_kernel (csrc/attn_bwd32.hip), whose arithmetic per element is attn_bwd_kernel's with 32-term dim
contractions: the derivation in oracle/attention.py ("Backward, MFMA kernels") applies as written, no bound of its own.

Every case, as tests/test_attention_gpu.py: outputs prefilled with NaN and required finite, every output buffer between
canary blocks, two runs bit-equal, the backward fed the forward kernel's own out and lse.  Token counts: one key tile,
ragged and exact last tiles, 49 (the kept tokens of MAE's encoder run at head_dim 64, but the count is a natural edge),
197, and the full 256; every input family of oracle.attention at every count.  The kernel is not persistent (one
workgroup per (image, head)); one case still runs 16 x 16 items and asks for the bits of one image per call.

Worst err / bound on an MI355X over all cases: O 0.633, lse 0.097, dQ 0.737, dK 0.362, dV 0.673 (profiles/mae_errors.txt
has every case; no bound was changed after the first GPU run)."""
import pytest
import torch

from oracle import attention as oa

pytestmark = pytest.mark.gpu

HD = 32
UNSUPPORTED = -2
CANARY, PAD = 1234.0, 4096
T_ALL = [1, 17, 32, 33, 49, 65, 129, 193, 197, 224, 225, 256]
WORST = {}


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\nhead_dim 32 attention, worst err / bound per output:")
    for name, val in sorted(WORST.items()):
        print(f"attn32-worst {name:4s} {val:.3f}")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _scale():
    return oa.f32(HD ** -0.5)


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
    first, second = fn(), fn()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "two runs differ"
    return first


def run_fwd_lse(L, qd, b, t, h):
    def once():
        out, lse = Guarded((b, t, h * HD), torch.float16), Guarded((b, h, t), torch.float32)
        assert L.hcir_attn_fwd_lse(qd.data_ptr(), b, t, h, HD, _scale(), out.ptr(), lse.ptr(), _st()) == 0
        return out.check(), lse.check()
    return _twice(once)


def run_fwd(L, qd, b, t, h):
    out = Guarded((b, t, h * HD), torch.float16)
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, HD, _scale(), t, out.ptr(), _st()) == 0
    return out.check()


def run_bwd(L, qd, out, dout, lse, b, t, h):
    def once():
        dqkv = Guarded((b, t, 3, h, HD), torch.float16)
        assert L.hcir_attn_bwd(qd.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), b, t, h, HD, _scale(),
                               dqkv.ptr(), _st()) == 0
        return (dqkv.check(),)
    return _twice(once)[0]


def _ratios(qd, out, lse, dout, dqkv, b, t, h):
    ref = oa.attention_f64(qd, b, t, h, HD, _scale(), dout)
    bo, bl = oa.fwd_bounds(ref)
    bdq, bdk, bdv = oa.bwd_bounds(ref, bo, bl)
    d = dqkv.double().permute(2, 0, 3, 1, 4)
    return {"o": oa.ratio(oa.heads_of(out, b, t, h, HD), ref.o, bo), "lse": oa.ratio(lse, ref.lse2, bl),
            "dq": oa.ratio(d[0], ref.dq, bdq), "dk": oa.ratio(d[1], ref.dk, bdk), "dv": oa.ratio(d[2], ref.dv, bdv)}


def _case(L, fam, b, t, h):
    qd = oa.make_qkv(fam, b, t, h, HD).cuda()
    dout = oa.make_dout(b, t, h, HD).cuda()
    out, lse = run_fwd_lse(L, qd, b, t, h)
    assert torch.equal(out, run_fwd(L, qd, b, t, h)), "hcir_attn_fwd_lse and hcir_attn_fwd differ"
    dqkv = run_bwd(L, qd, out, dout, lse, b, t, h)
    r = _ratios(qd, out, lse, dout, dqkv, b, t, h)
    print(f"\nattn32-err {fam} b{b} t{t} h{h}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert all(v <= 1.0 for v in r.values()), (fam, t, r)
    return qd, dout, out, lse, dqkv


@pytest.mark.parametrize("t", T_ALL)
def test_fwd_lse_and_bwd_every_family(L, t):
    for fam in oa.FAMILIES:
        _case(L, fam, 2, t, 3)


def test_single_head_single_image(L):
    for t in (1, 197):
        _case(L, "marker_last", 1, t, 1)


def test_many_items_equal_one_image_per_call(L):
    """16 images x 16 heads (the decoder's head count): the (image, head) of a workgroup, and the strides that follow
    from 16 heads of 32, against one image per call."""
    b, t, h = 16, 197, 16
    qd, dout, out, lse, dqkv = _case(L, "marker_first", b, t, h)
    for i in (0, 7, 15):
        o1, l1 = run_fwd_lse(L, qd[i:i + 1], 1, t, h)
        assert torch.equal(o1, out[i:i + 1]) and torch.equal(l1, lse[i:i + 1])
        one = run_bwd(L, qd[i:i + 1], out[i:i + 1], dout[i:i + 1], lse[i:i + 1], 1, t, h)
        assert torch.equal(one, dqkv[i:i + 1]), i


def test_exact_zero_ds(L):
    """uniform family, dout constant along the queries and confined to V's key-constant dims 0..3: dS = 0 in exact
    arithmetic, so dQ = dK = 0 and dV = dout; what is left of the bounds are their absolute terms."""
    b, t, h = 2, 197, 3
    dout = torch.zeros(b, t, h, HD)
    dout[..., :4] = torch.tensor([0.5, -0.25, 1.0, 0.125])
    dout = dout.reshape(b, t, h * HD).half().cuda()
    qd = oa.make_qkv("uniform", b, t, h, HD).cuda()
    out, lse = run_fwd_lse(L, qd, b, t, h)
    dqkv = run_bwd(L, qd, out, dout, lse, b, t, h)
    ref = oa.attention_f64(qd, b, t, h, HD, _scale(), dout)
    assert float(ref.dq.abs().max()) <= 1e-14 and float(ref.dk.abs().max()) <= 1e-14
    r = _ratios(qd, out, lse, dout, dqkv, b, t, h)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("hd,status", [(32, 0), (64, 0), (48, UNSUPPORTED), (96, UNSUPPORTED), (128, UNSUPPORTED)])
def test_training_head_dims(L, hd, status):
    """hd 32 and 64 train; every other head dim the forward serves keeps returning UNSUPPORTED from hcir_attn_fwd_lse
    and hcir_attn_bwd, before a launch (the outputs keep their NaN prefill)."""
    t = 17
    qkv = torch.zeros(t * 3 * hd, dtype=torch.float16, device="cuda")
    out = torch.full((t * hd,), float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full((t,), float("nan"), dtype=torch.float32, device="cuda")
    dqkv = torch.full((t * 3 * hd,), float("nan"), dtype=torch.float16, device="cuda")
    sc = oa.f32(hd ** -0.5)
    assert L.hcir_attn_fwd_lse(qkv.data_ptr(), 1, t, 1, hd, sc, out.data_ptr(), lse.data_ptr(), _st()) == status
    torch.cuda.synchronize()
    if status:
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all())
        lse.zero_()
        out.zero_()
    dout = torch.zeros(t * hd, dtype=torch.float16, device="cuda")
    assert L.hcir_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), 1, t, 1, hd, sc,
                           dqkv.data_ptr(), _st()) == status
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv).all()) == bool(status)
    if hd == 32:
        assert L.hcir_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), 1, 257, 1, hd, sc,
                               dqkv.data_ptr(), _st()) == UNSUPPORTED
