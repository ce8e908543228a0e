"""hcir_msn_targets / hcir_msn_fwd / hcir_msn_bwd against float64, through the C ABI, between canaries.

Reference and bounds: tests/_msn_ref.py (the float64 restatement of lightly's MSNLoss pinned to torch's own ops by
tests/test_msn_host.py; bounds that count the kernels' roundings).  Every element of q, row_lse, pbar and danchors, both
loss parts and the loss satisfy err / bound <= 1 on every entry of _msn_ref.table() - the shapes, input families and
(sinkhorn_iterations, regularization_weight) corners - in fp32, fp16 and bf16; no entry is left out.  Two runs, one on
a zero-filled and one on a 0xFF-filled workspace of exactly the advertised size, are bit-identical; every refused call
returns its documented status and writes nothing.

The bounds are worst cases: at 1 / (T Ts) = 40 a prototype rounded to bf16 may move a target logit by 0.16 and the
Sinkhorn rounds may multiply that by 4 x iterations, so the 16-bit bounds of q after Sinkhorn (and of what depends on
it) allow errors of the size of the value; the fp32 bounds are below 2 % of it.  The observed errors are far inside.

Worst err / bound per quantity on an MI355X (fp32 / fp16 / bf16; with the entry of each: profiles/msn_errors.txt):

    q               row_lse         pbar            ce                 reg                loss               danchors
    0.10 0.33 0.42  0.09 0.23 0.32  0.04 0.25 0.27  .0009 .0005 .0005  .013 .003 .005     .0009 .0005 .0005  0.35 0.04 0.02
"""
import pytest
import torch

import _msn_ref as mr

pytestmark = pytest.mark.gpu

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
_PAD = 256
_CANARY = -1536.0     # exact in fp32, fp16 and bf16
_WS_CANARY = 0xA5
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _guarded(n, dtype, canary):
    full = torch.full((n + 2 * _PAD,), canary, dtype=dtype, device="cuda")
    return full, full[_PAD:_PAD + n]


def _pads_intact(full, n, canary):
    return bool((full[:_PAD] == canary).all()) and bool((full[_PAD + n:] == canary).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


class _MsnCall:
    """One problem on the device, outputs between canaries, workspaces of exactly the advertised size."""

    def __init__(self, case, anchors, targets, protos, dtype, iterations, weight, ws_fill=0x00):
        from hcir import _lib
        from hcir.ops import _DT
        self.L, self.dt, self.dtype = _lib.lib(), _DT[dtype], dtype
        self.b, self.v, self.k, self.d = case
        self.n = self.b * self.v
        self.iterations, self.weight = iterations, weight
        self.a, self.t, self.c = anchors.cuda(), targets.cuda(), protos.cuda()
        self.st = torch.cuda.current_stream().cuda_stream
        self.bytes = [self.L.hcir_msn_workspace_bytes(self.b if s == 0 else self.n, self.k, self.d, self.dt, s)
                      for s in range(3)]
        self.q_full, self.q = _guarded(self.b * self.k, torch.float32, _CANARY)
        self.loss_full, self.loss = _guarded(1, torch.float32, _CANARY)
        self.parts_full, self.parts = _guarded(2, torch.float32, _CANARY)
        self.lse_full, self.lse = _guarded(self.n, torch.float32, _CANARY)
        self.pbar_full, self.pbar = _guarded(self.k, torch.float32, _CANARY)
        self.da_full, self.da = _guarded(self.n * self.d, dtype, _CANARY)
        self.ws_fill = ws_fill

    def workspace(self, nbytes):
        full, ws = _guarded(nbytes, torch.uint8, _WS_CANARY)
        ws.fill_(self.ws_fill)
        return full, ws

    def fulls(self):
        return (self.q_full, self.loss_full, self.parts_full, self.lse_full, self.pbar_full, self.da_full)

    def outputs_untouched(self):
        torch.cuda.synchronize()
        return all(bool((f == _CANARY).all()) for f in self.fulls())

    def targets(self, ws, ws_bytes, b=None, k=None, d=None, dt=None, inv=None, it=None, t="own", q="own"):
        return self.L.hcir_msn_targets(
            self.t.data_ptr() if t == "own" else t, self.c.data_ptr(), self.b if b is None else b,
            self.k if k is None else k, self.d if d is None else d, self.dt if dt is None else dt,
            1.0 / (mr.T_DEFAULT * mr.TS_DEFAULT) if inv is None else inv, self.iterations if it is None else it,
            self.q.data_ptr() if q == "own" else q, None if ws is None else ws.data_ptr(), ws_bytes, self.st)

    def fwd(self, ws, ws_bytes, n=None, b=None, k=None, d=None, dt=None, inv=None, a="own", loss="own", q="own",
            optional=True):
        return self.L.hcir_msn_fwd(
            self.a.data_ptr() if a == "own" else a, self.c.data_ptr(), self.q.data_ptr() if q == "own" else q,
            self.n if n is None else n, self.b if b is None else b, self.k if k is None else k,
            self.d if d is None else d, self.dt if dt is None else dt, 1.0 / mr.T_DEFAULT if inv is None else inv,
            self.weight, self.loss.data_ptr() if loss == "own" else loss, self.parts.data_ptr() if optional else None,
            self.lse.data_ptr() if optional else None, self.pbar.data_ptr() if optional else None,
            None if ws is None else ws.data_ptr(), ws_bytes, self.st)

    def bwd(self, ws, ws_bytes, n=None, b=None, k=None, d=None, dt=None, inv=None, da="own", lse="own", pbar="own"):
        return self.L.hcir_msn_bwd(
            self.a.data_ptr(), self.c.data_ptr(), self.q.data_ptr(), self.n if n is None else n,
            self.b if b is None else b, self.k if k is None else k, self.d if d is None else d,
            self.dt if dt is None else dt, 1.0 / mr.T_DEFAULT if inv is None else inv, self.weight,
            self.lse.data_ptr() if lse == "own" else lse, self.pbar.data_ptr() if pbar == "own" else pbar, 1.0,
            self.da.data_ptr() if da == "own" else da, None if ws is None else ws.data_ptr(), ws_bytes, self.st)

    def run(self):
        """targets, forward, backward once; asserts the buffer discipline; returns the outputs' bit patterns."""
        for stage, call in ((0, self.targets), (1, self.fwd), (2, self.bwd)):
            ws_full, ws = self.workspace(self.bytes[stage])
            assert call(ws, self.bytes[stage]) == 0
            torch.cuda.synchronize()
            assert _pads_intact(ws_full, self.bytes[stage], _WS_CANARY)
        views = (self.q, self.loss, self.parts, self.lse, self.pbar, self.da)
        for full, view in zip(self.fulls(), views):
            assert _pads_intact(full, view.numel(), _CANARY)
            assert bool((view != _CANARY).all())
        return [_bits(x) for x in views]

    def outputs(self):
        return {"q": self.q.view(self.b, self.k).cpu(), "row_lse": self.lse.cpu(), "pbar": self.pbar.cpu(),
                "ce": self.parts[0].cpu(), "reg": self.parts[1].cpu(), "loss": self.loss[0].cpu(),
                "danchors": self.da.view(self.n, self.d).cpu()}


_RUNS = [(c, dt) for c in mr.CASES for dt in mr.DTYPES]


@pytest.mark.parametrize("case,dtype", _RUNS, ids=["-".join(str(x) for x in c) + f"-{_NAME[dt]}" for c, dt in _RUNS])
def test_msn_vs_f64(case, dtype):
    """Every quantity on every (family, iterations, weight) entry of the table for this shape; two runs on differently
    filled workspaces are bit-identical."""
    entries = [e for e in mr.table() if e[0] == case]
    assert len(entries) == sum(len(mr.CONFIGS[f]) for f in mr.FAMILIES)
    for _, family, iterations, weight in entries:
        anchors, targets, protos = mr.make_inputs(case, family, dtype)
        ref = mr.msn_f64(anchors, targets, protos, iterations=iterations, weight=weight)
        gref = mr.grads_f64(anchors, targets, protos, iterations=iterations, weight=weight)
        bd = mr.bounds(ref, anchors, targets, dtype, iterations=iterations, weight=weight)
        c = _MsnCall(case, anchors, targets, protos, dtype, iterations, weight, 0x00)
        first = c.run()
        out = c.outputs()
        for name in ("q", "row_lse", "pbar", "ce", "reg", "loss"):
            assert bool(torch.isfinite(out[name]).all()), (family, name)
        r = mr.verdicts(out, ref, bd, gref, dtype)
        assert set(r) == set(mr.QUANTITIES)
        print(f"\nmsn {case} {_NAME[dtype]} {family} it={iterations} w={weight}: "
              + " ".join(f"{q} {v:.4f}" for q, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), (family, iterations, weight, r)
        second = _MsnCall(case, anchors, targets, protos, dtype, iterations, weight, 0xFF).run()
        for name, x, y in zip(("q", "loss", "parts", "row_lse", "pbar", "danchors"), first, second):
            assert torch.equal(x, y), (family, name)


def test_msn_optional_outputs_may_be_null():
    """loss_parts, row_lse and pbar are optional: the loss is the same bits without them."""
    case, dtype = (5, 3, 136, 8), torch.float16
    anchors, targets, protos = mr.make_inputs(case, "gauss", dtype)
    c = _MsnCall(case, anchors, targets, protos, dtype, 3, 1.0)
    c.run()
    full = c.loss.clone()
    c.loss.fill_(_CANARY)
    _, ws = c.workspace(c.bytes[1])
    assert c.fwd(ws, c.bytes[1], optional=False) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(c.loss), _bits(full))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_msn_error_statuses_write_nothing(dtype):
    """Every refused call returns its documented status (include/hcir.h) and leaves every output untouched."""
    case = (5, 3, 136, 8)
    anchors, targets, protos = mr.make_inputs(case, "gauss", dtype)
    c = _MsnCall(case, anchors, targets, protos, dtype, 3, 1.0)
    big = max(c.bytes)
    ws = torch.zeros(big, dtype=torch.uint8, device="cuda")
    refused = [
        ("targets workspace one byte short", c.targets(ws, c.bytes[0] - 1), WORKSPACE),
        ("fwd workspace one byte short", c.fwd(ws, c.bytes[1] - 1), WORKSPACE),
        ("bwd workspace one byte short", c.bwd(ws, c.bytes[2] - 1), WORKSPACE),
        ("targets null workspace", c.targets(None, big), WORKSPACE),
        ("fwd null workspace", c.fwd(None, big), WORKSPACE),
        ("bwd null workspace", c.bwd(None, big), WORKSPACE),
        ("targets d = 12", c.targets(ws, big, d=12), INVALID),
        ("fwd d = 12", c.fwd(ws, big, d=12), INVALID),
        ("bwd d = 12", c.bwd(ws, big, d=12), INVALID),
        ("targets b = 0", c.targets(ws, big, b=0), INVALID),
        ("targets k = 0", c.targets(ws, big, k=0), INVALID),
        ("targets iterations = -1", c.targets(ws, big, it=-1), INVALID),
        ("targets inv = 0", c.targets(ws, big, inv=0.0), INVALID),
        ("targets inv = nan", c.targets(ws, big, inv=float("nan")), INVALID),
        ("targets null targets", c.targets(ws, big, t=None), INVALID),
        ("targets null q", c.targets(ws, big, q=None), INVALID),
        ("fwd n = 0", c.fwd(ws, big, n=0), INVALID),
        ("fwd n % b", c.fwd(ws, big, n=14), INVALID),
        ("fwd b = 0", c.fwd(ws, big, b=0), INVALID),
        ("fwd null anchors", c.fwd(ws, big, a=None), INVALID),
        ("fwd null q", c.fwd(ws, big, q=None), INVALID),
        ("fwd null loss", c.fwd(ws, big, loss=None), INVALID),
        ("fwd inv_t = 0", c.fwd(ws, big, inv=0.0), INVALID),
        ("bwd k = 132", c.bwd(ws, big, k=132), INVALID),
        ("bwd n % b", c.bwd(ws, big, n=14), INVALID),
        ("bwd null danchors", c.bwd(ws, big, da=None), INVALID),
        ("bwd null row_lse", c.bwd(ws, big, lse=None), INVALID),
        ("bwd null pbar", c.bwd(ws, big, pbar=None), INVALID),
        ("bwd inv_t = nan", c.bwd(ws, big, inv=float("nan")), INVALID),
        ("targets dtype 7", c.targets(ws, big, dt=7), UNSUPPORTED),
        ("fwd dtype 7", c.fwd(ws, big, dt=7), UNSUPPORTED),
        ("bwd dtype 7", c.bwd(ws, big, dt=7), UNSUPPORTED),
    ]
    for name, got, want in refused:
        assert got == want, (name, got, want)
    assert c.outputs_untouched()
    assert c.L.hcir_msn_workspace_bytes(0, 8, 8, c.dt, 0) == 0
    assert c.L.hcir_msn_workspace_bytes(8, 8, 8, c.dt, 3) == 0
