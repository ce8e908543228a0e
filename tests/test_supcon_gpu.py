"""hcir_supcon_fwd / hcir_supcon_bwd against float64, per row and per element, forward and backward.

Reference: tests/_supcon_ref.py (supcon_f64, pinned to the reference class by tests/golden/supcon_ref.npz; autograd for
the gradients) on the inputs after rounding to the tested dtype.  Bounds: lse_bound / loss_bound / grad_bound, derived
term by term there; every row's lse, the loss and every gradient element are held to them, row_npos exactly.  Cases
(B, V, D, T, T_base) sit around the 128-row tile edge and both staging paths (_supcon_ref.CASES); label families: none,
three classes, all one class, singletons and pairs (rows without positives at V = 1), classes {5, 5 + 2^32, -1}; input
families exact / norms / exact_norms of oracle.ntxent.make_inputs stacked to [B, V, D]; normalize off and on.

Without normalize the rows keep their norms (2^-6 .. 2^6 times sqrt(D) in "norms"): logits reach 1e6 and the softmax is
one-hot; the bounds scale every logit term with ||x_i|| ||x_j|| / |T| and hold there as well.  fp16 gradients of an
un-scaled loss reach the subnormal range, and at grad_out = 65536 some overflow to the infinity of the reference's
sign, as in tests/test_ntxent_gpu.py (oracle.ntxent.err_over_bound).

Worst err/bound per quantity (max over cases, families and label families; fp32 / fp16 / bf16) and the sharpness table
of tests/test_supcon_host.py: profiles/supcon_errors.txt.

                          lse                  loss                 grad
  CPU emulation     0.131 0.258 0.357    0.032 0.089 0.032    0.396 0.486 0.447
  MI355X kernels    0.123 0.258 0.357    0.031 0.089 0.027    0.396 0.486 0.447

The NT-Xent special case (labels None, normalize, T_base = T) against oracle.ntxent's own bounds on NT-Xent's cases:
lse 0.144 0.237 0.357, loss 0.058 0.058 0.058, grad 0.250 0.599 0.415.  The step on a Linear(24, 16): weight-gradient
error 1.154e-04 on the MI355X, 1.154e-04 in the emulation (|grad| max 0.329).
"""
import math

import pytest
import torch

import _supcon_ref as sc
from oracle import ntxent as ont

pytestmark = pytest.mark.gpu

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
_FWD = [(c, dt) for c in sc.CASES for dt in sc.case_dtypes(c)]
_BWD = [(c, dt) for c in sc.CASES if sc.has_backward(c) for dt in sc.case_dtypes(c)]


def _ids(pairs):
    return ["-".join(str(x) for x in c) + "-" + _NAME[dt] for c, dt in pairs]


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _forward(pr, case, normalize):
    from hcir.losses import supcon_forward
    f = pr.features.cuda()
    labels = None if pr.labels is None else pr.labels.cuda()
    loss, lse, npos = supcon_forward(f, labels, case[3], case[4], normalize, want_saved=True)
    return f, labels, loss, lse, npos


@pytest.mark.parametrize("case,dtype", _FWD, ids=_ids(_FWD))
def test_forward_rows_vs_f64(case, dtype):
    """Every row's lse and positive count and the loss, on every input family, label family and normalize setting."""
    b, v, d, t, tb = case
    worst_lse = worst_loss = 0.0
    for normalize in (False, True):
        for lab in sc.LABEL_FAMILIES:
            for fam in sc.MAIN_FAMILIES:
                pr = sc.problem(fam, lab, case, dtype, normalize)
                _, _, loss, lse, npos = _forward(pr, case, normalize)
                what = (fam, lab, normalize)
                assert math.isfinite(loss.item()) and bool(torch.isfinite(lse).all()), what
                assert torch.equal(npos.cpu().long(), pr.ref.npos), what
                r_lse = sc.err_over_bound(lse.cpu(), pr.ref.lse, sc.lse_bound(pr.ref, t, pr.u_in))
                r_loss = sc.err_over_bound(loss.cpu(), pr.ref.loss, sc.loss_bound(pr.ref, t, tb, pr.u_in))
                print(f"\nsupcon fwd {case} {_NAME[dtype]} {fam} {lab} normalize={int(normalize)}: "
                      f"lse {r_lse:.3f} loss {r_loss:.3f}")
                assert r_lse <= 1.0 and r_loss <= 1.0, what
                worst_lse, worst_loss = max(worst_lse, r_lse), max(worst_loss, r_loss)
                if not bool((pr.ref.npos > 0).any()):    # no row has a positive: exactly 0, not merely small
                    assert loss.item() == 0.0, what
    print(f"\nsupcon fwd {case} {_NAME[dtype]} WORST: lse {worst_lse:.3f} loss {worst_loss:.3f}")


@pytest.mark.parametrize("case,dtype", _BWD, ids=_ids(_BWD))
def test_backward_elements_vs_f64(case, dtype):
    """Every element of d features at grad_out = 1 and 65536 (GradScaler's initial scale, what the step passes)."""
    from hcir.losses import supcon_backward
    b, v, d, t, tb = case
    worst = 0.0
    for normalize in (False, True):
        for lab in sc.LABEL_FAMILIES:
            for fam in sc.MAIN_FAMILIES:
                pr = sc.problem(fam, lab, case, dtype, normalize)
                f, labels, _, lse, npos = _forward(pr, case, normalize)
                for go in (1.0, 65536.0):
                    got = sc.rows_of(supcon_backward(f, labels, t, tb, normalize, lse, npos, go).cpu())
                    bound = sc.grad_bound(pr.ref, pr.features, pr.dx * go, t, tb, normalize, go, dtype, pr.u_in)
                    r = sc.err_over_bound(got, pr.dx * go, bound, dtype)
                    print(f"\nsupcon bwd {case} {_NAME[dtype]} {fam} {lab} normalize={int(normalize)} "
                          f"grad_out {go:g}: grad {r:.3f}")
                    assert r <= 1.0, (fam, lab, normalize, go)
                    worst = max(worst, r)
                    if not bool((pr.ref.npos > 0).any()):
                        assert float(got.abs().max()) == 0.0
    print(f"\nsupcon bwd {case} {_NAME[dtype]} WORST: grad {worst:.3f}")


_NT = [(c, dt) for c in ont.FWD_CASES for dt in ont.case_dtypes(c)]


@pytest.mark.parametrize("case,dtype", _NT, ids=[f"{c[0]}-{c[1]}-{c[2]}-{_NAME[dt]}" for c, dt in _NT])
def test_special_case_inside_ntxent_bounds(case, dtype):
    """labels None, normalize, T_base = T, V = 2 is NT-Xent: held to oracle.ntxent's own bounds of ntxent_f64, on
    NT-Xent's own cases (N = 2B: backward where N % 8 == 0, NT-Xent's BWD_CASES)."""
    from hcir.losses import supcon_backward, supcon_forward
    b, d, t = case
    for fam in ont.MAIN_FAMILIES:
        pr = ont.problem(fam, case, dtype)
        f = torch.stack([pr.z0, pr.z1], 1).contiguous().cuda()
        loss, lse, npos = supcon_forward(f, None, t, t, True, want_saved=True)
        assert bool((npos == 1).all())
        r_lse = ont.err_over_bound(lse.cpu(), pr.ref.lse, ont.lse_bound(pr.ref.lse, t, pr.u_in))
        r_loss = ont.err_over_bound(loss.cpu(), pr.ref.loss, ont.loss_bound(pr.ref.loss, t, pr.u_in))
        r = 0.0
        if case in ont.BWD_CASES:
            got = sc.rows_of(supcon_backward(f, None, t, t, True, lse, npos, 1.0).cpu())
            bound = ont.grad_bound(pr.ref, pr.x, pr.dz, t, 1.0, dtype, pr.u_in)
            r = ont.err_over_bound(got, pr.dz, bound, dtype)
        print(f"\nsupcon as ntxent {case} {_NAME[dtype]} {fam}: lse {r_lse:.3f} loss {r_loss:.3f} grad {r:.3f}")
        assert r_lse <= 1.0 and r_loss <= 1.0 and r <= 1.0, fam


def test_autograd_path_noncontiguous_fp16():
    """SupConLoss(...)(x, labels) then (loss * 3).backward(): a column-sliced view in, one host read of the upstream
    grad; a 4-D input is flattened to [B, V, -1]; labels given as a column [B, 1] as the reference allows"""
    from hcir.losses import SupConLoss
    case, dtype = (68, 2, 72, .2, .1), torch.float16
    b, v, d, t, tb = case
    for normalize in (False, True):
        pr = sc.problem("norms", "three", case, dtype, normalize)
        base = torch.zeros(b, v, d + 8, dtype=dtype)
        base[:, :, 4:4 + d] = pr.features
        base = base.cuda().requires_grad_(True)
        x = base[:, :, 4:4 + d]
        assert not x.is_contiguous()
        loss = SupConLoss(t, "all", tb, normalize=normalize)(x, pr.labels.view(-1, 1).cuda())
        (loss * 3).backward()
        r_loss = sc.err_over_bound(loss.detach().cpu(), pr.ref.loss, sc.loss_bound(pr.ref, t, tb, pr.u_in))
        got = base.grad.cpu()
        bound = sc.grad_bound(pr.ref, pr.features, pr.dx * 3.0, t, tb, normalize, 3.0, dtype, pr.u_in)
        r = sc.err_over_bound(sc.rows_of(got[:, :, 4:4 + d]), pr.dx * 3.0, bound, dtype)
        print(f"\nsupcon autograd {case} fp16 normalize={int(normalize)}: loss {r_loss:.3f} grad {r:.3f}")
        assert r_loss <= 1.0 and r <= 1.0
        assert float(got[:, :, :4].abs().max()) == 0.0 and float(got[:, :, 4 + d:].abs().max()) == 0.0
        # [B, V, 8, 9] -> [B, V, 72]; no grad: the forward alone
        with torch.no_grad():
            loss4 = SupConLoss(t, "all", tb, normalize=normalize)(pr.features.view(b, v, 8, 9).cuda(), pr.labels.cuda())
        assert loss4.item() == loss.item()


def test_module_refuses_backward_with_n_not_multiple_of_8():
    from hcir import HcirError
    from hcir.losses import SupConLoss
    x = torch.randn(37, 2, 32, device="cuda", requires_grad=True)
    with pytest.raises(HcirError, match="multiple of 8"):
        SupConLoss()(x)
    assert math.isfinite(SupConLoss()(x.detach()).item())


# ------------------------------------------------------------------ buffer discipline, determinism, statuses (C ABI)
_PAD = 256
_CANARY = -1536.0     # exact in fp32, fp16 and bf16
_ICANARY = -77
_WS_CANARY = 0xA5


def _guarded(n, dtype, canary):
    """(whole tensor, the n-element slice between two canary pads)."""
    full = torch.full((n + 2 * _PAD,), canary, dtype=dtype, device="cuda")
    return full, full[_PAD:_PAD + n]


def _pads_intact(full, n, canary):
    return bool((full[:_PAD] == canary).all()) and bool((full[_PAD + n:] == canary).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


class _Call:
    """One forward + backward through the C ABI with canaries around every output and an exactly sized workspace."""

    def __init__(self, pr, case, dtype, normalize):
        from hcir import _lib
        from hcir.ops import _DT
        self.L, self.dt = _lib.lib(), _DT[dtype]
        self.b, self.v, self.d, self.t, self.tb = case
        self.n = self.b * self.v
        self.normalize = int(normalize)
        self.f = pr.features.cuda()
        self.labels = None if pr.labels is None else pr.labels.cuda()
        self.st = torch.cuda.current_stream().cuda_stream
        self.fwd_bytes = self.L.hcir_supcon_workspace_bytes(self.b, self.v, self.d, self.dt, 0)
        self.bwd_bytes = self.L.hcir_supcon_workspace_bytes(self.b, self.v, self.d, self.dt, 1)
        self.loss_full, self.loss = _guarded(1, torch.float32, _CANARY)
        self.lse_full, self.lse = _guarded(self.n, torch.float32, _CANARY)
        self.npos_full, self.npos = _guarded(self.n, torch.int32, _ICANARY)
        self.df_full, self.df = _guarded(self.n * self.d, dtype, _CANARY)

    def _lab(self):
        return None if self.labels is None else self.labels.data_ptr()

    def outputs_untouched(self):
        torch.cuda.synchronize()
        return all(bool((f == _CANARY).all()) for f in (self.loss_full, self.lse_full, self.df_full)) \
            and bool((self.npos_full == _ICANARY).all())

    def fwd(self, ws, ws_bytes, b=None, v=None, d=None, dt=None, inv_t=None, loss="own", feat="own"):
        return self.L.hcir_supcon_fwd(self.f.data_ptr() if feat == "own" else feat, self._lab(),
                                      self.b if b is None else b, self.v if v is None else v,
                                      self.d if d is None else d, self.dt if dt is None else dt,
                                      1.0 / self.t if inv_t is None else inv_t, self.t / self.tb, self.normalize,
                                      self.loss.data_ptr() if loss == "own" else loss, self.lse.data_ptr(),
                                      self.npos.data_ptr(), ws.data_ptr(), ws_bytes, self.st)

    def bwd(self, lse, npos, ws, ws_bytes, b=None, v=None, d=None, dt=None, inv_t=None, df="own", npos_ptr="own"):
        return self.L.hcir_supcon_bwd(self.f.data_ptr(), self._lab(), self.b if b is None else b,
                                      self.v if v is None else v, self.d if d is None else d,
                                      self.dt if dt is None else dt, 1.0 / self.t if inv_t is None else inv_t,
                                      1.0 / self.tb, self.normalize, lse.data_ptr(),
                                      npos.data_ptr() if npos_ptr == "own" else npos_ptr, 1.0,
                                      self.df.data_ptr() if df == "own" else df, ws.data_ptr(), ws_bytes, self.st)


_BUF = [(c, dt, nz) for c in ((68, 2, 72, .2, .1), (132, 2, 8, .2, .07), (136, 1, 64, .3, .07))
        for dt in (torch.float16, torch.float32) for nz in (False, True)]


@pytest.mark.parametrize("case,dtype,normalize", _BUF,
                         ids=["-".join(str(x) for x in c) + f"-{_NAME[dt]}-nz{int(nz)}" for c, dt, nz in _BUF])
def test_canaries_exact_workspace_stale_workspace_and_determinism(case, dtype, normalize):
    """Outputs and workspace are slices with canaries on both sides, the workspace exactly as long as
    hcir_supcon_workspace_bytes says; every output element is written; a zero-filled and a 0xFF-filled (NaN patterns)
    workspace give bit-equal loss, lse, npos and d features - the production workspace is shared with every other op
    and always stale - which is also the run-to-run determinism the kernel file's header claims."""
    pr = sc.problem("norms", "mixed", case, dtype, normalize)
    runs = []
    for fill in (0x00, 0xFF):
        c = _Call(pr, case, dtype, normalize)
        ws_full, ws = _guarded(c.fwd_bytes, torch.uint8, _WS_CANARY)
        ws.fill_(fill)
        assert c.fwd(ws, c.fwd_bytes) == 0
        torch.cuda.synchronize()
        assert _pads_intact(ws_full, c.fwd_bytes, _WS_CANARY)
        assert _pads_intact(c.loss_full, 1, _CANARY) and _pads_intact(c.lse_full, c.n, _CANARY)
        assert _pads_intact(c.npos_full, c.n, _ICANARY)
        assert bool((c.lse != _CANARY).all()) and bool((c.loss != _CANARY).all()) and bool((c.npos != _ICANARY).all())
        assert bool(torch.isfinite(c.lse).all()) and bool(torch.isfinite(c.loss).all())
        ws_full, ws = _guarded(c.bwd_bytes, torch.uint8, _WS_CANARY)
        ws.fill_(fill)
        lse, npos = c.lse.clone(), c.npos.clone()
        assert c.bwd(lse, npos, ws, c.bwd_bytes) == 0
        torch.cuda.synchronize()
        assert _pads_intact(ws_full, c.bwd_bytes, _WS_CANARY)
        assert _pads_intact(c.df_full, c.n * c.d, _CANARY)
        assert bool((c.df != _CANARY).all()) and bool(torch.isfinite(c.df).all())
        assert _pads_intact(c.lse_full, c.n, _CANARY) and _pads_intact(c.loss_full, 1, _CANARY)
        runs.append([_bits(x) for x in (c.loss, c.lse, c.npos, c.df)])
        t, tb = case[3], case[4]
        assert torch.equal(c.npos.cpu().long(), pr.ref.npos)
        r_lse = sc.err_over_bound(c.lse.cpu(), pr.ref.lse, sc.lse_bound(pr.ref, t, pr.u_in))
        r_loss = sc.err_over_bound(c.loss[0].cpu(), pr.ref.loss, sc.loss_bound(pr.ref, t, tb, pr.u_in))
        bound = sc.grad_bound(pr.ref, pr.features, pr.dx, t, tb, normalize, 1.0, dtype, pr.u_in)
        r = sc.err_over_bound(sc.rows_of(c.df.view(c.b, c.v, c.d).cpu()), pr.dx, bound, dtype)
        print(f"\nsupcon abi {case} {_NAME[dtype]} ws fill {fill:#04x}: lse {r_lse:.3f} loss {r_loss:.3f} grad {r:.3f}")
        assert r_lse <= 1.0 and r_loss <= 1.0 and r <= 1.0
    for name, x, y in zip(("loss", "lse", "npos", "dfeat"), *runs):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_error_statuses_write_nothing(dtype):
    """Every refused call returns its documented status (include/hcir.h) and leaves every output untouched"""
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    case = (68, 2, 72, .2, .1)
    c = _Call(sc.problem("norms", "three", case, dtype, False), case, dtype, False)
    ws = torch.zeros(max(c.bwd_bytes, c.fwd_bytes), dtype=torch.uint8, device="cuda")
    big = ws.numel()
    lse = torch.zeros(c.n, device="cuda")
    npos = torch.ones(c.n, dtype=torch.int32, device="cuda")
    refused = [
        ("fwd workspace one byte short", c.fwd(ws, c.fwd_bytes - 1), WORKSPACE),
        ("bwd workspace one byte short", c.bwd(lse, npos, ws, c.bwd_bytes - 1), WORKSPACE),
        ("fwd d = 12", c.fwd(ws, big, d=12), INVALID),
        ("bwd d = 12", c.bwd(lse, npos, ws, big, d=12), INVALID),
        ("fwd b = 0", c.fwd(ws, big, b=0), INVALID),
        ("fwd v = 0", c.fwd(ws, big, v=0), INVALID),
        ("fwd N = 1", c.fwd(ws, big, b=1, v=1), INVALID),
        ("bwd N = 12", c.bwd(lse, npos, ws, big, b=6), INVALID),
        ("bwd N = 9", c.bwd(lse, npos, ws, big, b=3, v=3), INVALID),
        ("fwd null features", c.fwd(ws, big, feat=None), INVALID),
        ("fwd null loss", c.fwd(ws, big, loss=None), INVALID),
        ("bwd null dfeat", c.bwd(lse, npos, ws, big, df=None), INVALID),
        ("bwd null row_npos", c.bwd(lse, npos, ws, big, npos_ptr=None), INVALID),
        ("fwd inv_t = 0", c.fwd(ws, big, inv_t=0.0), INVALID),
        ("bwd inv_t = 0", c.bwd(lse, npos, ws, big, inv_t=0.0), INVALID),
        ("fwd inv_t = NaN", c.fwd(ws, big, inv_t=float("nan")), INVALID),
        ("bwd inv_t = NaN", c.bwd(lse, npos, ws, big, inv_t=float("nan")), INVALID),
        ("fwd dtype 7", c.fwd(ws, big, dt=7), UNSUPPORTED),
        ("bwd dtype 7", c.bwd(lse, npos, ws, big, dt=7), UNSUPPORTED),
    ]
    for what, status, want in refused:
        assert status == want, (what, status)
    assert c.outputs_untouched()
    assert float(ws.max()) == 0.0     # nor the workspace
    # the same object still serves a valid call
    assert c.fwd(ws, c.fwd_bytes) == 0 and c.bwd(c.lse.clone(), c.npos.clone(), ws, c.bwd_bytes) == 0
    torch.cuda.synchronize()
    assert bool((c.lse != _CANARY).all()) and bool((c.df != _CANARY).all()) and bool((c.npos != _ICANARY).all())


# ------------------------------------------------------------------ the step
def test_supcon_train_step_on_a_tiny_linear_model():
    """SupConTrainStep (two views through one model call, stack, criterion with labels, backward, step, zero_grad) on a
    Linear(24, 16): the loss inside loss_bound of the float64 loss of the features the model produced, and the weight
    gradient's error at most 2x the error the emulation of the kernels' arithmetic makes on the same features."""
    from hcir.losses import SupConLoss
    from hcir.pretrain_engine import SupConTrainStep
    b, k, p, t, tb = 36, 24, 16, 0.07, 0.07
    g = torch.Generator().manual_seed(5)
    anchor, pos1 = torch.randn(b, k, generator=g), torch.randn(b, k, generator=g)
    labels = sc.make_labels("three", b)
    model = torch.nn.Linear(k, p, bias=False)
    with torch.no_grad():
        model.weight.copy_(torch.randn(p, k, generator=g) * 0.2)
    w0 = model.weight.detach().clone()
    model = model.cuda()
    seen = {}

    class Sgd(torch.optim.SGD):       # keeps the gradient the step is about to zero
        def step(self, *a, **kw):
            seen["grad"] = model.weight.grad.detach().clone()
            return super().step(*a, **kw)

    model.register_forward_hook(lambda mod, args, out: seen.__setitem__("features", out.detach().clone()))
    opt = Sgd(model.parameters(), lr=0.125)
    step = SupConTrainStep(model, opt, None, SupConLoss(t, "all", tb, normalize=True))
    out = step({"anchor": anchor.cuda(), "pos1": pos1.cuda(), "labels": labels.cuda()}, epoch=0, batch_id=0)
    assert set(out) == {"loss"} and isinstance(out["loss"], float)
    assert model.weight.grad is None or float(model.weight.grad.abs().max()) == 0.0     # zero_grad ran
    images = torch.cat([anchor, pos1], 0)
    feats = seen["features"].float().cpu()                             # what the model produced
    f = torch.stack(torch.split(feats, [b, b], 0), 1).contiguous()
    ref = sc.supcon_f64(f, labels, t, tb, True, full=True)
    u_in = sc.U_ROUND[torch.float32]
    assert abs(out["loss"] - float(ref.loss)) <= float(sc.loss_bound(ref, t, tb, u_in))
    dref = sc.rows_of(sc.supcon_grad_f64(f, labels, t, tb, True))
    demu = sc.rows_of(sc.emulate(f, labels, t, tb, True)[3]).double()
    wg_ref, wg_emu = dref.t() @ images.double(), demu.t() @ images.double()
    err_gpu = float((seen["grad"].cpu().double() - wg_ref).abs().max())
    err_emu = float((wg_emu - wg_ref).abs().max())
    print(f"\nsupcon step: loss {out['loss']:.6f} weight-grad error GPU {err_gpu:.3e} emulation {err_emu:.3e} "
          f"(|grad| max {float(wg_ref.abs().max()):.3e})")
    assert err_gpu <= 2.0 * err_emu
    assert torch.equal(model.weight.detach().cpu(), (w0.cuda() - 0.125 * seen["grad"]).cpu())    # the optimizer stepped
