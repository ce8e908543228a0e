"""hcir_ntxent_fwd / hcir_ntxent_bwd against float64, per row and per element, forward and backward.

Reference: oracle.ntxent.ntxent_f64 (F.normalize, 2B x 2B logits, diagonal masked, logsumexp; autograd for the
gradients) on the inputs after rounding to the tested dtype.  Bounds: oracle.ntxent.lse_bound / loss_bound / grad_bound,
derived term by term there; every row's lse and every gradient element is held to them.  Inputs (make_inputs there):
"exact" (norms 1, cosines multiples of 0.25, held to the fp32 bound in every dtype), "norms" (row scales 2^-6 .. 2^6,
partner scales differ), "exact_norms" (exact rows, z1 != z0, power-of-two row scales: still exact in every dtype, and
the one family on which mistakes of the backward show in bf16 at |T| = 0.07) and the degenerate states collapsed,
z0 == z1 and one zero row.  Cases (oracle.ntxent.FWD_CASES / BWD_CASES) are the smallest shapes that reach each path:
n = 2, one tile, two tiles with a ragged last one, a last tile of 2 and of 8 rows, n % 8 != 0, D below one K stage, odd
stage counts, D on the LDS-DMA path in fp32 only, negative temperature, and the backward's W.U on hcir_gemm_f16 at
M = K = N = 8.

fp16 gradients of an un-scaled loss reach the fp16 subnormal range already at these shapes (at the workload's B = 1024,
T = 0.5, ||x|| ~ 22: c rn ~ 4e-5).  torch's own fp16 autograd does the same and the training step passes GradScaler's
65536; the q term of grad_bound pins the subnormal spacing instead of hiding it, and grad_out = 65536 is tested.  With
that factor a few elements of the smallest-norm rows exceed fp16's range: an infinity of the reference's sign is the
correct rounding there (oracle.ntxent.err_over_bound).

Worst err/bound per quantity (max over cases and families; fp32 / fp16 / bf16):

                          lse                  loss                 grad
  CPU emulation     0.198 0.557 0.446    0.046 0.063 0.046    0.250 0.599 0.415
  MI355X kernels    0.153 0.557 0.446    0.061 0.063 0.058    0.250 0.599 0.415

Sharpness (tests/test_ntxent_host.py): factor by which a mistake applied to the float64 reference exceeds the bound, at
the row / column / tile where it shows LEAST, best of the three main families.  (a) one row's positive taken from
another off-diagonal column, (b) one row's diagonal not masked, (c) one column tile's partial missing in one row's lse,
(d) rn of a row replaced by its partner's, (e) the -2 missing at one position of W.  inf: the mistake cannot be made at
that shape without destroying the value (single tile, n = 2).  (d), (e) exist only where the case has a backward.

  case (B, D, T)      dtype     (a)      (b)      (c)     (d)    (e)
  (1, 8, 0.5)         fp32       inf 1.95e+05      inf       -      -
  (1, 8, 0.5)         fp16       inf 1.95e+05      inf       -      -
  (1, 8, 0.5)         bf16       inf 1.95e+05      inf       -      -
  (4, 8, 0.5)         fp32  1.65e+04 5.95e+04      inf     240    464
  (4, 8, 0.5)         fp16     1e+04 4.98e+04      inf     174    365
  (4, 8, 0.5)         bf16     1e+04 4.98e+04      inf    42.2   84.7
  (37, 32, 0.5)       fp32   1.5e+03 7.52e+03      inf       -      -
  (37, 32, 0.5)       fp16   1.5e+03 7.21e+03      inf       -      -
  (37, 32, 0.5)       bf16   1.5e+03 7.21e+03      inf       -      -
  (64, 64, 0.2)       fp32  1.32e+03 2.68e+04      inf     274    507
  (64, 64, 0.2)       fp16       771 1.81e+04      inf     214    412
  (64, 64, 0.2)       bf16       771 1.81e+04      inf    50.1   98.7
  (100, 72, 0.5)      fp32       382 2.61e+03 3.31e+04     258    539
  (100, 72, 0.5)      fp16       230  2.4e+03 2.99e+04     199    400
  (100, 72, 0.5)      bf16       230  2.4e+03 2.99e+04    48.4   98.9
  (101, 40, 0.1)      fp32       675 4.21e+04 2.65e+03       -      -
  (101, 40, 0.1)      fp16       530 4.21e+04 2.65e+03       -      -
  (101, 40, 0.1)      bf16       530 4.21e+04 2.65e+03       -      -
  (128, 96, 0.07)     fp32       823 5.57e+04 1.36e+03     307 9.2e+03
  (128, 96, 0.07)     fp16       428 5.57e+04 1.36e+03     236    446
  (128, 96, 0.07)     bf16       428 5.57e+04 1.36e+03    53.6    101
  (129, 136, 0.5)     fp32       384 2.05e+03      397       -      -
  (129, 136, 0.5)     fp16       171  1.8e+03      233       -      -
  (129, 136, 0.5)     bf16       171  1.8e+03      233       -      -
  (132, 8, 0.2)       fp32       324 5.52e+03      252     215    316
  (132, 8, 0.2)       fp16       324 5.52e+03      252     178    203
  (132, 8, 0.2)       bf16       324 5.52e+03      252    38.7   40.4
  (100, 72, -0.5)     fp32       238     50.3 3.39e+04     276    535
  (100, 72, -0.5)     fp16       136     42.9 3.16e+04     211    397
"""
import math

import pytest
import torch

from oracle import ntxent as ont

pytestmark = pytest.mark.gpu

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
_FWD = [(c, dt) for c in ont.FWD_CASES for dt in ont.case_dtypes(c)]
_BWD = [(c, dt) for c in ont.BWD_CASES for dt in ont.case_dtypes(c)]


def _ids(pairs):
    return [f"{c[0]}-{c[1]}-{c[2]}-{_NAME[dt]}" for c, dt in pairs]


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _forward(pr, t):
    from hcir.losses import ntxent_forward
    z0, z1 = pr.z0.cuda(), pr.z1.cuda()
    loss, lse = ntxent_forward(z0, z1, t, want_lse=True)
    return z0, z1, loss, lse


def _forward_ratios(pr, t, loss, lse):
    return (ont.err_over_bound(lse.cpu(), pr.ref.lse, ont.lse_bound(pr.ref.lse, t, pr.u_in)),
            ont.err_over_bound(loss.cpu(), pr.ref.loss, ont.loss_bound(pr.ref.loss, t, pr.u_in)))


@pytest.mark.parametrize("case,dtype", _FWD, ids=_ids(_FWD))
def test_forward_rows_vs_f64(case, dtype):
    """Every row's lse and the loss, on every family.  A row that takes a wrong positive moves the loss of the exact
    family by >= 0.25 / (|T| 2B), more than 100x its bound (docstring, column (a))."""
    b, d, t = case
    worst_lse = worst_loss = 0.0
    for fam in ont.MAIN_FAMILIES + ont.DEGENERATE_FAMILIES:
        pr = ont.problem(fam, case, dtype)
        _, _, loss, lse = _forward(pr, t)
        assert math.isfinite(loss.item()) and bool(torch.isfinite(lse).all()), fam
        r_lse, r_loss = _forward_ratios(pr, t, loss, lse)
        print(f"\nntxent fwd {case} {_NAME[dtype]} {fam}: lse {r_lse:.3f} loss {r_loss:.3f}")
        worst_lse, worst_loss = max(worst_lse, r_lse), max(worst_loss, r_loss)
        if fam == "collapsed" and b > 1:
            want = torch.tensor(math.log(2 * b - 1), dtype=torch.float64)
            assert abs(loss.item() - want.item()) <= float(ont.loss_bound(want, t, pr.u_in)), fam
        if b == 1:   # the only column of a row is its positive
            assert abs(loss.item()) <= float(ont.loss_bound(torch.zeros((), dtype=torch.float64), t, pr.u_in)), fam
    print(f"\nntxent fwd {case} {_NAME[dtype]} WORST: lse {worst_lse:.3f} loss {worst_loss:.3f}")
    assert worst_lse <= 1.0 and worst_loss <= 1.0


@pytest.mark.parametrize("case,dtype", _BWD, ids=_ids(_BWD))
def test_backward_elements_vs_f64(case, dtype):
    """Every element of dz0 and dz1 at grad_out = 1 and 65536 (GradScaler's initial scale, what the step passes)."""
    from hcir.losses import ntxent_backward
    b, d, t = case
    worst = 0.0
    for fam in ont.MAIN_FAMILIES + ("collapsed", "same"):
        pr = ont.problem(fam, case, dtype)
        z0, z1, _, lse = _forward(pr, t)
        got = {}
        for go in (1.0, 65536.0):
            g0, g1 = ntxent_backward(z0, z1, t, lse, go)
            got[go] = torch.cat([g0, g1], 0).cpu()
            bound = ont.grad_bound(pr.ref, pr.x, pr.dz * go, t, go, dtype, pr.u_in)
            r = ont.err_over_bound(got[go], pr.dz * go, bound, dtype)
            print(f"\nntxent bwd {case} {_NAME[dtype]} {fam} grad_out {go:g}: grad {r:.3f}")
            worst = max(worst, r)
        if dtype == torch.float32:
            # coef = grad_out * inv_t / n: a power-of-two grad_out scales every product exactly (no fp32 underflow
            # at |dz(1)| >= 2^-100, no overflow at these shapes)
            big = got[1.0].abs() >= 2.0 ** -100
            assert torch.equal(got[65536.0][big], got[1.0][big] * 65536.0), fam
    print(f"\nntxent bwd {case} {_NAME[dtype]} WORST: grad {worst:.3f}")
    assert worst <= 1.0


def test_autograd_path_noncontiguous_fp16():
    """NTXentLoss(...)(x0, x1) then (loss * 3).backward(): column-sliced views in, one host read of the upstream grad"""
    from hcir.losses import NTXentLoss
    case, dtype = (100, 72, 0.5), torch.float16
    b, d, t = case
    pr = ont.problem("norms", case, dtype)
    base0 = torch.zeros(b, d + 8, dtype=dtype)
    base1 = torch.zeros(b, d + 8, dtype=dtype)
    base0[:, 4:4 + d], base1[:, 4:4 + d] = pr.z0, pr.z1
    base0 = base0.cuda().requires_grad_(True)
    base1 = base1.cuda().requires_grad_(True)
    x0, x1 = base0[:, 4:4 + d], base1[:, 4:4 + d]
    assert not x0.is_contiguous()
    loss = NTXentLoss(t)(x0, x1)
    (loss * 3).backward()
    r_loss = ont.err_over_bound(loss.detach().cpu(), pr.ref.loss, ont.loss_bound(pr.ref.loss, t, pr.u_in))
    got = torch.cat([base0.grad, base1.grad], 0).cpu()
    bound = ont.grad_bound(pr.ref, pr.x, pr.dz * 3.0, t, 3.0, dtype, pr.u_in)
    r = ont.err_over_bound(got[:, 4:4 + d], pr.dz * 3.0, bound, dtype)
    print(f"\nntxent autograd {case} fp16: loss {r_loss:.3f} grad {r:.3f}")
    assert r_loss <= 1.0 and r <= 1.0
    assert float(got[:, :4].abs().max()) == 0.0 and float(got[:, 4 + d:].abs().max()) == 0.0


# ------------------------------------------------------------------ buffer discipline, determinism, statuses (C ABI)
_PAD = 256
_CANARY = -1536.0     # exact in fp32, fp16 and bf16
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

    def __init__(self, pr, case, dtype):
        from hcir import _lib
        from hcir.ops import _DT
        self.L, self.dt = _lib.lib(), _DT[dtype]
        self.b, self.d, self.t = case
        self.n = 2 * self.b
        self.z0, self.z1 = pr.z0.cuda(), pr.z1.cuda()
        self.st = torch.cuda.current_stream().cuda_stream
        self.fwd_bytes = self.L.hcir_ntxent_workspace_bytes(self.b, self.d, self.dt)
        self.bwd_bytes = self.L.hcir_ntxent_bwd_workspace_bytes(self.b, self.d, self.dt)
        self.loss_full, self.loss = _guarded(1, torch.float32, _CANARY)
        self.lse_full, self.lse = _guarded(self.n, torch.float32, _CANARY)
        self.dz0_full, self.dz0 = _guarded(self.b * self.d, dtype, _CANARY)
        self.dz1_full, self.dz1 = _guarded(self.b * self.d, dtype, _CANARY)

    def outputs_untouched(self):
        torch.cuda.synchronize()
        return all(bool((f == _CANARY).all()) for f in (self.loss_full, self.lse_full, self.dz0_full, self.dz1_full))

    def fwd(self, ws, ws_bytes, b=None, d=None, dt=None, inv_t=None, loss="own"):
        return self.L.hcir_ntxent_fwd(self.z0.data_ptr(), self.z1.data_ptr(), self.b if b is None else b,
                                      self.d if d is None else d, self.dt if dt is None else dt,
                                      1.0 / self.t if inv_t is None else inv_t,
                                      self.loss.data_ptr() if loss == "own" else loss, self.lse.data_ptr(),
                                      ws.data_ptr(), ws_bytes, self.st)

    def bwd(self, lse, ws, ws_bytes, b=None, d=None, dt=None, inv_t=None, dz0="own"):
        return self.L.hcir_ntxent_bwd(self.z0.data_ptr(), self.z1.data_ptr(), self.b if b is None else b,
                                      self.d if d is None else d, self.dt if dt is None else dt,
                                      1.0 / self.t if inv_t is None else inv_t, lse.data_ptr(), 1.0,
                                      self.dz0.data_ptr() if dz0 == "own" else dz0, self.dz1.data_ptr(),
                                      ws.data_ptr(), ws_bytes, self.st)


_BUF = [(c, dt) for c in ((100, 72, 0.5), (132, 8, 0.2)) for dt in (torch.float16, torch.float32)]


@pytest.mark.parametrize("case,dtype", _BUF, ids=_ids(_BUF))
def test_canaries_exact_workspace_and_stale_workspace(case, dtype):
    """Outputs and workspace are slices with canaries on both sides, the workspace exactly as long as
    hcir_ntxent_*workspace_bytes says; every output element is written; a zero-filled and a 0xFF-filled (NaN patterns)
    workspace give bit-equal loss, lse, dz0 and dz1 - the production workspace is shared with every other op and always
    stale - which is also the determinism the kernel file's header claims."""
    pr = ont.problem("norms", case, dtype)
    runs = []
    for fill in (0x00, 0xFF):
        c = _Call(pr, case, dtype)
        ws_full, ws = _guarded(c.fwd_bytes, torch.uint8, _WS_CANARY)
        ws.fill_(fill)
        assert c.fwd(ws, c.fwd_bytes) == 0
        torch.cuda.synchronize()
        assert _pads_intact(ws_full, c.fwd_bytes, _WS_CANARY)
        assert _pads_intact(c.loss_full, 1, _CANARY) and _pads_intact(c.lse_full, c.n, _CANARY)
        assert bool((c.lse != _CANARY).all()) and bool((c.loss != _CANARY).all())
        assert bool(torch.isfinite(c.lse).all()) and bool(torch.isfinite(c.loss).all())
        ws_full, ws = _guarded(c.bwd_bytes, torch.uint8, _WS_CANARY)
        ws.fill_(fill)
        lse = c.lse.clone()
        assert c.bwd(lse, ws, c.bwd_bytes) == 0
        torch.cuda.synchronize()
        assert _pads_intact(ws_full, c.bwd_bytes, _WS_CANARY)
        assert _pads_intact(c.dz0_full, c.b * c.d, _CANARY) and _pads_intact(c.dz1_full, c.b * c.d, _CANARY)
        assert bool((c.dz0 != _CANARY).all()) and bool((c.dz1 != _CANARY).all())
        assert bool(torch.isfinite(c.dz0).all()) and bool(torch.isfinite(c.dz1).all())
        assert _pads_intact(c.lse_full, c.n, _CANARY) and _pads_intact(c.loss_full, 1, _CANARY)
        runs.append([_bits(x) for x in (c.loss, c.lse, c.dz0, c.dz1)])
        r_lse, r_loss = _forward_ratios(pr, c.t, c.loss[0], c.lse)
        bound = ont.grad_bound(pr.ref, pr.x, pr.dz, c.t, 1.0, dtype, pr.u_in)
        r = ont.err_over_bound(torch.cat([c.dz0, c.dz1]).view(c.n, c.d).cpu(), pr.dz, bound, dtype)
        print(f"\nntxent abi {case} {_NAME[dtype]} ws fill {fill:#04x}: lse {r_lse:.3f} loss {r_loss:.3f} grad {r:.3f}")
        assert r_lse <= 1.0 and r_loss <= 1.0 and r <= 1.0
    for name, x, y in zip(("loss", "lse", "dz0", "dz1"), *runs):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_error_statuses_write_nothing(dtype):
    """Every refused call returns its documented status (include/hcir.h) and leaves loss, row_lse, dz0, dz1 untouched"""
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    case = (100, 72, 0.5)
    c = _Call(ont.problem("norms", case, dtype), case, dtype)
    ws = torch.zeros(c.bwd_bytes, dtype=torch.uint8, device="cuda")
    lse = torch.zeros(c.n, device="cuda")
    assert c.bwd_bytes >= c.fwd_bytes
    assert c.L.hcir_status_string(WORKSPACE) and c.L.hcir_status_string(INVALID)
    refused = [
        ("fwd workspace one byte short", c.fwd(ws, c.fwd_bytes - 1), WORKSPACE),
        ("bwd workspace one byte short", c.bwd(lse, ws, c.bwd_bytes - 1), WORKSPACE),
        ("fwd d = 12", c.fwd(ws, c.bwd_bytes, d=12), INVALID),
        ("bwd d = 12", c.bwd(lse, ws, c.bwd_bytes, d=12), INVALID),
        ("bwd b = 6", c.bwd(lse, ws, c.bwd_bytes, b=6), INVALID),
        ("fwd null loss", c.fwd(ws, c.bwd_bytes, loss=None), INVALID),
        ("bwd null dz0", c.bwd(lse, ws, c.bwd_bytes, dz0=None), INVALID),
        ("fwd inv_t = 0", c.fwd(ws, c.bwd_bytes, inv_t=0.0), INVALID),
        ("bwd inv_t = 0", c.bwd(lse, ws, c.bwd_bytes, inv_t=0.0), INVALID),
        ("fwd inv_t = NaN", c.fwd(ws, c.bwd_bytes, inv_t=float("nan")), INVALID),
        ("bwd inv_t = NaN", c.bwd(lse, ws, c.bwd_bytes, inv_t=float("nan")), INVALID),
        ("fwd dtype 7", c.fwd(ws, c.bwd_bytes, dt=7), UNSUPPORTED),
        ("bwd dtype 7", c.bwd(lse, ws, c.bwd_bytes, dt=7), UNSUPPORTED),
    ]
    for what, status, want in refused:
        assert status == want, (what, status)
    assert c.outputs_untouched()
    assert float(ws.max()) == 0.0     # nor the workspace
    # the same object still serves a valid call
    assert c.fwd(ws, c.fwd_bytes) == 0 and c.bwd(c.lse.clone(), ws, c.bwd_bytes) == 0
    torch.cuda.synchronize()
    assert bool((c.lse != _CANARY).all()) and bool((c.dz0 != _CANARY).all()) and bool((c.dz1 != _CANARY).all())
