"""hcir_ntxent_bank_fwd / _bwd and hcir_dense_match_f16 against float64, through the C ABI, between canaries.

Reference and bounds: tests/_densecl_ref.py (float64 restatements pinned to torch's own ops by
tests/test_densecl_host.py; bounds that count the kernels' roundings).  Bank loss: every row_lse, row_pos and k_unit
element, the loss and - where K is a multiple of 8, at every N - every dz0 / dz1 element satisfies err / bound <= 1 on the
shapes, dtypes, input families (oracle.ntxent.make_inputs on a unit-row bank, and "scaled_bank": a bank of non-unit
rows, which a kernel that renormalised the bank would miss) and temperatures of _densecl_ref; dz1 = NULL leaves dz0
bit-identical; two runs (one on a zero-filled, one on a 0xFF-filled workspace of exactly the advertised size) are
bit-identical; every refused call returns its documented status and writes nothing.  Dense match: the chosen key's
float64 score lies within the bound of the float64 maximum for every (b, n); where the float64 top-two gap exceeds
twice the bound the index is the float64 arg-max; at most 10 % of a case's rows are left to the weaker condition; on
the exact integer family idx equals the arg-max (lowest index on a tie) and out is bit-equal to y_values[b, idx].

Worst err / bound per quantity (fp32 / fp16 / bf16; raw with the case of each: profiles/densecl_errors.txt):

                      row_lse            row_pos            k_unit             loss               dz0                dz1
  CPU emulation   0.14 0.43 0.64    0.21 0.47 0.69    0.59 0.50 0.50    0.02 0.06 0.11    0.65 0.81 0.54    0.10 0.99 0.88
  MI355X kernels  0.12 0.43 0.64    0.16 0.47 0.69    0.44 0.46 0.42    0.03 0.06 0.11    0.65 0.81 0.54    0.10 0.99 0.88

Dense match on the MI355X: every chosen score is the float64 maximum on every case; 0 rows of 0.7 % (C = 8, ReLU) and
1.0 % (C = 2048, ReLU) left to the weaker condition, 0 % elsewhere.
"""
import pytest
import torch

import _densecl_ref as dr

pytestmark = pytest.mark.gpu

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
_PAD = 256
_CANARY = -1536.0     # exact in fp32, fp16 and bf16
_ICANARY = -77
_WS_CANARY = 0xA5
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _guarded(n, dtype, canary):
    """(whole tensor, the n-element slice between two canary pads)."""
    full = torch.full((n + 2 * _PAD,), canary, dtype=dtype, device="cuda")
    return full, full[_PAD:_PAD + n]


def _pads_intact(full, n, canary):
    return bool((full[:_PAD] == canary).all()) and bool((full[_PAD + n:] == canary).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


class _BankCall:
    """One problem on the device, outputs between canaries, workspaces of exactly the advertised size."""

    def __init__(self, pr, case, t, dtype, ws_fill=0x00):
        from hcir import _lib
        from hcir.ops import _DT
        self.L, self.dt, self.dtype = _lib.lib(), _DT[dtype], dtype
        self.n, self.k, self.d = case
        self.t = t
        self.z0, self.z1, self.bank = pr.z0.cuda(), pr.z1.cuda(), pr.bank.cuda()
        self.st = torch.cuda.current_stream().cuda_stream
        self.fwd_bytes = self.L.hcir_ntxent_bank_workspace_bytes(self.n, self.k, self.d, self.dt, 0)
        self.bwd_bytes = self.L.hcir_ntxent_bank_workspace_bytes(self.n, self.k, self.d, self.dt, 1)
        nd = self.n * self.d
        self.loss_full, self.loss = _guarded(1, torch.float32, _CANARY)
        self.lse_full, self.lse = _guarded(self.n, torch.float32, _CANARY)
        self.pos_full, self.pos = _guarded(self.n, torch.float32, _CANARY)
        self.ku_full, self.ku = _guarded(nd, torch.float32, _CANARY)
        self.d0_full, self.d0 = _guarded(nd, dtype, _CANARY)
        self.d1_full, self.d1 = _guarded(nd, dtype, _CANARY)
        self.ws_fill = ws_fill

    def workspace(self, nbytes):
        full, ws = _guarded(nbytes, torch.uint8, _WS_CANARY)
        ws.fill_(self.ws_fill)
        return full, ws

    def outputs_untouched(self):
        torch.cuda.synchronize()
        return all(bool((f == _CANARY).all()) for f in (self.loss_full, self.lse_full, self.pos_full, self.ku_full,
                                                        self.d0_full, self.d1_full))

    def fwd(self, ws, ws_bytes, n=None, k=None, d=None, dt=None, inv_t=None, z0="own", bank="own", loss="own"):
        return self.L.hcir_ntxent_bank_fwd(
            self.z0.data_ptr() if z0 == "own" else z0, self.z1.data_ptr(),
            self.bank.data_ptr() if bank == "own" else bank, self.n if n is None else n, self.k if k is None else k,
            self.d if d is None else d, self.dt if dt is None else dt, 1.0 / self.t if inv_t is None else inv_t,
            self.loss.data_ptr() if loss == "own" else loss, self.lse.data_ptr(), self.pos.data_ptr(),
            self.ku.data_ptr(), ws.data_ptr(), ws_bytes, self.st)

    def bwd(self, lse, pos, ws, ws_bytes, n=None, k=None, d=None, dt=None, inv_t=None, dz0="own", dz1="own",
            pos_ptr="own"):
        return self.L.hcir_ntxent_bank_bwd(
            self.z0.data_ptr(), self.z1.data_ptr(), self.bank.data_ptr(), self.n if n is None else n,
            self.k if k is None else k, self.d if d is None else d, self.dt if dt is None else dt,
            1.0 / self.t if inv_t is None else inv_t, lse.data_ptr(), pos.data_ptr() if pos_ptr == "own" else pos_ptr,
            1.0, self.d0.data_ptr() if dz0 == "own" else dz0, self.d1.data_ptr() if dz1 == "own" else dz1,
            ws.data_ptr(), ws_bytes, self.st)

    def run(self, backward, want_dz1=True):
        """Forward (and backward) once; asserts the buffer discipline; returns the outputs' bit patterns."""
        ws_full, ws = self.workspace(self.fwd_bytes)
        assert self.fwd(ws, self.fwd_bytes) == 0
        torch.cuda.synchronize()
        assert _pads_intact(ws_full, self.fwd_bytes, _WS_CANARY)
        for full, view in ((self.loss_full, self.loss), (self.lse_full, self.lse), (self.pos_full, self.pos),
                           (self.ku_full, self.ku)):
            assert _pads_intact(full, view.numel(), _CANARY)
            assert bool((view != _CANARY).all()) and bool(torch.isfinite(view).all())
        out = [_bits(x) for x in (self.loss, self.lse, self.pos, self.ku)]
        if backward:
            ws_full, ws = self.workspace(self.bwd_bytes)
            lse, pos = self.lse.clone(), self.pos.clone()
            assert self.bwd(lse, pos, ws, self.bwd_bytes, dz1="own" if want_dz1 else None) == 0
            torch.cuda.synchronize()
            assert _pads_intact(ws_full, self.bwd_bytes, _WS_CANARY)
            assert _pads_intact(self.d0_full, self.d0.numel(), _CANARY)
            assert bool((self.d0 != _CANARY).all())
            if want_dz1:
                assert _pads_intact(self.d1_full, self.d1.numel(), _CANARY) and bool((self.d1 != _CANARY).all())
            else:
                assert bool((self.d1_full == _CANARY).all())
            assert torch.equal(lse, self.lse) and torch.equal(pos, self.pos)
            out += [_bits(self.d0)] + ([_bits(self.d1)] if want_dz1 else [])
        return out


_BANK = [(c, t, dt) for c in dr.CASES for t in dr.TEMPERATURES for dt in dr.DTYPES]


@pytest.mark.parametrize("case,t,dtype", _BANK,
                         ids=["-".join(str(x) for x in c) + f"-T{t}-{_NAME[dt]}" for c, t, dt in _BANK])
def test_bank_loss_vs_f64(case, t, dtype):
    """Every row_lse, row_pos, k_unit element, the loss and every gradient element on every input family; two runs on
    differently filled workspaces are bit-identical; dz1 = NULL leaves dz0 bit-identical."""
    n, k, d = case
    for family in dr.MAIN_FAMILIES + dr.DEGENERATE_FAMILIES:
        pr = dr.problem(family, case, t, dtype)
        ref = pr.ref
        backward = pr.dz0 is not None
        c = _BankCall(pr, case, t, dtype, 0x00)
        first = c.run(backward)
        r = {"lse": dr.err_over_bound(c.lse.cpu(), ref.lse, dr.lse_bound(ref, t, dtype, pr.u_in)),
             "pos": dr.err_over_bound(c.pos.cpu(), ref.pos, dr.pos_bound(ref, t, pr.u_in)),
             "k_unit": dr.err_over_bound(c.ku.view(n, d).cpu(), ref.k, dr.k_unit_bound(ref)),
             "loss": dr.err_over_bound(c.loss[0].cpu(), ref.loss, dr.loss_bound(ref, t, dtype, pr.u_in))}
        if backward:
            b0, b1 = dr.grad_bounds(ref, pr.z0, pr.z1, pr.dz0, pr.dz1, t, 1.0, dtype, pr.u_in)
            r["dz0"] = dr.err_over_bound(c.d0.view(n, d).cpu(), pr.dz0, b0, dtype)
            r["dz1"] = dr.err_over_bound(c.d1.view(n, d).cpu(), pr.dz1, b1, dtype)
        print(f"\nbank {case} T={t} {_NAME[dtype]} {family}: " + " ".join(f"{q} {v:.3f}" for q, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), (family, r)
        c2 = _BankCall(pr, case, t, dtype, 0xFF)
        second = c2.run(backward)
        for name, x, y in zip(("loss", "lse", "pos", "k_unit", "dz0", "dz1"), first, second):
            assert torch.equal(x, y), (family, name)
        if backward:
            c3 = _BankCall(pr, case, t, dtype, 0xFF)
            third = c3.run(True, want_dz1=False)
            assert torch.equal(third[4], first[4]), (family, "dz0 with dz1 = NULL")


def test_bank_optional_outputs_may_be_null():
    """row_lse, row_pos and k_unit are optional: the loss is the same bits without them."""
    case, t, dtype = (74, 128, 72), 0.5, torch.float16
    pr = dr.problem("norms", case, t, dtype)
    c = _BankCall(pr, case, t, dtype)
    _, ws = c.workspace(c.fwd_bytes)
    assert c.fwd(ws, c.fwd_bytes) == 0
    full = c.loss.clone()
    loss = torch.full((1,), _CANARY, device="cuda")
    assert c.L.hcir_ntxent_bank_fwd(c.z0.data_ptr(), c.z1.data_ptr(), c.bank.data_ptr(), c.n, c.k, c.d, c.dt, 1.0 / t,
                                    loss.data_ptr(), None, None, None, ws.data_ptr(), c.fwd_bytes, c.st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(loss), _bits(full))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_bank_error_statuses_write_nothing(dtype):
    """Every refused call returns its documented status (include/hcir.h) and leaves every output untouched."""
    case, t = (136, 520, 136), 0.5
    c = _BankCall(dr.problem("norms", case, t, dtype), case, t, dtype)
    ws = torch.zeros(max(c.bwd_bytes, c.fwd_bytes), dtype=torch.uint8, device="cuda")
    big = ws.numel()
    lse, pos = torch.zeros(c.n, device="cuda"), torch.zeros(c.n, device="cuda")
    refused = [
        ("fwd workspace one byte short", c.fwd(ws, c.fwd_bytes - 1), WORKSPACE),
        ("bwd workspace one byte short", c.bwd(lse, pos, ws, c.bwd_bytes - 1), WORKSPACE),
        ("fwd null workspace", c.L.hcir_ntxent_bank_fwd(c.z0.data_ptr(), c.z1.data_ptr(), c.bank.data_ptr(), c.n, c.k,
                                                        c.d, c.dt, 2.0, c.loss.data_ptr(), None, None, None, None, big,
                                                        c.st), WORKSPACE),
        ("fwd d = 12", c.fwd(ws, big, d=12), INVALID),
        ("bwd d = 12", c.bwd(lse, pos, ws, big, d=12), INVALID),
        ("fwd n = 0", c.fwd(ws, big, n=0), INVALID),
        ("fwd k = 0", c.fwd(ws, big, k=0), INVALID),
        ("fwd d = 0", c.fwd(ws, big, d=0), INVALID),
        ("bwd k = 516", c.bwd(lse, pos, ws, big, k=516), INVALID),
        ("fwd null z0", c.fwd(ws, big, z0=None), INVALID),
        ("fwd null bank", c.fwd(ws, big, bank=None), INVALID),
        ("fwd null loss", c.fwd(ws, big, loss=None), INVALID),
        ("bwd null dz0", c.bwd(lse, pos, ws, big, dz0=None), INVALID),
        ("bwd null row_pos", c.bwd(lse, pos, ws, big, pos_ptr=None), INVALID),
        ("fwd inv_t = 0", c.fwd(ws, big, inv_t=0.0), INVALID),
        ("fwd inv_t = nan", c.fwd(ws, big, inv_t=float("nan")), INVALID),
        ("bwd inv_t = 0", c.bwd(lse, pos, ws, big, inv_t=0.0), INVALID),
        ("fwd dtype 7", c.fwd(ws, big, dt=7), UNSUPPORTED),
        ("bwd dtype 7", c.bwd(lse, pos, ws, big, dt=7), UNSUPPORTED),
    ]
    for name, got, want in refused:
        assert got == want, (name, got, want)
    assert c.outputs_untouched()
    assert c.L.hcir_ntxent_bank_workspace_bytes(0, 8, 8, c.dt, 0) == 0


# ------------------------------------------------------------------------------------------------------ dense match
class _MatchCall:
    def __init__(self, x, y, vals):
        from hcir import _lib
        from hcir.ops import _DT
        self.L = _lib.lib()
        self.b, self.n, self.c = x.shape
        self.m = y.shape[1]
        self.x, self.y = x.cuda().contiguous(), y.cuda().contiguous()
        self.vals = None if vals is None else vals.cuda().contiguous()
        self.dv = 0 if vals is None else vals.shape[2]
        self.vdt = _DT[torch.float16 if vals is None else vals.dtype]
        self.idx_full, self.idx = _guarded(self.b * self.n, torch.int32, _ICANARY)
        self.out_full, self.out = _guarded(self.b * self.n * self.dv, torch.float16 if vals is None else vals.dtype,
                                           _CANARY)
        self.ws_bytes = self.L.hcir_dense_match_workspace_bytes(self.b, self.m)
        self.st = torch.cuda.current_stream().cuda_stream

    def call(self, ws, ws_bytes, n=None, m=None, c=None, dv=None, b=None, vdt=None, x="own", idx="own", out="own"):
        return self.L.hcir_dense_match_f16(
            self.x.data_ptr() if x == "own" else x, self.y.data_ptr(),
            None if self.vals is None else self.vals.data_ptr(), self.vdt if vdt is None else vdt,
            self.b if b is None else b, self.n if n is None else n, self.m if m is None else m,
            self.c if c is None else c, self.dv if dv is None else dv,
            self.idx.data_ptr() if idx == "own" else idx, self.out.data_ptr() if out == "own" else out,
            ws.data_ptr(), ws_bytes, self.st)

    def run(self, fill=0x00):
        ws_full, ws = _guarded(self.ws_bytes, torch.uint8, _WS_CANARY)
        ws.fill_(fill)
        assert self.call(ws, self.ws_bytes) == 0
        torch.cuda.synchronize()
        assert _pads_intact(ws_full, self.ws_bytes, _WS_CANARY)
        assert _pads_intact(self.idx_full, self.idx.numel(), _ICANARY)
        assert _pads_intact(self.out_full, self.out.numel(), _CANARY)
        idx = self.idx.view(self.b, self.n).cpu().long()
        assert int(idx.min()) >= 0 and int(idx.max()) < self.m
        out = None if self.vals is None else self.out.view(self.b, self.n, self.dv).cpu()
        return idx, out


def _gathered(vals, idx):
    return torch.gather(vals, 1, idx.unsqueeze(-1).expand(-1, -1, vals.shape[2]))


_MATCH = [(c, f) for c in dr.MATCH_CASES for f in dr.MATCH_FAMILIES]


@pytest.mark.parametrize("case,family", _MATCH, ids=["-".join(str(x) for x in c) + "-" + f for c, f in _MATCH])
def test_dense_match_vs_f64(case, family):
    """The dense-match rule of the issue on random maps, fp16 and fp32 values; the gather is bit-exact; two runs agree."""
    for vdt in (torch.float16, torch.float32):
        x, y, vals = dr.match_inputs(family, case, vdt)
        c = _MatchCall(x, y, vals)
        idx, out = c.run(0x00)
        ratio, wrong, weak = dr.match_verdict(idx, x, y)
        print(f"\nmatch {case} {family} values {_NAME[vdt]}: (max - chosen) / bound {ratio:.3f}, strict rows wrong "
              f"{wrong}, rows left to the weaker condition {100 * weak:.2f} %")
        assert ratio <= 1.0 and wrong == 0 and weak <= 0.10
        assert torch.equal(_bits(out), _bits(_gathered(vals, idx)))
        idx2, out2 = _MatchCall(x, y, vals).run(0xFF)
        assert torch.equal(idx, idx2) and torch.equal(_bits(out), _bits(out2))
    idx3, none = _MatchCall(x, y, None).run()
    assert none is None and torch.equal(idx3, idx)


@pytest.mark.parametrize("case", dr.MATCH_CASES[:6], ids=["-".join(str(x) for x in c) for c in dr.MATCH_CASES[:6]])
def test_dense_match_exact_family_is_argmax(case):
    """Every product and score exact: idx is torch's arg-max, the lowest index on the planted duplicate keys and on
    the many integer ties, index 0 for the zero query row; out is bit-equal to y_values[b, idx]."""
    x, y, vals = dr.match_exact_inputs(case)
    ref_idx, _ = dr.select_most_similar_f64(x, y, vals.double())
    xf, yf = x.float(), y.float()
    torch_idx = torch.bmm(xf, torch.nn.functional.normalize(yf, dim=2).transpose(1, 2)).argmax(dim=2)
    assert torch.equal(torch_idx, ref_idx)
    idx, out = _MatchCall(x, y, vals).run()
    assert torch.equal(idx, torch_idx)
    assert bool((idx[:, 0] == 0).all())
    assert torch.equal(_bits(out), _bits(_gathered(vals, idx)))


def test_dense_match_error_statuses_write_nothing():
    x, y, vals = dr.match_inputs("relu", (3, 49, 49, 72, 16))
    c = _MatchCall(x, y, vals)
    ws = torch.zeros(c.ws_bytes, dtype=torch.uint8, device="cuda")
    refused = [
        ("workspace one byte short", c.call(ws, c.ws_bytes - 1), WORKSPACE),
        ("n = 257", c.call(ws, c.ws_bytes, n=257), UNSUPPORTED),
        ("m = 257", c.call(torch.zeros(4 * 3 * 257, dtype=torch.uint8, device="cuda"), 4 * 3 * 257, m=257), UNSUPPORTED),
        ("c = 20", c.call(ws, c.ws_bytes, c=20), UNSUPPORTED),
        ("dv = 12", c.call(ws, c.ws_bytes, dv=12), UNSUPPORTED),
        ("values dtype bf16", c.call(ws, c.ws_bytes, vdt=2), UNSUPPORTED),
        ("n = 0", c.call(ws, c.ws_bytes, n=0), INVALID),
        ("b = 0", c.call(ws, c.ws_bytes, b=0), INVALID),
        ("null x", c.call(ws, c.ws_bytes, x=None), INVALID),
        ("null idx", c.call(ws, c.ws_bytes, idx=None), INVALID),
        ("null out with values", c.call(ws, c.ws_bytes, out=None), INVALID),
    ]
    for name, got, want in refused:
        assert got == want, (name, got, want)
    torch.cuda.synchronize()
    assert bool((c.idx_full == _ICANARY).all()) and bool((c.out_full == _CANARY).all())
