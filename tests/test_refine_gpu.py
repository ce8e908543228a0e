"""GPU: hcir_topk_refine_f32 (csrc/refine.hip) through the C ABI against oracle.refine, over the case table of
tests/_refine_cases.py (tests/test_refine_host.py shows that the table sees every mistake of oracle.refine.MISTAKES).

Every case: out_val, out_idx and certified lie between canary rows, prefilled with NaN, a sentinel and 7; the case runs
twice with bit-equal results; values, indices and flags equal refine_ref bit for bit.  The decision rule is pinned at
its threshold: err_bound = e*, the smallest fp32 with fl32(t + e*) >= vk, must not certify, the fp32 just below must,
and t + err == vk exactly must not.  E_i as the kernel forms it from mirror_consts is recovered from the flip point of
`certified` over a grid of cand_val[kc-1] and held between E64 (soundness) and the bound derived in oracle/refine.py.
Candidate indices are never out of range here: the kernel trusts them.

The recovered E_i / E64 per family is printed at the end of the module (profiles/refine_bounds.txt keeps a copy)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_cases as rc  # noqa: E402
from oracle import refine as orf  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1
CANARY = 2
SENTINEL_IDX, SENTINEL_CERT = -555, 7
SPECS = rc.specs()
ROWS = []


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\nrefine-probe: E_i recovered from the kernel, per query family")
    for r in ROWS:
        print(r)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(spec):
        key = rc.spec_id(spec)
        if key not in cache:
            cache[key] = rc.build(spec)
        return cache[key]
    return get


class Out:
    """[CANARY + rows + CANARY, cols]: a pattern everywhere, `init` in the live rows; check() wants the canaries back"""

    def __init__(self, rows, cols, dtype, init):
        total = (rows + 2 * CANARY) * cols
        self.buf = ((torch.arange(total, device="cuda") % 251) - 125).to(dtype).view(rows + 2 * CANARY, cols)
        self.t = self.buf[CANARY:CANARY + rows]
        self.t[...] = init
        self.before = self.buf.clone()

    def check(self):
        rows = self.t.shape[0]
        assert torch.equal(self.buf[:CANARY], self.before[:CANARY]), "rows before the buffer written"
        assert torch.equal(self.buf[CANARY + rows:], self.before[CANARY + rows:]), "rows past the buffer written"
        return self.t.cpu().numpy()

    def untouched(self):
        a, b = self.buf.cpu().numpy(), self.before.cpu().numpy()
        return a.tobytes() == b.tobytes()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(L, case, err=None, consts=None, dev=None):
    """one call -> (status, out_val Out, out_idx Out, certified Out).  dev: the device copies, made once per case"""
    ng, d = case["g"].shape
    nq, kc = case["cand_idx"].shape
    k = case["k"]
    live = case["cand_idx"][case["cand_idx"] >= 0] - case["idx_base"]
    assert live.size == 0 or (0 <= live.min() and live.max() < ng), "a candidate index out of range"
    dev = dev if dev is not None else {n: _dev(case[n]) for n in ("q", "g", "cand_idx", "cand_val", "qn", "gn")}
    err_d = _dev(None if err is None else np.asarray(err, dtype=np.float32))
    host = None if consts is None else (ctypes.c_float * 4)(*[float(c) for c in consts])
    val, idx = Out(nq, k, torch.float32, float("nan")), Out(nq, k, torch.int64, SENTINEL_IDX)
    cert = Out(1, nq, torch.int32, SENTINEL_CERT)
    st = L.hcir_topk_refine_f32(dev["q"].data_ptr(), nq, dev["g"].data_ptr(), ng, d, dev["cand_idx"].data_ptr(),
                                dev["cand_val"].data_ptr(), kc, k, case["idx_base"], _ptr(dev["qn"]), _ptr(dev["gn"]),
                                _ptr(err_d), host, val.t.data_ptr(), idx.t.data_ptr(), cert.t.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, val, idx, cert


def run_twice(L, case, err=None, consts=None):
    dev = {n: _dev(case[n]) for n in ("q", "g", "cand_idx", "cand_val", "qn", "gn")}
    outs = []
    for _ in range(2):
        st, val, idx, cert = launch(L, case, err, consts, dev)
        assert st == 0
        outs.append((val.check(), idx.check(), cert.check()[0]))
    assert orf.same_bits(outs[0], outs[1]), "two runs differ"
    return outs[0]


@pytest.mark.parametrize("spec", SPECS, ids=rc.spec_id)
def test_refine_bit_for_bit(spec, cases, L):
    case = cases(spec)
    got = run_twice(L, case, err=case["err"])
    want = orf.refine_ref(err=case["err"], **rc.ref_args(case))
    assert np.array_equal(got[1], want[1]), "indices"
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), "values"
    assert np.array_equal(got[2], want[2]), "certified"


DECISION_SPECS = ([s for s in SPECS if s["name"] == "shape"][2:9]             # d 40 .. 2048, kc 2 .. 64, nq 3 .. 130
                  + [s for s in SPECS if s["name"] == "combo"][::7])          # no norms at base 0, both norms at base 7


@pytest.mark.parametrize("spec", DECISION_SPECS, ids=rc.spec_id)
def test_decision_rule_at_the_threshold(spec, cases, L):
    """err_bound = e*: no query certified; the fp32 number below e*: every one"""
    case = cases(spec)
    assert case["decided"].any()
    for err, want in rc.decision_runs(case):
        got = run_twice(L, case, err=err)
        on = want >= 0
        assert np.array_equal(got[2][on], want[on]), (got[2][on], want[on])
        assert orf.same_bits(got, orf.refine_ref(err=err, **rc.ref_args(case)))


def test_equality_is_not_certified(cases, L):
    """t + err == vk in real numbers, on every case that holds such queries"""
    seen = 0
    for spec in SPECS:
        if spec["nq"] > 5 or spec["d"] > 768:
            continue
        case = cases(spec)
        eq = case["equal"]
        if eq.any():
            t, e = case["cand_val"][eq, -1].astype(np.float64), case["err"][eq].astype(np.float64)
            vk = orf.refine_ref(err=case["err"], **rc.ref_args(case))[0][eq, case["k"] - 1].astype(np.float64)
            assert (t + e == vk).all()
            assert (run_twice(L, case, err=case["err"])[2][eq] == 0).all()
            seen += int(eq.sum())
    assert seen >= 5


@pytest.mark.parametrize("family", orf.PROBE_FAMILIES)
def test_kernel_error_bound_recovered(family, L):
    """err_bound = NULL: E64 <= E_i <= (1.01 + delta) E64 + 1e-7 + resolution, E_i bracketed by the flip of certified"""
    p = orf.probe_make(*orf.probe_query(family))
    case = dict(q=p["q"], g=p["g"], cand_idx=p["cand_idx"], cand_val=p["cand_val"], k=orf.PROBE_K, idx_base=0, qn=None,
                gn=None)
    val, idx, cert = run_twice(L, case, consts=p["consts"])
    want = orf.refine_ref(err=np.zeros(len(cert), dtype=np.float32), **case)
    assert np.array_equal(idx, want[1]) and np.array_equal(val.view(np.int32), want[0].view(np.int32))
    assert set(cert) <= {0, 1}
    b = orf.probe_bracket(p, cert)
    ROWS.append(f"refine-probe {family:11s} d {p['d']:4d}  E64 {p['e64']:.6e}  E_i in [{b['lo']:.9e}, {b['hi']:.9e})  "
                f"(hi - 1e-7) / E64 {(b['hi'] - 1e-7) / p['e64']:.8f}  1.01 + delta {1.01 + orf.ei_delta(p['d']):.8f}  "
                f"resolution / E64 {b['resolution'] / p['e64']:.2e}")
    assert b["inside"], "certified does not flip on the grid: E_i is far from 1.01 E64 + 1e-7"
    order = np.argsort(p["x"])
    assert (np.diff(cert[order]) >= 0).all(), "certified is not monotone in cand_val[kc-1]"
    assert b["sound"], b
    assert b["tight"], b


def test_values_and_indices_with_the_kernel_bound(cases, L):
    """err_bound = NULL on a case of the table: the same values and indices, flags where the decision is clear"""
    spec = [s for s in SPECS if s["name"] == "combo"][7]
    case = cases(spec)
    e64, c64 = orf.err_bound64(case["q"], case["g"])
    got = run_twice(L, case, consts=orf.consts32(c64))
    want = orf.refine_ref(consts=c64, **rc.ref_args(case))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    t, vk = case["cand_val"][:, -1].astype(np.float64), want[0][:, case["k"] - 1].astype(np.float64)
    clear_no = t + e64 >= vk + 1e-3 * np.abs(vk)
    clear_yes = t + orf.ei_upper(e64, spec["d"]) < vk - 1e-3 * np.abs(vk)
    assert (got[2][clear_no] == 0).all() and (got[2][clear_yes] == 1).all()
    assert (clear_no | clear_yes).any()


def test_argument_checks_write_nothing(cases, L):
    case = cases(SPECS[3])                                          # nq 5, d 72, kc 16, k 5
    dev = {n: _dev(case[n]) for n in ("q", "g", "cand_idx", "cand_val", "qn", "gn")}
    nq, kc = case["cand_idx"].shape
    ng, d = case["g"].shape
    err = _dev(case["err"])
    consts = (ctypes.c_float * 4)(0.0, 1.0, 1.0, 1e-6)
    val, idx = Out(nq, case["k"], torch.float32, float("nan")), Out(nq, case["k"], torch.int64, SENTINEL_IDX)
    cert = Out(1, nq, torch.int32, SENTINEL_CERT)

    def call(nq=nq, d=d, kc=kc, k=case["k"], err=err.data_ptr(), mc=None):
        st = L.hcir_topk_refine_f32(dev["q"].data_ptr(), nq, dev["g"].data_ptr(), ng, d, dev["cand_idx"].data_ptr(),
                                    dev["cand_val"].data_ptr(), kc, k, 0, None, None, err, mc, val.t.data_ptr(),
                                    idx.t.data_ptr(), cert.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert val.untouched() and idx.untouched() and cert.untouched()
        return st

    assert call(d=68) == INVALID                                    # d % 8 != 0
    assert call(kc=65) == INVALID
    assert call(kc=4, k=5) == INVALID                               # k > kc
    assert call(err=None, mc=None) == INVALID
    assert call(nq=0) == INVALID and call(nq=-1) == INVALID
    assert call(err=None, mc=consts, k=0) == INVALID
