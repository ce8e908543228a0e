"""CPU-only: the SupConLoss restatement of tests/_supcon_ref.py is the reference's loss, its bounds are honest and sharp,
and the module refuses what it must before any launch.

Pinned: the float64 restatement equals the vectors the reference class produced (tests/golden/supcon_ref.npz) to 1e-12,
value and gradient; the closed form the kernels implement (W = G + G^T, g = W x, scale, projection) equals autograd.
Honest: a plain-torch emulation of the kernels' arithmetic stays inside every bound for every case, dtype, input family,
label family and both normalize settings of tests/test_supcon_gpu.py.  Sharp: seven specific kernel mistakes, applied
to the float64 reference, exceed the bound at least tenfold on at least one main input family wherever they can be made.
The factors are printed (pytest -s) and recorded in profiles/supcon_errors.txt.
"""
import os

import numpy as np
import pytest
import torch

import _supcon_ref as sc
from oracle import ntxent as ont

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
_CASE_DT = [(c, dt) for c in sc.CASES for dt in sc.case_dtypes(c)]
_IDS = ["-".join(str(x) for x in c) + "-" + _NAME[dt] for c, dt in _CASE_DT]
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supcon_ref.npz")


def test_restatement_equals_reference_goldens():
    z = np.load(_GOLDEN)
    assert int(z["n"]) >= 6
    seen_v, seen_zero_rows, seen_none = set(), False, False
    for i in range(int(z["n"])):
        f = torch.from_numpy(z[f"features_{i}"])
        labels = torch.from_numpy(z[f"labels_{i}"]) if bool(z[f"has_labels_{i}"]) else None
        t, tb = float(z[f"t_{i}"]), float(z[f"t_base_{i}"])
        ref = sc.supcon_f64(f, labels, t, tb, normalize=False, full=True)
        grad = sc.supcon_grad_f64(f, labels, t, tb, normalize=False)
        assert abs(float(ref.loss) - float(z[f"loss_{i}"])) <= 1e-12 * max(1.0, abs(float(z[f"loss_{i}"]))), i
        want = torch.from_numpy(z[f"grad_{i}"])
        assert float((grad - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), i
        seen_v.add(f.shape[1])
        seen_zero_rows |= bool((ref.npos == 0).any())
        seen_none |= labels is None
    assert seen_v == {1, 2, 3} and seen_zero_rows and seen_none


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalize"])
def test_closed_form_reproduces_autograd(normalize):
    """p, W and x of ScRef reproduce autograd's gradient; rows without positives have a zero loss term and, without
    the G^T term of other rows, no gradient of their own."""
    for case, lab in (((68, 2, 72, .2, .1), "three"), ((136, 1, 64, .3, .07), "mixed"), ((48, 3, 96, .07, .07), "wide"),
                      ((100, 2, 72, -.5, .07), "none")):
        pr = sc.problem("norms", lab, case, torch.float32, normalize)
        closed = sc.closed_form_grad(pr.ref, pr.features, case[4], normalize)
        # raw rows of norm up to 2^6 sqrt(D): logits of 1e6 and more, whose float64 spacing (1e-10) is the relative
        # error of exp(s - lse) either way
        tol = 1e-11 if normalize else 1e-8
        assert float((closed - pr.dx).abs().max()) <= tol * float(pr.dx.abs().max()), (case, lab)
        assert pr.ref.row_loss.dtype == torch.float64 and pr.ref.W.dtype == torch.float64
        off = pr.ref.p.sum(1)
        assert torch.allclose(off, torch.ones_like(off), atol=1e-13)
        assert torch.equal(pr.ref.W, pr.ref.W.t()) and float(pr.ref.W.abs().max()) <= 2.0
        assert bool((pr.ref.row_loss[pr.ref.npos == 0] == 0).all())
        same = pr.ref.m
        assert torch.equal((pr.ref.npos[:, None] * same), (pr.ref.npos[None, :] * same))   # m_ij = 1 -> n_i = n_j
    pr = sc.problem("norms", "mixed", (136, 1, 64, .3, .07), torch.float32, normalize)
    assert bool((pr.ref.npos == 0).any()) and bool((pr.ref.npos == 1).any())


def test_special_case_is_ntxent():
    """V = 2, labels None, normalize, T_base = T: lightly's NT-Xent (oracle.ntxent.ntxent_f64), value, lse and gradient"""
    for b, d, t in ((4, 8, 0.5), (37, 32, 0.5), (100, 72, -0.5)):
        z0, z1 = ont.make_inputs("norms", b, d)
        f = torch.stack([z0, z1], 1)
        ref = sc.supcon_f64(f, None, t, t, True, full=True)
        nt = ont.ntxent_f64(z0, z1, t, full=True)
        assert abs(float(ref.loss - nt.loss)) <= 1e-13 * max(1.0, abs(float(nt.loss)))
        assert float((ref.lse - nt.lse).abs().max()) <= 1e-13 * float(nt.lse.abs().max())
        assert float((ref.W - nt.w).abs().max()) <= 1e-14
        g0, g1 = ont.ntxent_grads_f64(z0, z1, t)
        mine = sc.supcon_grad_f64(f, None, t, t, True)
        assert float((mine - torch.stack([g0, g1], 1)).abs().max()) <= 1e-12 * float(g0.abs().max())


def emulation_ratios(case, dtype):
    """Worst err/bound of the emulation per quantity over every family, label family and normalize of the case."""
    b, v, d, t, tb = case
    worst = {"lse": 0.0, "loss": 0.0, "grad": 0.0}
    for normalize in (False, True):
        for lab in sc.LABEL_FAMILIES:
            for fam in sc.MAIN_FAMILIES:
                pr = sc.problem(fam, lab, case, dtype, normalize)
                bwd = sc.has_backward(case)
                for go in (1.0, 65536.0) if bwd else (1.0,):
                    loss, lse, npos, dfeat = sc.emulate(pr.features, pr.labels, t, tb, normalize, go, backward=bwd)
                    assert torch.equal(npos, pr.ref.npos)
                    worst["lse"] = max(worst["lse"], sc.err_over_bound(lse, pr.ref.lse, sc.lse_bound(pr.ref, t, pr.u_in)))
                    worst["loss"] = max(worst["loss"], sc.err_over_bound(loss, pr.ref.loss,
                                                                         sc.loss_bound(pr.ref, t, tb, pr.u_in)))
                    if bwd:
                        bound = sc.grad_bound(pr.ref, pr.features, pr.dx * go, t, tb, normalize, go, dtype, pr.u_in)
                        worst["grad"] = max(worst["grad"],
                                            sc.err_over_bound(sc.rows_of(dfeat), pr.dx * go, bound, dtype))
    return worst


@pytest.mark.parametrize("case,dtype", _CASE_DT, ids=_IDS)
def test_emulation_within_bounds(case, dtype):
    r = emulation_ratios(case, dtype)
    print(f"\nsupcon emulation {case} {_NAME[dtype]}: lse {r['lse']:.3f} loss {r['loss']:.3f} grad {r['grad']:.3f}")
    assert r["lse"] <= 1.0 and r["loss"] <= 1.0 and r["grad"] <= 1.0, r


def best_mutation_factors(case, dtype, lab, normalize):
    """Per mutation, the largest of the main input families' factors."""
    per = [sc.mutation_factors(sc.problem(fam, lab, case, dtype, normalize), case, dtype, normalize)
           for fam in sc.MAIN_FAMILIES]
    return {k: max(f[k] for f in per) for k in per[0]}


@pytest.mark.parametrize("case,dtype", _CASE_DT, ids=_IDS)
def test_mutations_exceed_bounds_tenfold(case, dtype):
    """Every mistake misses its bound at least tenfold on at least one main input family, at every shape and normalize
    setting at which it can be made.  (a), (c), (e), (f), (g): with every label family that allows the mistake.
    (b), (d): with the best label family - in a class of n + 1 rows a count that is off by one moves P / n by P / (n (n + 1))
    only, and a missing tile takes 128 of 2B - 1 near-cancelling logits out of the all-one-class mean; with those
    labels it is the exact row_npos check of tests/test_supcon_gpu.py that catches (b)."""
    b, v, d, t, tb = case
    inf = float("inf")
    for normalize in (False, True):
        best = {}
        for lab in sc.LABEL_FAMILIES:
            f = best_mutation_factors(case, dtype, lab, normalize)
            print(f"\nsupcon mutations {case} {_NAME[dtype]} {lab} normalize={int(normalize)}: "
                  + " ".join(f"({k}) {x:.3g}" for k, x in f.items()))
            assert all(f[k] >= 10.0 for k in f if k not in "bd"), (lab, normalize, f)
            for k, x in f.items():
                best[k] = x if best.get(k, inf) == inf else (max(best[k], x) if x != inf else best[k])
            if lab == "wide" and b >= 3:
                assert f["f"] != inf
            if lab == "mixed" and v == 1 and sc.has_backward(case):
                assert f["e"] != inf
            if lab == "one" and b * v > 128:
                assert f["d"] != inf
        print(f"\nsupcon mutations {case} {_NAME[dtype]} BEST normalize={int(normalize)}: "
              + " ".join(f"({k}) {x:.3g}" for k, x in best.items()))
        assert all(x >= 10.0 for x in best.values()), (normalize, best)


# ------------------------------------------------------------------ the module, without a device
def test_module_value_errors_as_the_reference():
    from hcir.losses import SupConLoss
    crit = SupConLoss()
    assert (crit.temperature, crit.contrast_mode, crit.base_temperature, crit.normalize) == (0.07, "all", 0.07, False)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        crit(torch.zeros(4, 8))
    with pytest.raises(ValueError, match="both `labels` and `mask`"):
        crit(torch.zeros(4, 2, 8), labels=torch.zeros(4, dtype=torch.int64), mask=torch.eye(4))
    with pytest.raises(ValueError, match="does not match"):
        crit(torch.zeros(4, 2, 8), labels=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="Unknown mode"):
        SupConLoss(contrast_mode="some")


def test_module_not_implemented_names_the_reference():
    from hcir.losses import SupConLoss
    with pytest.raises(NotImplementedError, match="never used by the reference"):
        SupConLoss(contrast_mode="one")
    with pytest.raises(NotImplementedError, match="never passed by the reference"):
        SupConLoss()(torch.zeros(4, 2, 8), mask=torch.eye(4))


def test_module_refuses_cpu_tensors_and_float_labels():
    from hcir import HcirError
    from hcir.losses import SupConLoss
    with pytest.raises(HcirError, match="no CPU fallback"):
        SupConLoss()(torch.zeros(4, 2, 8), labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(HcirError, match="no CPU fallback"):
        SupConLoss()(torch.zeros(4, 2, 2, 4))      # flattened to [4, 2, 8] first
    with pytest.raises(HcirError, match="64-bit integers"):
        SupConLoss()(torch.zeros(4, 2, 8), labels=torch.zeros(4))


def test_backward_shape_rule_is_checked_before_launch():
    """N % 8 != 0 with a gradient wanted: HcirError from supcon_backward's own check, no library call"""
    from hcir import HcirError
    from hcir.losses import supcon_backward
    f = torch.zeros(3, 2, 8)
    with pytest.raises(HcirError, match="multiple of 8"):
        supcon_backward(f, None, 0.07, 0.07, False, torch.zeros(6), torch.zeros(6, dtype=torch.int32), 1.0)


def test_abi_null_features_is_invalid(hcir_built):
    from hcir import _lib
    L = _lib.lib()
    assert L.hcir_supcon_fwd(None, None, 4, 2, 8, 0, 1.0, 1.0, 0, None, None, None, None, 0, None) == -1
    assert L.hcir_supcon_bwd(None, None, 4, 2, 8, 0, 1.0, 1.0, 0, None, None, 1.0, None, None, 0, None) == -1
    assert L.hcir_supcon_workspace_bytes(4, 2, 8, 0, 0) > 0 and L.hcir_supcon_workspace_bytes(0, 2, 8, 0, 0) == 0
    assert L.hcir_supcon_workspace_bytes(4, 2, 8, 0, 1) > 0
