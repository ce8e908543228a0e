"""CPU-only: the NT-Xent error bounds of oracle.ntxent are honest and sharp.

Honest: a plain-torch emulation of the kernels' arithmetic (oracle.ntxent.emulate) stays inside the bounds for every
case, dtype and input family of tests/test_ntxent_gpu.py.  Sharp: five specific kernel mistakes, applied to the float64
reference, exceed the bound by at least 10x on at least one of the main input families in every case - at the row,
column or tile where the mistake shows least.  The factors are printed (pytest -s) and recorded in the docstring of
tests/test_ntxent_gpu.py.
"""
import math

import pytest
import torch

from oracle import ntxent as ont

_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
_CASE_DT = [(c, dt) for c in ont.FWD_CASES for dt in ont.case_dtypes(c)]
_IDS = [f"{c[0]}-{c[1]}-{c[2]}-{_NAME[dt]}" for c, dt in _CASE_DT]


def emulation_ratios(case, dtype):
    """Worst err/bound of the emulation per quantity over every family of the case."""
    b, d, t = case
    worst = {"lse": 0.0, "loss": 0.0, "grad": 0.0}
    for fam in ont.MAIN_FAMILIES + ont.DEGENERATE_FAMILIES:
        pr = ont.problem(fam, case, dtype)
        bwd = case in ont.BWD_CASES and fam != "zero_row"
        for go in (1.0, 65536.0) if bwd else (1.0,):
            loss, lse, dz0, dz1 = ont.emulate(pr.z0, pr.z1, t, go, backward=bwd)
            worst["lse"] = max(worst["lse"], ont.err_over_bound(lse, pr.ref.lse, ont.lse_bound(pr.ref.lse, t, pr.u_in)))
            worst["loss"] = max(worst["loss"],
                                ont.err_over_bound(loss, pr.ref.loss, ont.loss_bound(pr.ref.loss, t, pr.u_in)))
            if bwd:
                bound = ont.grad_bound(pr.ref, pr.x, pr.dz * go, t, go, dtype, pr.u_in)
                worst["grad"] = max(worst["grad"],
                                    ont.err_over_bound(torch.cat([dz0, dz1], 0), pr.dz * go, bound, dtype))
    return worst


def best_mutation_factors(case, dtype):
    """Per mutation, the largest of the main families' factors (each already the minimum over rows)."""
    bwd = case in ont.BWD_CASES
    per = [ont.mutation_factors(ont.problem(fam, case, dtype), case, dtype, bwd) for fam in ont.MAIN_FAMILIES]
    return {k: max(f[k] for f in per) for k in per[0]}


@pytest.mark.parametrize("case,dtype", _CASE_DT, ids=_IDS)
def test_emulation_within_bounds(case, dtype):
    r = emulation_ratios(case, dtype)
    print(f"\nntxent emulation {case} {_NAME[dtype]}: lse {r['lse']:.3f} loss {r['loss']:.3f} grad {r['grad']:.3f}")
    assert r["lse"] <= 1.0 and r["loss"] <= 1.0 and r["grad"] <= 1.0, r


@pytest.mark.parametrize("case,dtype", _CASE_DT, ids=_IDS)
def test_mutations_exceed_bounds_tenfold(case, dtype):
    f = best_mutation_factors(case, dtype)
    print(f"\nntxent mutations {case} {_NAME[dtype]}: " + " ".join(f"({k}) {v:.3g}" for k, v in f.items()))
    assert all(v >= 10.0 for v in f.values()), f


def test_reference_pieces_are_consistent():
    """NtRef's p, W and u reproduce autograd's gradient in closed form, and the exact family is exact in every dtype."""
    case = (100, 72, 0.5)
    pr = ont.problem("norms", case, torch.float32)
    b, d, t = case
    g = pr.ref.w @ pr.ref.u
    rn = 1.0 / pr.x.norm(dim=1, keepdim=True)
    closed = rn * (g - (g * pr.ref.u).sum(1, keepdim=True) * pr.ref.u) / (t * 2 * b)
    assert (closed - pr.dz).abs().max() <= 1e-12 * pr.dz.abs().max()
    assert torch.allclose(pr.ref.p.sum(1), torch.ones(2 * b, dtype=torch.float64), atol=1e-14)
    loss2, lse2 = ont.ntxent_f64(pr.z0, pr.z1, t)
    assert torch.equal(loss2, pr.ref.loss) and torch.equal(lse2, pr.ref.lse)
    assert torch.equal(pr.ref.pos, pr.ref.sim[torch.arange(2 * b), ont.positives(b)])
    for bb, dd in ((132, 8), (128, 96)):
        z0, z1 = ont.make_inputs("exact", bb, dd)
        for dt in ont.DTYPES:
            assert torch.equal(z0.to(dt).float(), z0)
        assert torch.equal(z0, z1) and len({tuple(r.tolist()) for r in z0}) == bb
        assert torch.equal(z0.norm(dim=1), torch.ones(bb))
        cos4 = (z0.double() @ z0.double().t()) * 4
        assert torch.equal(cos4, cos4.round())
        assert (z0 != 0).sum(1).eq(4).all() and (z0[:, min(dd, 16):] == 0).all()
        z0, z1 = ont.make_inputs("exact_norms", bb, dd)
        z = torch.cat([z0, z1], 0)
        for dt in ont.DTYPES:
            assert torch.equal(z.to(dt).float(), z)
        u = z / z.norm(dim=1, keepdim=True)
        assert len({tuple(r.tolist()) for r in u}) == 2 * bb and (u.abs() * 2).sum(1).eq(4).all()
        ratio = z0.norm(dim=1) / z1.norm(dim=1)
        assert torch.equal(ratio, 2.0 ** torch.log2(ratio).round()) and (ratio != 1).all()
    z0, z1 = ont.make_inputs("norms", 100, 72)
    ratio = z0.norm(dim=1) / z1.norm(dim=1)
    assert (torch.maximum(ratio, 1 / ratio) > 1.25).all()


def test_collapsed_loss_is_log_n_minus_1():
    for case in ((4, 8, 0.5), (132, 8, 0.2)):
        pr = ont.problem("collapsed", case, torch.float32)
        assert abs(float(pr.ref.loss) - math.log(2 * case[0] - 1)) <= 1e-12
        assert float(pr.dz.abs().max()) <= 1e-12
