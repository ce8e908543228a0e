"""CPU tests of hcir.optim: the float64 restatement of the optimizer tail against torch, the numpy fp32 emulation of
csrc/optim.hip inside the per-element bound of tests/_optim_ref.py, every listed mistake at least 10-fold outside it,
get_optimizer's groups against the reference's name rule, state-dict round trips with torch, and the argument checks.
Nothing here touches a device."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_ref as R  # noqa: E402

SIZES = (1, 3, 4, 5, 0, 1023, 16384 + 5)


def _families():
    fam = R.families(SIZES, none_at=2, misaligned_at=5)
    ts, cfg = R.families(SIZES, none_at=2, misaligned_at=5)["unit_clip_active"]
    fam["non_finite"] = (R.with_non_finite(ts), cfg)
    ts, cfg = R.families(SIZES, none_at=2)["unit_clip_active"]
    fam["plain_step"] = (ts, R.Cfg(scale=None, max_norm=None, use_norm=False))
    ts, cfg = R.families(SIZES, none_at=2)["small_norm_clip_inactive"]
    fam["growth_due"] = (ts, R.Cfg(tracker=1, growth_interval=2))
    return fam


FAMILIES = _families()


def _ratios(ts, cfg, mistake=None):
    r64 = R.tail64(ts, cfg)
    bnd = R.bounds(ts, r64, cfg)
    emu = R.emulate(ts, cfg, mistake)
    worst = {}
    for k in ("p", "m", "v"):
        worst[k] = max([R.worst_ratio(e[k], o[k], b[k]) for e, o, b in zip(emu["out"], r64["out"], bnd["out"])
                        if o is not None], default=0.0)
    if math.isfinite(r64["norm"]):
        worst["norm"] = abs(emu["norm"] - r64["norm"]) / bnd["norm"]
    else:
        worst["norm"] = 0.0 if not math.isfinite(emu["norm"]) else math.inf
    return worst, r64, emu


def test_float64_restatement_is_torch_adam_with_clip():
    """tail64 against torch.optim.Adam + clip_grad_norm_ in float64 over three steps and two weight-decay groups."""
    ts = R.make_tensors((7, 33, 5, 12), 11, 3.0)
    cfg = R.Cfg(scale=None)
    params = [torch.nn.Parameter(torch.from_numpy(t["p"]).double()) for t in ts]
    opt = torch.optim.Adam([{"params": params[0::2], "weight_decay": 1e-4}, {"params": params[1::2], "weight_decay": 0.0}],
                           lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(3):
        for t, p in zip(ts, params):
            t["g"] = (3.0 * rng.standard_normal(len(t["p"]))).astype(np.float32)
            p.grad = torch.from_numpy(t["g"]).double()
        r = R.tail64(ts, cfg)
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        assert abs(float(norm) - r["norm"]) <= 1e-14 * r["norm"]
        for t, p, o in zip(ts, params, r["out"]):
            st = opt.state[p]
            for got, want in ((p.detach(), o["p"]), (st["exp_avg"], o["m"]), (st["exp_avg_sq"], o["v"])):
                worst = max(worst, float(np.max(np.abs(got.numpy() - want))))
            assert int(st["step"]) == o["step"]
            # continue in float64 from torch's own state: the restatement takes fp32 inputs, so hand it float64 ones
            t["p"], t["m"], t["v"], t["step"] = p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), \
                st["exp_avg_sq"].numpy().copy(), o["step"]
    print(f"tail64 vs torch float64: worst absolute difference {worst:.3e}")
    assert worst <= 1e-15


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_emulation_stays_inside_the_bound(name):
    ts, cfg = FAMILIES[name]
    worst, r64, emu = _ratios(ts, cfg)
    print(name, {k: f"{v:.3f}" for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    assert emu["found_inf"] == r64["found_inf"] == (name == "non_finite")
    assert emu["scale"] == r64["scale"] and emu["tracker"] == r64["tracker"]
    for e, o in zip(emu["out"], r64["out"]):
        assert (e is None) == (o is None) and (e is None or e["step"] == o["step"])
    if name == "non_finite":
        assert emu["scale"] == 32768.0 and emu["tracker"] == 0 and not math.isfinite(emu["norm"])
    if name == "growth_due":
        assert emu["scale"] == 131072.0 and emu["tracker"] == 0
    if name == "small_norm_clip_inactive":
        assert r64["coef"] == 1.0 and emu["coef"] == 1.0
    if name == "unit_clip_active":
        assert r64["coef"] < 0.05


def test_emulation_three_steps_from_zero_state():
    ts, cfg = copy.deepcopy(FAMILIES["unit_clip_active"])
    rng = np.random.default_rng(8)
    for step in range(3):
        worst, r64, emu = _ratios(ts, cfg)
        assert all(v <= 1.0 for v in worst.values()), (step, worst)
        for t, e in zip(ts, emu["out"]):
            if e is not None:
                t["p"], t["m"], t["v"], t["step"] = e["p"], e["m"], e["v"], e["step"]
                t["g"] = (65536.0 * rng.standard_normal(len(t["p"]))).astype(np.float32)
        cfg = R.Cfg(tracker=emu["tracker"])
    assert cfg.tracker == 3 and all(t["step"] == (0 if t["g"] is None else 3) for t in ts)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_mistake_exceeds_the_bound_tenfold(mistake):
    best = (0.0, None)
    for name, (ts, cfg) in sorted(FAMILIES.items()):
        worst, _, _ = _ratios(ts, cfg, mistake)
        w = max(worst["p"], worst["m"], worst["v"])
        if w > best[0]:
            best = (w, name)
    print(f"{mistake}: worst err / bound {best[0]:.3e} on {best[1]}")
    assert best[0] >= 10.0, best


@pytest.mark.parametrize("name", ["resnet18", "vit_b_16"])
def test_get_optimizer_groups_follow_the_reference_rule(name):
    from hcir import optim
    from hcir.main_backbone import SHAM2
    model = SHAM2(name)
    opt = optim.get_optimizer(model, 1e-3, 1e-4, 0.9, 0.999)
    assert isinstance(opt, optim.Adam) and isinstance(opt, torch.optim.Optimizer)
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (no_decay if (n.endswith(".bias") or "bn" in n or "norm" in n) else decay).append(n)
    by_id = {id(p): n for n, p in model.named_parameters()}
    g0, g1 = opt.param_groups
    assert [by_id[id(p)] for p in g0["params"]] == decay and [by_id[id(p)] for p in g1["params"]] == no_decay
    assert g0["weight_decay"] == 1e-4 and g1["weight_decay"] == 0.0
    assert g0["lr"] == g1["lr"] == 1e-3 and g0["betas"] == g1["betas"] == (0.9, 0.999)
    grouped = {id(p) for g in opt.param_groups for p in g["params"]}
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen and all("momentum" in n for n in frozen)
    assert not any(id(p) in grouped for n, p in model.named_parameters() if not p.requires_grad)
    if name == "vit_b_16":
        assert "backbone.encoder.ln.weight" in decay or any(n.endswith("encoder.ln.weight") for n in decay)
        assert any(n.endswith("ln_1.weight") for n in decay)
    else:
        assert any(n.endswith("downsample.1.weight") for n in decay)


def _stepped_torch_adam():
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    opt = torch.optim.Adam([{"params": ps[:1], "weight_decay": 1e-4}, {"params": ps[1:], "weight_decay": 0.0}], lr=2e-3)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
    return ps, opt


def test_adam_state_dict_round_trips_through_torch():
    from hcir import optim
    ps, topt = _stepped_torch_adam()
    ours = optim.Adam([{"params": ps[:1], "weight_decay": 0.5}, {"params": ps[1:]}], lr=1.0)
    ours.load_state_dict(topt.state_dict())
    assert ours.param_groups[0]["weight_decay"] == 1e-4 and ours.param_groups[0]["lr"] == 2e-3
    for p in ps:
        assert set(ours.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(ours.state[p]["step"]) == 2.0
    back = torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:]}])
    back.load_state_dict(ours.state_dict())
    for p in ps:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(back.state[p][k]), torch.as_tensor(topt.state[p][k])), k
    for a, b in zip(back.param_groups, topt.param_groups):
        assert all(a[k] == b[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"))
    # the loaded optimizer is a working torch optimizer
    for p in ps:
        p.grad = torch.ones_like(p)
    back.step()
    assert all(float(back.state[p]["step"]) == 3.0 for p in ps)


def test_grad_scaler_state_dict_uses_torch_keys():
    from hcir import optim
    hand = {"scale": 1024.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 100, "_growth_tracker": 7}
    s = optim.GradScaler()
    assert s.state_dict() == {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                              "_growth_tracker": 0}
    s.load_state_dict(hand)
    assert s.state_dict() == hand and s.get_scale() == 1024.0
    t = torch.amp.GradScaler("cpu")                       # torch's own loader takes what ours wrote
    t.load_state_dict(s.state_dict())
    assert t.state_dict() == hand
    s2 = optim.GradScaler(init_scale=2.0)
    s2.load_state_dict(t.state_dict())
    assert s2.state_dict() == hand
    with pytest.raises(optim.HcirError):
        s2.load_state_dict({})


def test_unsupported_arguments_raise_without_a_device():
    from hcir import optim
    from hcir.optim import HcirError
    p = torch.nn.Parameter(torch.randn(4))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0)):
        with pytest.raises(HcirError):
            optim.Adam([p], **kw)
    for bad in (torch.nn.Parameter(torch.randn(4).double()), torch.nn.Parameter(torch.randn(4).half()),
                torch.nn.Parameter(torch.randn(4, dtype=torch.complex64))):
        with pytest.raises(HcirError):
            optim.Adam([bad])
    opt = optim.Adam([p])                                  # a CPU parameter: there is no CPU path
    p.grad = torch.ones(4)
    with pytest.raises(HcirError):
        opt.step()
    with pytest.raises(HcirError):
        opt.step_scaled(optim.GradScaler())
    with pytest.raises(HcirError):
        opt.step_scaled(torch.amp.GradScaler("cpu"))
    with pytest.raises(HcirError):
        optim.GradScaler().scale(torch.ones(()))
    with pytest.raises(HcirError):
        optim.GradScaler(growth_factor=1.0)
    opt.param_groups[0]["amsgrad"] = True                  # as a loaded state dict could set it
    with pytest.raises(HcirError):
        opt.step()
    assert not opt.state[p] if p in opt.state else True    # nothing was stepped


def test_abi_argument_checks(hcir_built):
    L = hcir_built
    one = 1 << 20                                          # a non-null address that is never dereferenced
    assert L.hcir_grad_sumsq(None, one, 1, None, one, one, None) == -1
    assert L.hcir_grad_sumsq(one, one, 0, None, one, one, None) == -1
    assert L.hcir_grad_sumsq(one, one, 1 << 31, None, one, one, None) == -1
    assert L.hcir_adam_step(one, one, one, None, one, one, one, 1, one, one, one, 0.999, 0.1, 0.001, 1e-8, None) == -1
    assert L.hcir_adam_step(one, one, one, one, one, one, one, 0, one, one, one, 0.999, 0.1, 0.001, 1e-8, None) == -1
    assert L.hcir_adam_step(one, one, one, one, one, one, one, 1 << 31, one, one, one, 0.999, 0.1, 0.001, 1e-8,
                            None) == -1
    import ctypes
    end, lr = (ctypes.c_int32 * 1)(1), (ctypes.c_double * 1)(1e-3)
    args = lambda **k: [k.get("partial", one), one, k.get("n_chunks", 1), None, None, 2.0, 0.5, 2000, 1, 1.0,  # noqa: E731
                        k.get("end", end), lr, k.get("n_groups", 1), 0.9, 0.999, one, k.get("n_part", 1), one, one,
                        one, k.get("ctl", one), None]
    assert L.hcir_optim_finalize(*args(partial=None)) == -1
    assert L.hcir_optim_finalize(*args(n_chunks=-1)) == -1
    assert L.hcir_optim_finalize(*args(n_chunks=1 << 31)) == -1
    assert L.hcir_optim_finalize(*args(n_part=0)) == -1
    assert L.hcir_optim_finalize(*args(ctl=None)) == -1
    assert L.hcir_optim_finalize(*args(n_groups=0)) == -1
    assert L.hcir_optim_finalize(*args(n_groups=17)) == -2
    assert L.hcir_optim_finalize(*args(n_part=2)) == -1    # the groups do not cover the participating parameters
