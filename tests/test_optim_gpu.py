"""hcir.optim on the device against the float64 restatement of tests/_optim_ref.py, element by element: every output
element of p, exp_avg and exp_avg_sq inside its bound, total_norm inside its own, over the input families of
_optim_ref.families and parameter sizes around the chunk boundaries of the table (hcir.optim._CHUNK = 16 384 and the
ABI's 65 536), a zero-element parameter, a parameter at a 4-byte offset (the kernels' 4-byte path) and one without
gradient.  Every buffer sits between canaries.  Worst err / bound per output and family: profiles/optim_errors.txt."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 4, 5, 0, 65535, 65536, 65537, 2 * 65536 + 3, 16383, 16384, 16385, 1001, 7)
MISALIGNED, NO_GRAD = 12, 13
CANARY = 12345.0
_ROWS = {}
N_ROWS = 19                                                # labels passed to _compare by the whole module


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()
    from hcir import optim
    assert optim._CHUNK == R.Cfg().chunk
    yield
    if len(_ROWS) == N_ROWS:                                # a partial run (-k ...) leaves the committed table alone
        with open(os.path.join(ROOT, "profiles", "optim_errors.txt"), "w") as f:
            f.write("# worst |kernel - float64| / bound per output (tests/test_optim_gpu.py; bound: tests/_optim_ref.py)\n")
            f.write(f"{'case':<34}{'p':>10}{'exp_avg':>10}{'exp_avg_sq':>12}{'total_norm':>12}\n")
            for k in sorted(_ROWS):
                w = _ROWS[k]
                f.write(f"{k:<34}{w['p']:>10.4f}{w['m']:>10.4f}{w['v']:>12.4f}{w['norm']:>12.4f}\n")


class Rig:
    """The tensors of one problem on the device, each of p / grad / exp_avg / exp_avg_sq a view into its own buffer
    with 4 canary elements on both sides (5 in front for the misaligned one: a 4-byte offset from 16-byte alignment)."""

    def __init__(self, ts, lr=1e-3):
        from hcir import optim
        self.ts = ts
        self.bufs, self.views = [], []
        params = []
        for i, t in enumerate(ts):
            lead = 5 if i == MISALIGNED else 4
            vw = {}
            for k in ("p", "g", "m", "v"):
                if t[k] is None:
                    continue
                n = len(t[k])
                b = torch.full((lead + n + 4,), CANARY, dtype=torch.float32)
                b[lead:lead + n] = torch.from_numpy(t[k])
                b = b.cuda()
                self.bufs.append((b, lead, n))
                vw[k] = b[lead:lead + n]
                assert n == 0 or vw[k].data_ptr() % 16 == (4 if i == MISALIGNED else 0)
            p = vw["p"].requires_grad_(True)
            if "g" in vw:
                p.grad = vw["g"]
            vw["p"] = p
            params.append(p)
            self.views.append(vw)
        self.params = params
        wds = sorted({t["wd"] for t in ts}, reverse=True)
        groups = [{"params": [p for p, t in zip(params, ts) if t["wd"] == wd], "weight_decay": wd} for wd in wds]
        self.opt = optim.Adam(groups, lr=lr)
        for p, vw, t in zip(params, self.views, ts):
            if "g" in vw:      # state in torch's layout, preloaded so that exp_avg / exp_avg_sq have canaries too
                self.opt.state[p] = {"step": torch.tensor(float(t["step"])), "exp_avg": vw["m"], "exp_avg_sq": vw["v"]}

    def download(self):
        """The current device values as a problem for _optim_ref (fp32 numpy)."""
        ts = []
        for t, vw, p in zip(self.ts, self.views, self.params):
            d = dict(t)
            d["p"] = p.detach().cpu().numpy().copy()
            if "g" in vw:
                st = self.opt.state[p]
                d["g"] = p.grad.cpu().numpy().copy()
                d["m"], d["v"] = st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy()
                d["step"] = int(st["step"])
            ts.append(d)
        return ts

    def check_canaries(self):
        for b, lead, n in self.bufs:
            h = b.cpu()
            assert bool((h[:lead] == CANARY).all()) and bool((h[lead + n:] == CANARY).all())

    def new_grads(self, seed, g_std):
        rng = np.random.default_rng(seed)
        for vw in self.views:
            if "g" in vw:
                vw["g"].copy_(torch.from_numpy((g_std * rng.standard_normal(vw["g"].numel())).astype(np.float32)))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _compare(before, after, r64, bnd, norm, label):
    worst = {}
    for k in ("p", "m", "v"):
        worst[k] = max(R.worst_ratio(a[k], o[k], b[k]) for a, o, b in zip(after, r64["out"], bnd["out"]) if o is not None)
    worst["norm"] = abs(norm - r64["norm"]) / bnd["norm"] if np.isfinite(r64["norm"]) else 0.0
    print(label, {k: f"{v:.4f}" for k, v in worst.items()})
    _ROWS[label] = worst
    assert all(v <= 1.0 for v in worst.values()), (label, worst)
    for a, b, o in zip(after, before, r64["out"]):
        if o is None:                                      # no gradient: nothing moved, the step count did not advance
            assert np.array_equal(a["p"].view(np.int32), b["p"].view(np.int32))
        else:
            assert a["step"] == o["step"]


FAMILY_STD = {"unit_clip_active": 65536.0, "tiny_below_eps": 65536.0 * 1e-12,
              "small_norm_clip_inactive": None, "preloaded_step_999": 65536.0}


@pytest.mark.parametrize("family", sorted(FAMILY_STD))
def test_three_steps_every_element_inside_its_bound(family):
    from hcir import optim
    ts, cfg = R.families(SIZES, none_at=NO_GRAD)[family]
    g_std = FAMILY_STD[family] or 65536.0 * 0.1 / np.sqrt(float(sum(SIZES)))
    rig = Rig(ts)
    scaler = optim.GradScaler()
    versions = [p._version for p in rig.params]
    for step in range(3):
        before = rig.download()
        grad_bits = [_bits(p.grad) for p in rig.params if p.grad is not None]
        if step == 1:                                      # write-only buffers prefilled with NaN
            rig.opt._aux.fill_(float("nan"))
            rig.opt._cache[1]["partial"].fill_(float("nan"))
            rig.opt._cache[1]["flags"].fill_(-1)
        norm = rig.opt.step_scaled(scaler, max_norm=1.0)
        assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32
        after = rig.download()
        c = dataclasses.replace(cfg, tracker=step)
        r64 = R.tail64(before, c)
        _compare(before, after, r64, R.bounds(before, r64, c), float(norm), f"{family} step {step + 1}")
        assert not r64["found_inf"] and scaler.get_scale() == 65536.0 and scaler._get_growth_tracker() == step + 1
        rig.check_canaries()
        for b, p in zip(grad_bits, [p for p in rig.params if p.grad is not None]):
            assert torch.equal(b, _bits(p.grad))           # the gradient buffers are not written
        if step == 1:
            aux = rig.opt._aux.cpu()
            assert torch.isnan(aux[:, -1]).all() and torch.isfinite(aux[:, :-1]).all()   # last = the one without grad
            assert torch.isfinite(rig.opt._cache[1]["partial"]).all()
            assert bool(((rig.opt._cache[1]["flags"] == 0)).all())
        rig.new_grads(100 + step, g_std)
    assert rig.opt.table_rebuilds == 1                     # same pointers, same weight decay: the table was cached
    for i, (p, v0) in enumerate(zip(rig.params, versions)):
        assert (p._version == v0) if i == NO_GRAD else (p._version >= v0 + 3), i
    rig.opt.param_groups[0]["weight_decay"] = 2e-4         # the table carries weight_decay: a change rebuilds it
    rig.opt.step_scaled(scaler)
    assert rig.opt.table_rebuilds == 2


def test_two_runs_give_the_same_bits():
    from hcir import optim
    outs = []
    for _ in range(2):
        ts, _ = R.families(SIZES, none_at=NO_GRAD)["unit_clip_active"]
        rig = Rig(ts)
        scaler = optim.GradScaler()
        norms = []
        for step in range(2):
            norms.append(_bits(rig.opt.step_scaled(scaler)))
            rig.new_grads(7 + step, 65536.0)
        outs.append((norms, [(_bits(p), _bits(rig.opt.state[p]["exp_avg"]), _bits(rig.opt.state[p]["exp_avg_sq"]))
                             for p in rig.params if p.grad is not None]))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0]))
    for ta, tb in zip(outs[0][1], outs[1][1]):
        assert all(torch.equal(a, b) for a, b in zip(ta, tb))


def test_non_finite_gradients_skip_the_step_and_back_off():
    from hcir import optim
    ts, cfg = R.families(SIZES, none_at=NO_GRAD)["preloaded_step_999"]
    rig = Rig(R.with_non_finite(ts))
    scaler = optim.GradScaler()
    scaler._lazy_init("cuda")
    scaler._growth_tracker.fill_(5)
    before = rig.download()
    norm = rig.opt.step_scaled(scaler)
    after = rig.download()
    assert not np.isfinite(float(norm))
    assert scaler.get_scale() == 65536.0 * 0.5 and scaler._get_growth_tracker() == 0
    for a, b in zip(after, before):
        for k in ("p", "m", "v"):
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
        assert a["step"] == b["step"]
        if a["g"] is not None:
            assert np.array_equal(a["g"].view(np.int32), b["g"].view(np.int32))
    rig.check_canaries()
    r64 = R.tail64(before, R.Cfg(tracker=5))
    assert r64["found_inf"] and r64["scale"] == 32768.0 and r64["tracker"] == 0
    # the next clean step is taken, at the backed-off scale
    rig.new_grads(3, 32768.0)
    before = rig.download()
    norm = rig.opt.step_scaled(scaler)
    c = R.Cfg(scale=32768.0)
    r64 = R.tail64(before, c)
    _compare(before, rig.download(), r64, R.bounds(before, r64, c), float(norm), "after_backoff")
    assert scaler._get_growth_tracker() == 1


def test_scale_grows_after_growth_interval_clean_steps():
    from hcir import optim
    ts, _ = R.families(SIZES[:5], none_at=None)["unit_clip_active"]
    rig = Rig(ts)
    scaler = optim.GradScaler(init_scale=1024.0, growth_interval=2)
    rig.opt.step_scaled(scaler)
    assert scaler.get_scale() == 1024.0 and scaler._get_growth_tracker() == 1
    rig.opt.step_scaled(scaler)
    assert scaler.get_scale() == 2048.0 and scaler._get_growth_tracker() == 0
    assert scaler.state_dict() == {"scale": 2048.0, "growth_factor": 2.0, "backoff_factor": 0.5,
                                   "growth_interval": 2, "_growth_tracker": 0}
    x = torch.ones((), device="cuda", requires_grad=True)
    assert float(scaler.scale(x * 3.0).detach()) == 3.0 * 2048.0


@pytest.mark.parametrize("mode", ["plain_step", "clip_without_scaler"])
def test_steps_without_a_scaler(mode):
    ts = R.make_tensors(SIZES, 21, 1.0, none_at=NO_GRAD)
    rig = Rig(ts)
    cfg = R.Cfg(scale=None, max_norm=None, use_norm=False) if mode == "plain_step" else R.Cfg(scale=None)
    for step in range(2):
        before = rig.download()
        if mode == "plain_step":
            assert rig.opt.step() is None
            norm = 0.0
        else:
            norm = float(rig.opt.step_scaled(None, max_norm=1.0))
        r64 = R.tail64(before, cfg)
        _compare(before, rig.download(), r64, R.bounds(before, r64, cfg), norm, f"{mode} step {step + 1}")
        rig.check_canaries()
        rig.new_grads(50 + step, 1.0)


def test_mixed_form_torch_scaler_and_clip_around_our_adam():
    """torch.amp.GradScaler + clip_grad_norm_ around hcir.optim.Adam: unscale and clip are torch's (they write the
    gradients), the Adam arithmetic is ours - held to float64 on the gradients torch's clip left."""
    ts = R.make_tensors(SIZES, 22, 1024.0, none_at=NO_GRAD)
    rig = Rig(ts)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    scaler.scale(torch.ones((), device="cuda"))            # initialises the scaler's device state
    scaler.unscale_(rig.opt)
    torch.nn.utils.clip_grad_norm_([p for p in rig.params if p.numel()], 1.0)
    before = rig.download()
    scaler.step(rig.opt)
    scaler.update()
    cfg = R.Cfg(scale=None, max_norm=None, use_norm=False)
    r64 = R.tail64(before, cfg)
    _compare(before, rig.download(), r64, R.bounds(before, r64, cfg), 0.0, "mixed_form")
    assert scaler.get_scale() == 1024.0
    rig.check_canaries()


def test_state_loaded_from_torch_adam_then_one_fused_step():
    from hcir import optim
    ts = R.make_tensors((5, 16385, 1001), 23, 1.0)
    ps = [torch.nn.Parameter(torch.from_numpy(t["p"]).cuda()) for t in ts]
    groups = lambda: [{"params": ps[0::2], "weight_decay": 1e-4}, {"params": ps[1::2], "weight_decay": 0.0}]  # noqa: E731
    topt = torch.optim.Adam(groups(), lr=1e-3)
    g = torch.Generator().manual_seed(1)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).cuda()
        topt.step()
    ours = optim.Adam(groups(), lr=5.0)
    ours.load_state_dict(topt.state_dict())
    scaler = optim.GradScaler(init_scale=256.0)
    for p in ps:
        p.grad = (256.0 * torch.randn(p.shape, generator=g)).cuda()
    before = [dict(p=p.detach().cpu().numpy().copy(), g=p.grad.cpu().numpy().copy(),
                   m=topt.state[p]["exp_avg"].cpu().numpy().copy(), v=topt.state[p]["exp_avg_sq"].cpu().numpy().copy(),
                   step=int(topt.state[p]["step"]), wd=t["wd"], lr=1e-3) for p, t in zip(ps, ts)]
    assert all(b["step"] == 2 for b in before)
    norm = ours.step_scaled(scaler)
    after = [dict(p=p.detach().cpu().numpy(), m=ours.state[p]["exp_avg"].cpu().numpy(),
                  v=ours.state[p]["exp_avg_sq"].cpu().numpy(), step=int(ours.state[p]["step"])) for p in ps]
    cfg = R.Cfg(scale=256.0)
    r64 = R.tail64(before, cfg)
    _compare(before, after, r64, R.bounds(before, r64, cfg), float(norm), "loaded_from_torch_adam")
    assert all(a["step"] == 3 for a in after)
    # and back: torch's Adam continues from our state dict
    back = torch.optim.Adam(groups(), lr=1e-3)
    back.load_state_dict(ours.state_dict())
    back.step()
    assert all(int(back.state[p]["step"]) == 4 for p in ps)
