"""SHAMTrainStep with the fused optimizer tail (hcir.optim.get_optimizer + hcir.optim.GradScaler): one step of the
smallest configurations the train tests use - ResNet-18 with every HIP switch on at B = 8, 32 x 32
(tests/_resnet_train_frame.py) and ViT-B/16 at B = 8 (tests/test_vit_train_gpu.py).  The parameters after the step are
held element by element to the float64 tail of tests/_optim_ref.py applied to the untouched scaled gradients the step
leaves in .grad; a twin model with torch's optimizer, scaler and clip returns the same loss dict and ends with the same
scale and tracker; none of torch's tail functions is entered; step_scaled runs under torch's sync debug mode, with
the chunk table rebuilt and with it cached."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LR, WD, INIT_SCALE = 1e-3, 1e-4, 256.0


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _model(name):
    from hcir.main_backbone import SHAM2
    torch.manual_seed(9)
    m = SHAM2(name).cuda()
    if name == "resnet18":
        for s in ("hip_train", "hip_train_norm", "hip_train_stem"):
            setattr(m, s, True)
    return m


def _batch(name):
    size = 32 if name == "resnet18" else 224
    gen = torch.Generator().manual_seed(1)
    return {"anchor": torch.randn(8, 3, size, size, generator=gen).cuda(),
            "pos1": torch.randn(8, 3, size, size, generator=gen).cuda()}


def _step(model, opt, scaler, batch):
    from hcir.pretrain_engine import SHAMTrainStep
    step = SHAMTrainStep(model, opt, scaler, warm_up_epochs=2)
    torch.manual_seed(77)                                  # the step's random negatives, angle, sigma and mask keys
    # a ResNet's momentum forward is torch's (MIOpen): pinned to its deterministic algorithms, as
    # tests/test_resnet_train_stem_gpu.py does, so that the twin's loss dict can be compared for equality
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        return step(batch, epoch=0, batch_id=0)


def _torch_pair(model):
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (no_decay if (n.endswith(".bias") or "bn" in n or "norm" in n) else decay).append(p)
    opt = torch.optim.Adam([{"params": decay, "weight_decay": WD}, {"params": no_decay, "weight_decay": 0.0}], LR,
                           betas=(0.9, 0.999))
    return opt, torch.amp.GradScaler("cuda", init_scale=INIT_SCALE)


@pytest.mark.parametrize("name", ["resnet18", "vit_b_16"])
def test_one_fused_step_against_float64_and_the_torch_twin(name):
    from hcir import optim
    model = _model(name)
    twin = copy.deepcopy(model)
    batch = _batch(name)
    opt = optim.get_optimizer(model, LR, WD, 0.9, 0.999)
    scaler = optim.GradScaler(init_scale=INIT_SCALE)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    before = {n: p.detach().clone() for n, p in named}
    versions = {n: p._version for n, p in named}
    calls = dict(clip=0, adam=0, unscale=0)

    def counting(key, real):
        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.nn.utils, "clip_grad_norm_", counting("clip", torch.nn.utils.clip_grad_norm_))
        mp.setattr(torch.optim.Adam, "step", counting("adam", torch.optim.Adam.step))
        mp.setattr(torch, "_amp_foreach_non_finite_check_and_unscale_",
                   counting("unscale", torch._amp_foreach_non_finite_check_and_unscale_))
        out = _step(model, opt, scaler, batch)
    assert calls == dict(clip=0, adam=0, unscale=0)
    # the float64 tail on the gradients the step left: scaled by the loss scale, unclipped
    wd_of = {id(p): g["weight_decay"] for g in opt.param_groups for p in g["params"]}
    ts = []
    for n, p in named:
        assert p.grad is not None and p._version > versions[n], n
        z = torch.zeros_like(p).flatten()
        ts.append(dict(p=before[n].flatten(), g=p.grad.flatten(), m=z, v=z, step=0, wd=wd_of[id(p)], lr=LR))
    cfg = R.Cfg(scale=INIT_SCALE)
    r64 = R.tail64(ts, cfg)
    bnd = R.bounds(ts, r64, cfg)
    assert not r64["found_inf"]
    worst = dict(p=0.0, m=0.0, v=0.0)
    for (n, p), o, b in zip(named, r64["out"], bnd["out"]):
        st = opt.state[p]
        assert float(st["step"]) == 1.0
        for k, got in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            w = R.worst_ratio(got.flatten(), o[k], b[k])
            worst[k] = max(worst[k], w)
            assert w <= 1.0, (n, k, w)
    print(f"{name}: worst err / bound {worst}, unscaled norm {r64['norm']:.4f}, clip {r64['coef']:.4f}")
    # the twin: torch's optimizer, scaler and clip on a deep copy, the same batch and seeds
    topt, tscaler = _torch_pair(twin)
    tout = _step(twin, topt, tscaler, batch)
    assert tout == out, (tout, out)
    assert tscaler.get_scale() == scaler.get_scale() == INIT_SCALE
    assert tscaler._get_growth_tracker() == scaler._get_growth_tracker() == 1
    # step_scaled issues no synchronising call, with the table rebuilt (the gradients moved, as they do in a loop that
    # frees them every step) and with the table cached: both run under torch's sync debug mode, which raises on
    # .item(), .tolist(), blocking copies and stream synchronisation
    for _, p in named:
        p.grad = p.grad.clone()
    rebuilds = opt.table_rebuilds
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()            # the mode works on this build
        norm = opt.step_scaled(scaler, max_norm=1.0)
        assert opt.table_rebuilds == rebuilds + 1
        opt.step_scaled(scaler, max_norm=1.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.table_rebuilds == rebuilds + 1
    assert abs(float(norm) - r64["norm"]) <= bnd["norm"]   # the same gradients: the same norm


def test_clip_set_that_differs_from_the_models_raises():
    from hcir import optim
    from hcir.optim import HcirError
    model = _model("resnet18")
    batch = _batch("resnet18")
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    left_out = named[-1][0]
    opt = optim.Adam([p for n, p in named[:-1]], lr=LR)
    with pytest.raises(HcirError, match=left_out.replace(".", r"\.")):
        _step(model, opt, optim.GradScaler(init_scale=INIT_SCALE), batch)
    assert all(not opt.state[p] for _, p in named[:-1] if p in opt.state)      # nothing was stepped
    # the other direction: an optimizer parameter with a gradient that model.parameters() does not have
    # (the model's gradients are those of the backward above; the step zeroes gradients first, so the check itself)
    from hcir.pretrain_engine import SHAMTrainStep
    extra = torch.zeros(3, device="cuda", requires_grad=True)
    extra.grad = torch.ones(3, device="cuda")
    opt = optim.Adam([p for _, p in named] + [extra], lr=LR)
    with pytest.raises(HcirError, match="not in model.parameters"):
        SHAMTrainStep(model, opt, None)._check_clip_set()
    SHAMTrainStep(model, optim.Adam([p for _, p in named], lr=LR), None)._check_clip_set()      # equal sets pass
