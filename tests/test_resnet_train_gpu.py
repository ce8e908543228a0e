"""The `hip_train` switch: a ResNet-18 / ResNet-50 trunk in train mode with its body convolutions, forward and
backward, on the HIP kernels (hcir.conv_train) against a float64 ground truth.

Ground truth G: a deep copy of the trunk on the CPU in float64, loss = (features * fixed random matrix).sum().
e_ref = the error against G of torch under torch.autocast(fp16) on the GPU with the switch off (the reference's way,
HP/src/pretrain_engine.py:681; existing code); e_hip = the same with the switch on.  Both round the same operands to
fp16 and differ only in summation order and in where activations are rounded, so

    over the concatenated trunk gradient     e_hip <= 2 e_ref
    for every single tensor                  e_hip <= max(2 e_ref, 1e-2)

(1e-2: the project's bar for the ViT's backbone gradients, tests/test_vit_train_gpu.py).  A wrong tap, a missing flip
or a lost split gives an error of order 1.  Measured values: DESIGN.md §3.4."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fp64 import rel  # noqa: E402

pytestmark = pytest.mark.gpu

B, SIZE = 4, 64


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _new_model(name, seed=21):
    from hcir.main_backbone import SHAM2
    torch.manual_seed(seed)
    m = SHAM2(name)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.backbone.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
    return m.train()


def _run(trunk_features, trunk, x, rmat):
    """features, {name: grad} and {name: running_mean} after one forward + backward of loss = (f * rmat).sum()."""
    for p in trunk.parameters():
        p.grad = None
    f = trunk_features(x)
    (f.double() * rmat.to(f.device)).sum().backward()
    grads = {n: p.grad.detach().cpu().double() for n, p in trunk.named_parameters()}
    means = {n: b.detach().cpu().double() for n, b in trunk.named_buffers() if n.endswith("running_mean")}
    return f.detach().cpu().double(), grads, means


_RESULTS = {}


def _results(name):
    """One ground truth and the two device runs per trunk, shared by the tests below."""
    if name in _RESULTS:
        return _RESULTS[name]
    from hcir import ops
    from hcir.resnet_engine import layer_table
    m = _new_model(name)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, SIZE, SIZE, generator=gen)
    dim = 512 if name == "resnet18" else 2048
    rmat = torch.randn(B, dim, generator=gen).double()

    truth = copy.deepcopy(m.backbone).double().train()
    G = _run(lambda t: truth(t).flatten(1), truth, x.double(), rmat)

    ref_m = copy.deepcopy(m).cuda().train()

    def autocast_features(t):
        with torch.autocast("cuda", dtype=torch.float16):
            return ref_m.extract_features(t)

    assert ref_m.hip_train is False
    REF = _run(autocast_features, ref_m.backbone, x.cuda(), rmat)

    hip_m = copy.deepcopy(m).cuda().train()
    hip_m.hip_train = True
    calls = []
    real = ops.conv2d_wgrad
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "conv2d_wgrad", lambda *a, **k: calls.append(1) or real(*a, **k))
        HIP = _run(hip_m.extract_features, hip_m.backbone, x.cuda(), rmat)
    nbt = [int(b) for n, b in hip_m.backbone.named_buffers() if n.endswith("num_batches_tracked")]
    _RESULTS[name] = dict(G=G, REF=REF, HIP=HIP, wgrad_calls=len(calls), body_convs=len(layer_table(m.backbone)),
                          nbt=nbt)
    return _RESULTS[name]


def _cat(d):
    return torch.cat([d[k].flatten() for k in sorted(d)])


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_gradients_vs_float64(name):
    r = _results(name)
    (fg, gg, _), (fr, gr, _), (fh, gh, _) = r["G"], r["REF"], r["HIP"]
    assert set(gh) == set(gg) and all(torch.isfinite(v).all() for v in gh.values())
    rows = []
    for n in gg:
        rows.append((n, rel(gr[n], gg[n]), rel(gh[n], gg[n])))
    e_ref_all, e_hip_all = rel(_cat(gr), _cat(gg)), rel(_cat(gh), _cat(gg))
    e_ref_f, e_hip_f = rel(fr, fg), rel(fh, fg)
    print(f"{name}: features e_ref {e_ref_f:.3e} e_hip {e_hip_f:.3e}; whole trunk gradient e_ref {e_ref_all:.3e} "
          f"e_hip {e_hip_all:.3e}")
    worst = max(rows, key=lambda t: t[2] / max(t[1], 1e-30))
    print(f"{name}: worst parameter by ratio {worst[0]}: e_ref {worst[1]:.3e} e_hip {worst[2]:.3e}; largest e_ref "
          f"{max(t[1] for t in rows):.3e}, largest e_hip {max(t[2] for t in rows):.3e}")
    for n, e_ref, e_hip in rows:
        print(f"  {n}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip_f <= max(2.0 * e_ref_f, 1e-2)
    assert e_hip_all <= 2.0 * e_ref_all
    for n, e_ref, e_hip in rows:
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}"


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_statistics_and_kernel_use(name):
    r = _results(name)
    mg, mr, mh = r["G"][2], r["REF"][2], r["HIP"][2]
    assert r["nbt"] and all(v == 1 for v in r["nbt"])            # every BatchNorm saw exactly one batch
    e_ref_all, e_hip_all = rel(_cat(mr), _cat(mg)), rel(_cat(mh), _cat(mg))
    print(f"{name}: running means e_ref {e_ref_all:.3e} e_hip {e_hip_all:.3e}")
    assert e_hip_all <= 2.0 * e_ref_all
    for n in mg:
        e_ref, e_hip = rel(mr[n], mg[n]), rel(mh[n], mg[n])
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}"
    assert r["wgrad_calls"] == r["body_convs"] == (20 - 1 if name == "resnet18" else 53 - 1)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_one_block_vs_float64(name):
    """The whole-trunk comparison above is only as sharp as e_ref, and at B = 4 and 64 x 64 the last stages normalise
    over 16 to 64 values per channel: e_ref itself is large there.  One block - layer3.0, stride 2 with a downsample
    branch, so both stride-2 data-gradient plans and the residual wiring - at 4 x 14 x 14 (196 values per channel
    after the stride) is well conditioned, and the same criterion then separates rounding from a wrong tap."""
    from hcir import conv_train
    blk = _new_model(name, seed=31).backbone[6][0]
    cin = blk.conv1.in_channels
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(4, cin, 14, 14, generator=gen).half()        # fp16-representable: every path starts from it
    rmat = torch.randn(4, blk.downsample[0].out_channels, 7, 7, generator=gen).double()

    def run(b, forward, xin, nhwc=False):
        xin = xin.requires_grad_(True)
        out = forward(xin)
        (out.double() * rmat.to(out.device)).sum().backward()
        g = {n: p.grad.detach().cpu().double() for n, p in b.named_parameters()}
        dx = xin.grad.detach().cpu().double()
        g["input"] = dx.permute(0, 3, 1, 2) if nhwc else dx
        return out.detach().cpu().double(), g

    truth = copy.deepcopy(blk).double().train()
    o64, g64 = run(truth, truth, x.double())
    ref_b = copy.deepcopy(blk).cuda().train()

    def autocast_block(t):
        with torch.autocast("cuda", dtype=torch.float16):
            return ref_b(t)

    o_ref, g_ref = run(ref_b, autocast_block, x.float().cuda())
    hip_b = copy.deepcopy(blk).cuda().train()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()           # NHWC leaf; the block sees its [B,C,H,W] view
    o_hip, g_hip = run(hip_b, lambda t: conv_train._block(hip_b, t.permute(0, 3, 1, 2)), x_nhwc,
                       nhwc=True)
    e_ref_o, e_hip_o = rel(o_ref, o64), rel(o_hip, o64)
    e_ref_all, e_hip_all = rel(_cat(g_ref), _cat(g64)), rel(_cat(g_hip), _cat(g64))
    print(f"{name} layer3.0: output e_ref {e_ref_o:.3e} e_hip {e_hip_o:.3e}; all gradients e_ref {e_ref_all:.3e} "
          f"e_hip {e_hip_all:.3e}")
    for n in g64:
        e_ref, e_hip = rel(g_ref[n], g64[n]), rel(g_hip[n], g64[n])
        print(f"  {n}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip_o <= max(2.0 * e_ref_o, 1e-2)
    assert e_hip_all <= 2.0 * e_ref_all
    for n in g64:
        e_ref, e_hip = rel(g_ref[n], g64[n]), rel(g_hip[n], g64[n])
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}"


def test_switch_off_is_inert():
    """hip_train defaults to False, and with it off a train-mode, autograd-on call is the torch path bit for bit."""
    from hcir import main_backbone
    m = _new_model("resnet18").cuda()
    assert m.hip_train is False
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(1)).cuda()

    def boom(trunk, t):
        raise AssertionError("train_trunk entered")

    # both sides of the torch.equal are the torch / MIOpen path: pin its algorithm choice (the first call of a shape
    # may pick another kernel than the later ones) so that the comparison is about the switch alone
    with pytest.MonkeyPatch.context() as mp, torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                                                       deterministic=True):
        mp.setattr(main_backbone, "train_trunk", boom)
        for _ in range(2):
            m.backbone(x)
        a = m(x)
        b = m.projection_head(m.backbone(x).flatten(1))
        assert a.requires_grad and torch.equal(a, b)
        assert torch.equal(m.extract_features(x), m.backbone(x).flatten(1))


def test_switch_on_applies_only_to_train_mode_with_autograd():
    from hcir import main_backbone
    m = _new_model("resnet18").cuda()
    m.hip_train = True
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(2)).cuda()
    entered = []
    real = main_backbone.train_trunk
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(main_backbone, "train_trunk", lambda trunk, t: entered.append(trunk) or real(trunk, t))
        with torch.no_grad():
            m.extract_features(x), m(x), m.forward_momentum(x), m.extract_features_ema(x)
        assert entered == []
        m.eval()
        f = m.extract_features(x)
        assert entered == [] and f.requires_grad          # eval mode: torch's differentiable path, running statistics
        m.train()
        f = m.extract_features(x)
        assert len(entered) == 1 and entered[0] is m.backbone and f.requires_grad and f.dtype == torch.float32


def test_switch_on_half_input_raises_from_torch_not_from_the_engine():
    from hcir import main_backbone
    m = _new_model("resnet18").cuda()
    m.hip_train = True
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(main_backbone, "train_trunk", lambda trunk, t: (_ for _ in ()).throw(AssertionError("entered")))
        with pytest.raises(RuntimeError):
            m.extract_features(torch.zeros(2, 3, 32, 32, dtype=torch.float16, device="cuda"))
        tiny = m.extract_features(torch.zeros(2, 3, 6, 6, device="cuda"))      # H, W < 7: the torch path
        assert tuple(tiny.shape) == (2, 512)


def test_vit_ignores_the_switch():
    from hcir import main_backbone
    from hcir.main_backbone import SHAM2
    torch.manual_seed(3)
    m = SHAM2("vit_b_16").cuda().train()
    m.hip_train = True
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(3)).cuda()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(main_backbone, "train_trunk", lambda trunk, t: (_ for _ in ()).throw(AssertionError("entered")))
        f = m.extract_features(x)
    assert tuple(f.shape) == (4, 768) and f.requires_grad


def test_unexpected_trunk_is_an_error_not_another_result():
    from hcir import HcirError
    m = _new_model("resnet18").cuda()
    m.hip_train = True
    m.backbone[5][0].conv1.dilation = (2, 2)
    with pytest.raises(HcirError):
        m.extract_features(torch.zeros(2, 3, 32, 32, device="cuda"))


def test_one_train_step_resnet18():
    """One SHAMTrainStep step with the switch on, a GradScaler, B = 8 at 32 x 32 (the masking transform's patch is 32:
    the smallest image the step's transforms accept)."""
    from hcir.main_backbone import SHAM2
    from hcir.pretrain_engine import SHAMTrainStep
    torch.manual_seed(9)
    model = SHAM2("resnet18").cuda()
    model.hip_train = True
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
    gen = torch.Generator().manual_seed(1)
    batch = {"anchor": torch.randn(8, 3, 32, 32, generator=gen).cuda(),
             "pos1": torch.randn(8, 3, 32, 32, generator=gen).cuda()}
    before = {n: p.detach().clone() for n, p in model.backbone.named_parameters()}
    step = SHAMTrainStep(model, opt, scaler, warm_up_epochs=2)
    out = step(batch, epoch=0, batch_id=0)
    assert np.isfinite(out["total"])
    assert scaler.get_scale() == 256.0                    # no overflow: the optimizer step was taken
    for n, p in model.backbone.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
