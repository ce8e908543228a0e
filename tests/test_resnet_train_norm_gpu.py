"""The `hip_train_norm` switch on top of `hip_train`: a ResNet-18 / ResNet-50 trunk in train mode with its body
convolutions AND its body BatchNorm2d + residual + ReLU on the HIP kernels (hcir.conv_train.train_trunk_fused) against a
float64 ground truth.  The frame, sizes and bars of tests/test_resnet_train_gpu.py:

Ground truth G: a deep copy of the trunk on the CPU in float64, loss = (features * fixed random matrix).sum().
e_ref = the error against G of torch under torch.autocast(fp16) on the GPU with both switches off; e_fused = the same
with both on.

    over the concatenated trunk gradient, the features, the concatenated running means     e_fused <= 2 e_ref
    for every single tensor                                                               e_fused <= max(2 e_ref, 1e-2)

Measured values: DESIGN.md §3.4."""
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
    import torch.nn.functional as F
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

    assert ref_m.hip_train is False and ref_m.hip_train_norm is False
    REF = _run(autocast_features, ref_m.backbone, x.cuda(), rmat)

    hip_m = copy.deepcopy(m).cuda().train()
    hip_m.hip_train = hip_m.hip_train_norm = True
    calls = {"bn_fwd": 0, "bn_bwd": 0, "wgrad": 0, "torch_bn": 0}

    def counted(key, real):
        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "bn2d_fwd", counted("bn_fwd", ops.bn2d_fwd))
        mp.setattr(ops, "bn2d_bwd", counted("bn_bwd", ops.bn2d_bwd))
        mp.setattr(ops, "conv2d_wgrad", counted("wgrad", ops.conv2d_wgrad))
        mp.setattr(F, "batch_norm", counted("torch_bn", F.batch_norm))
        HIP = _run(hip_m.extract_features, hip_m.backbone, x.cuda(), rmat)
    nbt = [int(b) for n, b in hip_m.backbone.named_buffers() if n.endswith("num_batches_tracked")]
    _RESULTS[name] = dict(G=G, REF=REF, HIP=HIP, calls=calls, body_convs=len(layer_table(m.backbone)), nbt=nbt)
    return _RESULTS[name]


def _cat(d):
    return torch.cat([d[k].flatten() for k in sorted(d)])


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_gradients_vs_float64(name):
    r = _results(name)
    (fg, gg, _), (fr, gr, _), (fh, gh, _) = r["G"], r["REF"], r["HIP"]
    assert set(gh) == set(gg) and all(torch.isfinite(v).all() for v in gh.values())
    rows = [(n, rel(gr[n], gg[n]), rel(gh[n], gg[n])) for n in gg]
    e_ref_all, e_hip_all = rel(_cat(gr), _cat(gg)), rel(_cat(gh), _cat(gg))
    e_ref_f, e_hip_f = rel(fr, fg), rel(fh, fg)
    print(f"{name}: features e_ref {e_ref_f:.3e} e_fused {e_hip_f:.3e}; whole trunk gradient e_ref {e_ref_all:.3e} "
          f"e_fused {e_hip_all:.3e}")
    worst = max(rows, key=lambda t: t[2] / max(t[1], 1e-30))
    print(f"{name}: worst parameter by ratio {worst[0]}: e_ref {worst[1]:.3e} e_fused {worst[2]:.3e}; largest e_ref "
          f"{max(t[1] for t in rows):.3e}, largest e_fused {max(t[2] for t in rows):.3e}")
    for n, e_ref, e_hip in rows:
        print(f"  {n}: e_ref {e_ref:.3e} e_fused {e_hip:.3e}")
    assert e_hip_f <= 2.0 * e_ref_f
    assert e_hip_all <= 2.0 * e_ref_all
    for n, e_ref, e_hip in rows:
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_fused {e_hip:.3e}, e_ref {e_ref:.3e}"


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_statistics_and_kernel_use(name):
    r = _results(name)
    mg, mr, mh = r["G"][2], r["REF"][2], r["HIP"][2]
    assert r["nbt"] and all(v == 1 for v in r["nbt"])            # every BatchNorm, the stem's too, saw exactly one batch
    e_ref_all, e_hip_all = rel(_cat(mr), _cat(mg)), rel(_cat(mh), _cat(mg))
    print(f"{name}: running means e_ref {e_ref_all:.3e} e_fused {e_hip_all:.3e}")
    assert e_hip_all <= 2.0 * e_ref_all
    for n in mg:
        e_ref, e_hip = rel(mr[n], mg[n]), rel(mh[n], mg[n])
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_fused {e_hip:.3e}, e_ref {e_ref:.3e}"
    # one HIP BatchNorm per body convolution (layer_table's count), forward and backward; torch's only for the stem
    body = 20 - 1 if name == "resnet18" else 53 - 1
    c = r["calls"]
    assert r["body_convs"] == body
    assert c["bn_fwd"] == c["bn_bwd"] == c["wgrad"] == body
    assert c["torch_bn"] == 1


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_one_block_vs_float64(name):
    """layer3.0 alone (stride 2, a downsample branch: every bn_act_nhwc form - ReLU, plain, residual + ReLU) at
    4 x 14 x 14, where 196 values per channel after the stride make the comparison sharp."""
    from hcir import conv_train
    blk = _new_model(name, seed=31).backbone[6][0]
    cin = blk.conv1.in_channels
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(4, cin, 14, 14, generator=gen).half()        # fp16-representable: every path starts from it
    rmat = torch.randn(4, blk.downsample[0].out_channels, 7, 7, generator=gen).double()

    def run(b, forward, xin, nhwc=False):
        xin = xin.requires_grad_(True)
        out = forward(xin)
        if nhwc:
            out = out.permute(0, 3, 1, 2)
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
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()
    o_hip, g_hip = run(hip_b, lambda t: conv_train._block_fused(hip_b, t), x_nhwc, nhwc=True)
    e_ref_o, e_hip_o = rel(o_ref, o64), rel(o_hip, o64)
    e_ref_all, e_hip_all = rel(_cat(g_ref), _cat(g64)), rel(_cat(g_hip), _cat(g64))
    print(f"{name} layer3.0: output e_ref {e_ref_o:.3e} e_fused {e_hip_o:.3e}; all gradients e_ref {e_ref_all:.3e} "
          f"e_fused {e_hip_all:.3e}")
    rows = [(n, rel(g_ref[n], g64[n]), rel(g_hip[n], g64[n])) for n in g64]
    for n, e_ref, e_hip in rows:
        print(f"  {n}: e_ref {e_ref:.3e} e_fused {e_hip:.3e}")
    assert e_hip_o <= 2.0 * e_ref_o
    assert e_hip_all <= 2.0 * e_ref_all
    for n, e_ref, e_hip in rows:
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_fused {e_hip:.3e}, e_ref {e_ref:.3e}"
    assert all(int(b) == 1 for n, b in hip_b.named_buffers() if n.endswith("num_batches_tracked"))


def _boom(which):
    def f(trunk, t):
        raise AssertionError(f"{which} entered")
    return f


def test_norm_switch_alone_is_inert():
    """hip_train_norm = True with hip_train = False: neither walk is entered, the call is the torch path bit for bit."""
    from hcir import main_backbone
    m = _new_model("resnet18").cuda()
    assert m.hip_train is False and m.hip_train_norm is False
    m.hip_train_norm = True
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(1)).cuda()
    # both sides of the torch.equal are the torch / MIOpen path: pin its algorithm choice so that the comparison is
    # about the switch alone (the framing of tests/test_resnet_train_gpu.py::test_switch_off_is_inert)
    with pytest.MonkeyPatch.context() as mp, torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                                                       deterministic=True):
        mp.setattr(main_backbone, "train_trunk", _boom("train_trunk"))
        mp.setattr(main_backbone, "train_trunk_fused", _boom("train_trunk_fused"))
        for _ in range(2):
            m.backbone(x)
        a = m(x)
        b = m.projection_head(m.backbone(x).flatten(1))
        assert a.requires_grad and torch.equal(a, b)
        assert torch.equal(m.extract_features(x), m.backbone(x).flatten(1))


def test_both_switches_apply_only_to_train_mode_with_autograd():
    from hcir import main_backbone
    m = _new_model("resnet18").cuda()
    m.hip_train = m.hip_train_norm = True
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(2)).cuda()
    entered = []
    real = main_backbone.train_trunk_fused
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(main_backbone, "train_trunk", _boom("train_trunk"))
        mp.setattr(main_backbone, "train_trunk_fused", lambda trunk, t: entered.append(trunk) or real(trunk, t))
        with torch.no_grad():
            m.extract_features(x), m(x), m.forward_momentum(x), m.extract_features_ema(x)
        assert entered == []
        m.eval()
        f = m.extract_features(x)
        assert entered == [] and f.requires_grad          # eval mode: torch's differentiable path, running statistics
        m.train()
        f = m.extract_features(x)
        assert len(entered) == 1 and entered[0] is m.backbone and f.requires_grad and f.dtype == torch.float32


def test_conv_switch_alone_takes_the_unfused_walk():
    from hcir import main_backbone
    m = _new_model("resnet18").cuda()
    m.hip_train = True
    assert m.hip_train_norm is False
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).cuda()
    entered = []
    real = main_backbone.train_trunk
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(main_backbone, "train_trunk", lambda trunk, t: entered.append(trunk) or real(trunk, t))
        mp.setattr(main_backbone, "train_trunk_fused", _boom("train_trunk_fused"))
        f = m.extract_features(x)
    assert len(entered) == 1 and entered[0] is m.backbone and f.requires_grad


def test_simclr_model_has_the_switch_too():
    from hcir import backbone
    from hcir.backbone import SimCLR
    torch.manual_seed(4)
    m = SimCLR("resnet18").cuda().train()
    m.hip_train = m.hip_train_norm = True
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(4)).cuda()
    entered = []
    real = backbone.train_trunk_fused
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(backbone, "train_trunk", _boom("train_trunk"))
        mp.setattr(backbone, "train_trunk_fused", lambda trunk, t: entered.append(trunk) or real(trunk, t))
        out = m(x)
    assert len(entered) == 1 and out.requires_grad and torch.isfinite(out).all()


def test_one_train_step_resnet18():
    """One SHAMTrainStep step with both switches on, a GradScaler, B = 8 at 32 x 32 (the masking transform's patch is
    32: the smallest image the step's transforms accept)."""
    from hcir.main_backbone import SHAM2
    from hcir.pretrain_engine import SHAMTrainStep
    torch.manual_seed(9)
    model = SHAM2("resnet18").cuda()
    model.hip_train = model.hip_train_norm = True
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
