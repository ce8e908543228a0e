"""The frame shared by tests/test_resnet_train_gpu.py (`hip_train`) and tests/test_resnet_train_norm_gpu.py (`hip_train`
+ `hip_train_norm`): a ResNet-18 / ResNet-50 trunk in train mode on the HIP kernels (hcir.conv_train) against a float64
ground truth.

Ground truth G: a deep copy of the trunk on the CPU in float64, loss = (features * fixed random matrix).sum().
e_ref = the error against G of torch under torch.autocast(fp16) on the GPU with every switch off (the reference's way,
HP/src/pretrain_engine.py:681); e_hip = the same with the switches under test on.  Both round the same operands to fp16
and differ only in summation order and in where activations are rounded, so

    over the concatenated gradient, the concatenated running means     e_hip <= 2 e_ref
    for every single tensor                                            e_hip <= max(2 e_ref, 1e-2)
    for the features / the block's output                              e_hip <= max(2 e_ref, out_floor)

(1e-2: the project's bar for the ViT's backbone gradients, tests/test_vit_train_gpu.py; out_floor is each file's own:
1e-2 with `hip_train` alone, 0 with both switches).  A wrong tap, a missing flip or a lost split gives an error of
order 1.  Measured values: DESIGN.md §3.4.  Test infrastructure, like tests/_fp64.py: no test lives here."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from _fp64 import rel

B, SIZE = 4, 64


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def new_model(name, seed=21):
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


def switch_on(m, switches):
    for s in switches:
        assert getattr(m, s) is False                      # every switch defaults to off
        setattr(m, s, True)
    return m


def run(trunk_features, trunk, x, rmat):
    """features, {name: grad} and {name: running_mean} after one forward + backward of loss = (f * rmat).sum()."""
    for p in trunk.parameters():
        p.grad = None
    f = trunk_features(x)
    (f.double() * rmat.to(f.device)).sum().backward()
    grads = {n: p.grad.detach().cpu().double() for n, p in trunk.named_parameters()}
    means = {n: b.detach().cpu().double() for n, b in trunk.named_buffers() if n.endswith("running_mean")}
    return f.detach().cpu().double(), grads, means


_RESULTS = {}


def results(name, switches, counted):
    """One ground truth and the two device runs per trunk and set of switches, shared by a file's tests.  `counted`
    maps a label to the (namespace, attribute) of a function whose calls during the switched-on run are counted."""
    if (name, switches) in _RESULTS:
        return _RESULTS[name, switches]
    from hcir.resnet_engine import layer_table
    m = new_model(name)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, SIZE, SIZE, generator=gen)
    dim = 512 if name == "resnet18" else 2048
    rmat = torch.randn(B, dim, generator=gen).double()

    truth = copy.deepcopy(m.backbone).double().train()
    G = run(lambda t: truth(t).flatten(1), truth, x.double(), rmat)

    ref_m = copy.deepcopy(m).cuda().train()

    def autocast_features(t):
        with torch.autocast("cuda", dtype=torch.float16):
            return ref_m.extract_features(t)

    assert ref_m.hip_train is False and ref_m.hip_train_norm is False
    REF = run(autocast_features, ref_m.backbone, x.cuda(), rmat)

    hip_m = switch_on(copy.deepcopy(m).cuda().train(), switches)
    calls = dict.fromkeys(counted, 0)

    def counting(key, real):
        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f

    with pytest.MonkeyPatch.context() as mp:
        for key, (where, attr) in counted.items():
            mp.setattr(where, attr, counting(key, getattr(where, attr)))
        HIP = run(hip_m.extract_features, hip_m.backbone, x.cuda(), rmat)
    nbt = [int(b) for n, b in hip_m.backbone.named_buffers() if n.endswith("num_batches_tracked")]
    _RESULTS[name, switches] = dict(G=G, REF=REF, HIP=HIP, calls=calls, body_convs=len(layer_table(m.backbone)),
                                    nbt=nbt)
    return _RESULTS[name, switches]


def cat(d):
    return torch.cat([d[k].flatten() for k in sorted(d)])


def check(title, label, what, out, tensors, out_floor=None):
    """Print and assert the criterion of the module docstring: `out` = (truth, reference, HIP) of the features or the
    block's output (None: no such term), `tensors` = the same three as {name: tensor} (`what` names them)."""
    t64, t_ref, t_hip = tensors
    assert set(t_hip) == set(t64) and all(torch.isfinite(v).all() for v in t_hip.values())
    rows = [(n, rel(t_ref[n], t64[n]), rel(t_hip[n], t64[n])) for n in t64]
    e_ref_all, e_hip_all = rel(cat(t_ref), cat(t64)), rel(cat(t_hip), cat(t64))
    if out is not None:
        e_ref_o, e_hip_o = rel(out[1], out[0]), rel(out[2], out[0])
        print(f"{title}: output e_ref {e_ref_o:.3e} {label} {e_hip_o:.3e}")
    print(f"{title}: {what} e_ref {e_ref_all:.3e} {label} {e_hip_all:.3e}")
    worst = max(rows, key=lambda t: t[2] / max(t[1], 1e-30))
    print(f"{title}: worst by ratio {worst[0]}: e_ref {worst[1]:.3e} {label} {worst[2]:.3e}; largest e_ref "
          f"{max(t[1] for t in rows):.3e}, largest {label} {max(t[2] for t in rows):.3e}")
    for n, e_ref, e_hip in rows:
        print(f"  {n}: e_ref {e_ref:.3e} {label} {e_hip:.3e}")
    if out is not None:
        assert e_hip_o <= max(2.0 * e_ref_o, out_floor)
    assert e_hip_all <= 2.0 * e_ref_all
    for n, e_ref, e_hip in rows:
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: {label} {e_hip:.3e}, e_ref {e_ref:.3e}"


def check_trunk_gradients(name, r, label, out_floor):
    (fg, gg, _), (fr, gr, _), (fh, gh, _) = r["G"], r["REF"], r["HIP"]
    check(name, label, "whole trunk gradient", (fg, fr, fh), (gg, gr, gh), out_floor)


def check_trunk_statistics(name, r, label):
    assert r["nbt"] and all(v == 1 for v in r["nbt"])      # every BatchNorm, the stem's too, saw exactly one batch
    check(name, label, "running means", None, (r["G"][2], r["REF"][2], r["HIP"][2]))


def check_one_block(name, norm, label, out_floor):
    """layer3.0 alone - stride 2 with a downsample branch, so both stride-2 data-gradient plans, the residual wiring
    and every form of `norm` (ReLU, plain, residual + ReLU) - through resnet_engine.block_table and conv_train.walk
    with conv_train's `norm`.  The whole-trunk comparison is only as sharp as e_ref, and at B = 4 and 64 x 64 the last
    stages normalise over 16 to 64 values per channel: e_ref itself is large there.  At 4 x 14 x 14 (196 values per
    channel after the stride) the block is well conditioned, and the same criterion separates rounding from a wrong
    tap."""
    from hcir import conv_train
    from hcir.resnet_engine import block_table
    blk = new_model(name, seed=31).backbone[6][0]
    cin = blk.conv1.in_channels
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(4, cin, 14, 14, generator=gen).half()        # fp16-representable: every path starts from it
    rmat = torch.randn(4, blk.downsample[0].out_channels, 7, 7, generator=gen).double()

    def run_block(b, forward, xin, nhwc=False):
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
    o64, g64 = run_block(truth, truth, x.double())
    ref_b = copy.deepcopy(blk).cuda().train()

    def autocast_block(t):
        with torch.autocast("cuda", dtype=torch.float16):
            return ref_b(t)

    o_ref, g_ref = run_block(ref_b, autocast_block, x.float().cuda())
    hip_b = copy.deepcopy(blk).cuda().train()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()           # a plain NHWC leaf
    o_hip, g_hip = run_block(hip_b, lambda t: conv_train.walk(block_table(hip_b), t, norm=getattr(conv_train, norm)),
                             x_nhwc, nhwc=True)
    check(f"{name} layer3.0", label, "all gradients", (o64, o_ref, o_hip), (g64, g_ref, g_hip), out_floor)
    assert all(int(b) == 1 for n, b in hip_b.named_buffers() if n.endswith("num_batches_tracked"))


@contextlib.contextmanager
def spy_train_trunk(forbid=False):
    """Patches the one seam between the models and the walk - train_trunk where HipTrunkSwitches looks it up - and
    yields the list of (trunk, fused_norm) it was entered with; `forbid` makes entering it an error."""
    from hcir import main_backbone
    entered, real = [], main_backbone.train_trunk

    def spy(trunk, t, fused_norm=False):
        if forbid:
            raise AssertionError("train_trunk entered")
        entered.append((trunk, fused_norm))
        return real(trunk, t, fused_norm=fused_norm)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(main_backbone, "train_trunk", spy)
        yield entered


def check_one_train_step(switches):
    """One SHAMTrainStep step of a ResNet-18 with `switches` on, a GradScaler, B = 8 at 32 x 32 (the masking
    transform's patch is 32: the smallest image the step's transforms accept)."""
    from hcir.main_backbone import SHAM2
    from hcir.pretrain_engine import SHAMTrainStep
    torch.manual_seed(9)
    model = switch_on(SHAM2("resnet18").cuda(), switches)
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
