"""The `hip_train_stem` switch on top of `hip_train` + `hip_train_norm`: a ResNet-18 / ResNet-50 trunk in train mode
with nothing of the stem or the body left to torch's convolution, batch norm or max pool, against a float64 ground
truth.  The frame, sizes and criteria are tests/_resnet_train_frame.py's, unchanged; the features are held, as with the
two other switches, to e_hip <= 2 e_ref (out_floor 0): the HIP stem rounds where autocast rounds - the conv's output
and the pooled map, to fp16 - and nowhere else.

Measured values: DESIGN.md §3.4."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_train_frame as frame  # noqa: E402
from _resnet_train_frame import B, SIZE, _gpu  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SWITCHES = ("hip_train", "hip_train_norm", "hip_train_stem")
OUT_FLOOR = 0.0


def _results(name):
    import torch.nn.functional as F
    from hcir import ops
    return frame.results(name, SWITCHES, {"stem_fwd": (ops, "stem_conv"), "stem_pool": (ops, "stem_bn_relu_pool"),
                                          "stem_wgrad": (ops, "stem_wgrad"), "torch_bn": (F, "batch_norm"),
                                          "torch_conv": (F, "conv2d"), "torch_pool": (F, "max_pool2d")})


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_gradients_vs_float64(name):
    frame.check_trunk_gradients(name, _results(name), "e_stem", OUT_FLOOR)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_statistics_and_kernel_use(name):
    r = _results(name)
    frame.check_trunk_statistics(name, r, "e_stem")
    c = r["calls"]
    assert c["torch_bn"] == c["torch_conv"] == c["torch_pool"] == 0
    assert c["stem_fwd"] == c["stem_pool"] == c["stem_wgrad"] == 1


def test_one_train_step_resnet18():
    frame.check_one_train_step(SWITCHES)


def test_stem_switch_alone_is_inert():
    """hip_train_stem = True with hip_train = False: the walk is not entered, the call is the torch path bit for bit."""
    m = frame.new_model("resnet18").cuda()
    assert m.hip_train is False and m.hip_train_stem is False
    m.hip_train_stem = True
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(1)).cuda()
    with frame.spy_train_trunk(forbid=True), torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                                                        deterministic=True):
        for _ in range(2):
            m.backbone(x)
        a = m(x)
        b = m.projection_head(m.backbone(x).flatten(1))
        assert a.requires_grad and torch.equal(a, b)
        assert torch.equal(m.extract_features(x), m.backbone(x).flatten(1))


def test_stem_switch_is_independent_of_the_norm_switch():
    """hip_train + hip_train_stem without hip_train_norm: the HIP stem feeds the unfused walk."""
    from hcir import conv_train, ops
    m = frame.switch_on(frame.new_model("resnet18").cuda(), ("hip_train", "hip_train_stem"))
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).cuda()
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        real_stem, real_bn = conv_train.stem_train, ops.bn2d_fwd
        mp.setattr(conv_train, "stem_train", lambda *a: (seen.append("stem"), real_stem(*a))[1])
        mp.setattr(ops, "bn2d_fwd", lambda *a, **k: (seen.append("bn"), real_bn(*a, **k))[1])
        f = m.extract_features(x)
        f.sum().backward()
    assert seen == ["stem"] and f.requires_grad and torch.isfinite(f).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.backbone.parameters())


def test_an_image_that_requires_grad_keeps_the_torch_stem():
    """There is no image-gradient kernel: with x.requires_grad the torch stem runs and x gets its gradient."""
    from hcir import conv_train
    m = frame.switch_on(frame.new_model("resnet18").cuda(), SWITCHES)
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    with pytest.MonkeyPatch.context() as mp:
        def forbidden(*a):
            raise AssertionError("stem_train entered")
        mp.setattr(conv_train, "stem_train", forbidden)
        m.extract_features(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and bool((x.grad != 0).any())


def _grads_and_features(m, x):
    for p in m.parameters():
        p.grad = None
    f = m.extract_features(x)
    f.square().sum().backward()
    return f.detach().clone(), {n: p.grad.detach().clone() for n, p in m.backbone.named_parameters()}


def test_new_switch_off_keeps_the_two_switch_path():
    """hip_train + hip_train_norm with hip_train_stem off: the walk is entered through the two-argument call the
    parent made, and features and gradients are bit-equal run to run - the stem conv's weight gradient excepted, for
    which DESIGN.md records MIOpen's own run-to-run difference."""
    m = frame.switch_on(frame.new_model("resnet18").cuda(), ("hip_train", "hip_train_norm"))
    assert m.hip_train_stem is False
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(5)).cuda()
    with frame.spy_train_trunk() as entered:                   # the spy takes (trunk, x, fused_norm) and nothing else
        fa, ga = _grads_and_features(m, x)
    assert len(entered) == 1 and entered[0][1] is True
    fb, gb = _grads_and_features(m, x)
    assert torch.equal(fa, fb)
    for n in ga:
        if n != "0.weight":
            assert torch.equal(ga[n], gb[n]), n
