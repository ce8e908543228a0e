"""The `hip_train_norm` switch on top of `hip_train`: a ResNet-18 / ResNet-50 trunk in train mode with its body
convolutions AND its body BatchNorm2d + residual + ReLU on the HIP kernels (hcir.conv_train, the walk with bn_act_nhwc)
against a float64 ground truth.  The frame, sizes and criterion are tests/_resnet_train_frame.py's; here the features
and the block's output are held, like the concatenated gradient, to

    e_fused <= 2 e_ref

Measured values: DESIGN.md §3.4."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_train_frame as frame  # noqa: E402
from _resnet_train_frame import B, SIZE, _gpu  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SWITCHES = ("hip_train", "hip_train_norm")
OUT_FLOOR = 0.0


def _results(name):
    import torch.nn.functional as F
    from hcir import ops
    return frame.results(name, SWITCHES, {"bn_fwd": (ops, "bn2d_fwd"), "bn_bwd": (ops, "bn2d_bwd"),
                                          "wgrad": (ops, "conv2d_wgrad"), "torch_bn": (F, "batch_norm")})


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_gradients_vs_float64(name):
    frame.check_trunk_gradients(name, _results(name), "e_fused", OUT_FLOOR)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_statistics_and_kernel_use(name):
    r = _results(name)
    frame.check_trunk_statistics(name, r, "e_fused")
    # one HIP BatchNorm per body convolution (layer_table's count), forward and backward; torch's only for the stem
    body = 20 - 1 if name == "resnet18" else 53 - 1
    c = r["calls"]
    assert r["body_convs"] == body
    assert c["bn_fwd"] == c["bn_bwd"] == c["wgrad"] == body
    assert c["torch_bn"] == 1


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_one_block_vs_float64(name):
    frame.check_one_block(name, "bn_act_nhwc", "e_fused", OUT_FLOOR)


def test_norm_switch_alone_is_inert():
    """hip_train_norm = True with hip_train = False: the walk is not entered, the call is the torch path bit for bit."""
    m = frame.new_model("resnet18").cuda()
    assert m.hip_train is False and m.hip_train_norm is False
    m.hip_train_norm = True
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(1)).cuda()
    # both sides of the torch.equal are the torch / MIOpen path: pin its algorithm choice so that the comparison is
    # about the switch alone (the framing of tests/test_resnet_train_gpu.py::test_switch_off_is_inert)
    with frame.spy_train_trunk(forbid=True), torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                                                        deterministic=True):
        for _ in range(2):
            m.backbone(x)
        a = m(x)
        b = m.projection_head(m.backbone(x).flatten(1))
        assert a.requires_grad and torch.equal(a, b)
        assert torch.equal(m.extract_features(x), m.backbone(x).flatten(1))


def test_both_switches_apply_only_to_train_mode_with_autograd():
    m = frame.switch_on(frame.new_model("resnet18").cuda(), SWITCHES)
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(2)).cuda()
    with frame.spy_train_trunk() as entered:
        with torch.no_grad():
            m.extract_features(x), m(x), m.forward_momentum(x), m.extract_features_ema(x)
        assert entered == []
        m.eval()
        f = m.extract_features(x)
        assert entered == [] and f.requires_grad          # eval mode: torch's differentiable path, running statistics
        m.train()
        f = m.extract_features(x)
        assert len(entered) == 1 and entered[0][0] is m.backbone and f.requires_grad and f.dtype == torch.float32
        assert entered[0][1] is True                      # both switches: the fused walk, never the unfused one


def test_conv_switch_alone_takes_the_unfused_walk():
    m = frame.switch_on(frame.new_model("resnet18").cuda(), ("hip_train",))
    assert m.hip_train_norm is False
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).cuda()
    with frame.spy_train_trunk() as entered:
        f = m.extract_features(x)
    assert len(entered) == 1 and entered[0][0] is m.backbone and f.requires_grad
    assert entered[0][1] is False


def test_simclr_model_has_the_switch_too():
    from hcir.backbone import SimCLR
    torch.manual_seed(4)
    m = frame.switch_on(SimCLR("resnet18").cuda().train(), SWITCHES)
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(4)).cuda()
    with frame.spy_train_trunk() as entered:
        out = m(x)
    assert len(entered) == 1 and entered[0][1] is True and out.requires_grad and torch.isfinite(out).all()
    assert entered[0][0] is m.backbone


def test_one_train_step_resnet18():
    frame.check_one_train_step(SWITCHES)
