"""The `hip_train` switch: a ResNet-18 / ResNet-50 trunk in train mode with its body convolutions, forward and
backward, on the HIP kernels (hcir.conv_train, the walk with torch_norm) against a float64 ground truth.  The frame,
sizes and criterion are tests/_resnet_train_frame.py's; here the features and the block's output are held to

    e_hip <= max(2 e_ref, 1e-2)

Measured values: DESIGN.md §3.4."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resnet_train_frame as frame  # noqa: E402
from _resnet_train_frame import B, SIZE, _gpu  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SWITCHES = ("hip_train",)
OUT_FLOOR = 1e-2


def _results(name):
    from hcir import ops
    return frame.results(name, SWITCHES, {"wgrad": (ops, "conv2d_wgrad")})


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_gradients_vs_float64(name):
    frame.check_trunk_gradients(name, _results(name), "e_hip", OUT_FLOOR)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_trunk_statistics_and_kernel_use(name):
    r = _results(name)
    frame.check_trunk_statistics(name, r, "e_hip")
    assert r["calls"]["wgrad"] == r["body_convs"] == (20 - 1 if name == "resnet18" else 53 - 1)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_one_block_vs_float64(name):
    frame.check_one_block(name, "torch_norm", "e_hip", OUT_FLOOR)


def test_switch_off_is_inert():
    """hip_train defaults to False, and with it off a train-mode, autograd-on call is the torch path bit for bit."""
    m = frame.new_model("resnet18").cuda()
    assert m.hip_train is False
    x = torch.randn(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(1)).cuda()
    # both sides of the torch.equal are the torch / MIOpen path: pin its algorithm choice (the first call of a shape
    # may pick another kernel than the later ones) so that the comparison is about the switch alone
    with frame.spy_train_trunk(forbid=True), torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                                                        deterministic=True):
        for _ in range(2):
            m.backbone(x)
        a = m(x)
        b = m.projection_head(m.backbone(x).flatten(1))
        assert a.requires_grad and torch.equal(a, b)
        assert torch.equal(m.extract_features(x), m.backbone(x).flatten(1))


def test_switch_on_applies_only_to_train_mode_with_autograd():
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
        assert entered[0][1] is False                     # hip_train alone: the walk keeps torch's BatchNorm2d


def test_switch_on_half_input_raises_from_torch_not_from_the_engine():
    m = frame.switch_on(frame.new_model("resnet18").cuda(), SWITCHES)
    with frame.spy_train_trunk(forbid=True):
        with pytest.raises(RuntimeError):
            m.extract_features(torch.zeros(2, 3, 32, 32, dtype=torch.float16, device="cuda"))
        tiny = m.extract_features(torch.zeros(2, 3, 6, 6, device="cuda"))      # H, W < 7: the torch path
        assert tuple(tiny.shape) == (2, 512)


def test_vit_ignores_the_switch():
    from hcir.main_backbone import SHAM2
    torch.manual_seed(3)
    m = SHAM2("vit_b_16").cuda().train()
    m.hip_train = True
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(3)).cuda()
    with frame.spy_train_trunk(forbid=True):
        f = m.extract_features(x)
    assert tuple(f.shape) == (4, 768) and f.requires_grad


def test_unexpected_trunk_is_an_error_not_another_result():
    from hcir import HcirError
    m = frame.switch_on(frame.new_model("resnet18").cuda(), SWITCHES)
    m.backbone[5][0].conv1.dilation = (2, 2)
    with pytest.raises(HcirError):
        m.extract_features(torch.zeros(2, 3, 32, 32, device="cuda"))


def test_one_train_step_resnet18():
    frame.check_one_train_step(SWITCHES)
