"""Host side of the convolution backward (csrc/conv_bwd.hip, hcir/conv_train.py): ABI, shape statuses decided before
any pointer is looked at, the split plan and its workspace, argument checks, the cached weight layouts.  No GPU."""
import ctypes

import pytest
import torch

NEW = ("hcir_conv2d_wgrad_f16", "hcir_conv2d_wgrad_workspace_bytes", "hcir_conv2d_wgrad_splits",
       "hcir_spread2_nhwc_f16")
HCIR_ERR_INVALID, HCIR_ERR_UNSUPPORTED, HCIR_ERR_WORKSPACE = -1, -2, -4


def test_new_symbols_declared_and_exported(hcir_built):
    from hcir import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(hcir_built, name)
    assert hcir_built.hcir_status_string(HCIR_ERR_INVALID) != hcir_built.hcir_status_string(HCIR_ERR_UNSUPPORTED)


@pytest.mark.parametrize("shape,status", [
    # b, h, w, cin, cout, r, s, stride, pad
    ((2, 8, 8, 3, 64, 3, 3, 1, 1), HCIR_ERR_UNSUPPORTED),      # Cin = 3
    ((2, 8, 8, 64, 64, 7, 7, 2, 3), HCIR_ERR_UNSUPPORTED),     # 7 x 7
    ((2, 8, 8, 64, 64, 3, 3, 1, 0), HCIR_ERR_UNSUPPORTED),     # 3 x 3 without its pad
    ((2, 8, 8, 64, 64, 1, 1, 1, 1), HCIR_ERR_UNSUPPORTED),     # 1 x 1 with a pad
    ((2, 8, 8, 64, 64, 3, 3, 3, 1), HCIR_ERR_UNSUPPORTED),     # stride 3
    ((0, 8, 8, 64, 64, 3, 3, 1, 1), HCIR_ERR_INVALID),         # B = 0
])
def test_wgrad_statuses_from_the_shape_alone(hcir_built, shape, status):
    b, h, w, cin, cout, r, s, stride, pad = shape
    got = hcir_built.hcir_conv2d_wgrad_f16(None, None, b, h, w, cin, cout, r, s, stride, pad, None, None, 0, None)
    assert got == status
    assert hcir_built.hcir_conv2d_wgrad_splits(*shape) == status
    assert hcir_built.hcir_conv2d_wgrad_workspace_bytes(*shape) == 0


def test_wgrad_null_pointers_on_a_supported_shape(hcir_built):
    assert hcir_built.hcir_conv2d_wgrad_f16(None, None, 2, 7, 7, 64, 64, 3, 3, 1, 1, None, None, 0, None) \
        == HCIR_ERR_INVALID


@pytest.mark.parametrize("shape", [
    (2, 7, 7, 64, 64, 3, 3, 1, 1), (4, 28, 28, 64, 64, 3, 3, 1, 1), (1, 1, 1, 512, 512, 3, 3, 1, 1),
    (2, 7, 7, 512, 2048, 1, 1, 1, 0), (2, 23, 23, 256, 256, 3, 3, 1, 1), (256, 56, 56, 64, 64, 3, 3, 1, 1),
    (64, 14, 14, 1024, 256, 1, 1, 1, 0), (2, 14, 14, 256, 512, 1, 1, 2, 0),
])
def test_wgrad_workspace_consistent_with_splits(hcir_built, shape):
    b, h, w, cin, cout, r, s, stride, pad = shape
    splits = hcir_built.hcir_conv2d_wgrad_splits(*shape)
    ws = hcir_built.hcir_conv2d_wgrad_workspace_bytes(*shape)
    assert splits >= 1
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    assert splits <= (b * ho * wo + 63) // 64                       # never less than one 64-pixel step per split
    assert ws == (0 if splits == 1 else splits * cout * r * s * cin * 4)
    if splits > 1:      # a shape short of its workspace is refused before the launch
        buf = ctypes.c_void_p(16)
        assert hcir_built.hcir_conv2d_wgrad_f16(buf, buf, b, h, w, cin, cout, r, s, stride, pad, buf, buf, ws - 1,
                                                None) == HCIR_ERR_WORKSPACE


def test_wgrad_split_plan_fills_the_chip_on_the_smallest_layer(hcir_built):
    # layer1's 3x3 (64 x 576 output = 9 tiles) at a training batch: at least two workgroups per CU (256 CUs)
    assert 9 * hcir_built.hcir_conv2d_wgrad_splits(256, 56, 56, 64, 64, 3, 3, 1, 1) >= 512
    assert hcir_built.hcir_conv2d_wgrad_splits(1, 1, 1, 512, 512, 3, 3, 1, 1) == 1


def test_spread2_statuses(hcir_built):
    f = hcir_built.hcir_spread2_nhwc_f16
    assert f(None, 1, 8, 7, 64, 14, 13, None, None) == HCIR_ERR_INVALID      # 2 * 7 > 14 - 1 along h
    assert f(None, 1, 7, 8, 64, 13, 14, None, None) == HCIR_ERR_INVALID      # 2 * 7 > 13 along w
    assert f(None, 0, 7, 7, 64, 14, 14, None, None) == HCIR_ERR_INVALID
    assert f(None, 1, 7, 7, 60, 14, 14, None, None) == HCIR_ERR_UNSUPPORTED
    assert f(None, 1, 7, 7, 64, 14, 14, None, None) == HCIR_ERR_INVALID      # shape fine, null pointers


def test_ops_raise_on_cpu_tensors_and_bad_shapes(hcir_built):
    from hcir import HcirError, ops
    x = torch.zeros(2, 7, 7, 64, dtype=torch.float16)
    dy = torch.zeros(2, 7, 7, 64, dtype=torch.float16)
    with pytest.raises(HcirError, match="no CPU fallback"):
        ops.conv2d_wgrad(x, dy, 3, 1, 1)
    with pytest.raises(HcirError, match="no CPU fallback"):
        ops.spread2_nhwc(x, 14, 14)
    with pytest.raises(HcirError):
        ops.conv2d_wgrad_splits(2, 7, 7, 3, 64, 3, 1, 1)
    assert ops.conv2d_wgrad_splits(2, 7, 7, 64, 64, 3, 1, 1) == 2


def test_weight_cache_layouts_and_refresh(hcir_built):
    """The packed weight is pack_conv_weight(w), the data-gradient weight is the packed flip + transpose; both follow
    the parameter's version."""
    from hcir import conv_train
    from hcir.resnet_engine import pack_conv_weight
    w = torch.nn.Parameter(torch.randn(128, 64, 3, 3, generator=torch.Generator().manual_seed(0)))
    cache = conv_train._WeightCache()
    w16, wt16 = cache.get(w)
    assert w16.dtype == torch.float16 and tuple(w16.shape) == (128, 3, 3, 64) and tuple(wt16.shape) == (64, 3, 3, 128)
    assert torch.equal(w16, pack_conv_weight(w))
    assert torch.equal(wt16, pack_conv_weight(w.detach().flip(2, 3).permute(1, 0, 2, 3)))
    # element-wise statement of the same: wT[c][r'][s'][n] = w[n][R-1-r'][S-1-s'][c]
    assert wt16[5, 0, 2, 7] == w.detach()[7, 5, 2, 0].half()
    again = cache.get(w)
    assert again[0] is w16 and again[1] is wt16                 # unchanged version: no repack
    with torch.no_grad():
        w.mul_(2.0)                                             # what an optimizer step does: bumps _version
    w16b, wt16b = cache.get(w)
    assert w16b is not w16 and torch.equal(w16b, pack_conv_weight(w))
    assert torch.equal(wt16b, pack_conv_weight(w.detach().flip(2, 3).permute(1, 0, 2, 3))) and not torch.equal(wt16b, wt16)


def test_hip_train_switch_defaults_and_gate(hcir_built):
    from hcir.backbone import SimCLR
    from hcir.conv_train import hip_train_active
    from hcir.main_backbone import SHAM2
    m = SHAM2("resnet18")
    assert m.hip_train is False and SimCLR("resnet18").hip_train is False
    x = torch.randn(2, 3, 32, 32)
    m.hip_train = True
    m.train()
    assert not hip_train_active(True, m.backbone, x)            # CPU tensor: the torch path
    a = m.extract_features(x)                                   # ... and it runs, differentiable, on torch
    assert a.requires_grad and tuple(a.shape) == (2, 512)
