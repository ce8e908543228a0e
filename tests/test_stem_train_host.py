"""Host side of the train-mode stem (csrc/stem_train.hip, csrc/stem_plan.h, the `hip_train_stem` switch): statuses from
the shape alone, the weight gradient's parts and workspace, the statistics entry point's shape rules, and the selection
rule of the pool backward pinned against float64 torch autograd on the CPU.  No GPU: every call here returns before a
kernel is launched."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stem_ref as ref  # noqa: E402

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope="module")
def L(hcir_built):
    assert hcir_built.hcir_status_string(INVALID) and hcir_built.hcir_status_string(UNSUPPORTED)
    return hcir_built


def _calls(L, b, h, w):
    """Every stem entry point at image size (b, h, w) with NULL pointers; the two that take the conv map's size get
    the conv map of that image."""
    hc, wc = (h - 1) // 2 + 1 if h >= 1 else h, (w - 1) // 2 + 1 if w >= 1 else w
    N = None
    return {"conv": L.hcir_stem_conv_f16(N, b, h, w, N, N, N),
            "pool": L.hcir_stem_bn_relu_pool_f16(N, b, hc, wc, N, N, N, N, N, N),
            "pool_bwd": L.hcir_stem_pool_relu_bwd_f16(N, N, b, hc, wc, N, N, N, N, N, N),
            "wgrad": L.hcir_stem_wgrad_f16(N, N, b, h, w, N, N, 0, N)}


def test_status_names(L):
    assert L.hcir_status_string(UNSUPPORTED).decode().lower().find("unsupported") >= 0
    assert L.hcir_status_string(WORKSPACE).decode().lower().find("workspace") >= 0


@pytest.mark.parametrize("b,h,w,want", [(2, 6, 32, UNSUPPORTED), (2, 32, 6, UNSUPPORTED), (2, 6, 6, UNSUPPORTED),
                                        (0, 32, 32, INVALID), (-1, 6, 6, INVALID), (2, 0, 32, INVALID),
                                        (2, 7, 7, INVALID), (4, 224, 224, INVALID)])
def test_statuses_come_from_the_shape_alone(L, b, h, w, want):
    """Every pointer is NULL: a shape without a kernel is reported as such before a pointer is looked at, and only a
    shape WITH a kernel gets as far as the NULL pointers (INVALID)."""
    for name, st in _calls(L, b, h, w).items():
        assert st == want, f"{name} at {(b, h, w)}: status {st}"
    parts, wsb = L.hcir_stem_wgrad_parts(b, h, w), L.hcir_stem_wgrad_workspace_bytes(b, h, w)
    if b >= 1 and h >= 7 and w >= 7:
        assert parts >= 1
    else:
        assert parts == want and wsb == 0


def _tiles(b, h, w):
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return b * ((hc + 15) // 16) * ((wc + 15) // 16)


@pytest.mark.parametrize("b,h,w", [(1, 7, 7), (2, 30, 23), (3, 33, 47), (4, 64, 64), (5, 7, 7), (8, 96, 96),
                                   (64, 224, 224), (256, 224, 224)])
def test_wgrad_parts_and_workspace_agree(L, b, h, w):
    parts, wsb, tiles = L.hcir_stem_wgrad_parts(b, h, w), L.hcir_stem_wgrad_workspace_bytes(b, h, w), _tiles(b, h, w)
    per = max(4, -(-tiles // 512))                       # stem_plan.h: at least 4 conv tiles a part, at most 512 parts
    assert parts == -(-tiles // per) and 1 <= parts <= 512
    assert wsb == (parts * 64 * 147 * 4 if parts > 1 else 0)
    # the workspace is what the entry point asks for: one byte less is refused, before any pointer is followed
    if parts > 1:
        dummy = ctypes.create_string_buffer(16)
        p = ctypes.addressof(dummy)
        assert L.hcir_stem_wgrad_f16(p, p, b, h, w, p, p, wsb - 1, None) == WORKSPACE
        assert L.hcir_stem_wgrad_f16(p, p, b, h, w, p, None, wsb, None) == WORKSPACE


def test_wgrad_parts_one_and_several(L):
    assert L.hcir_stem_wgrad_parts(1, 7, 7) == 1 and L.hcir_stem_wgrad_workspace_bytes(1, 7, 7) == 0
    assert L.hcir_stem_wgrad_parts(2, 30, 23) == 1        # 2 conv tiles: still one part
    assert L.hcir_stem_wgrad_parts(4, 64, 64) == 4        # 16 conv tiles, 4 a part
    assert L.hcir_stem_wgrad_parts(5, 7, 7) == 2          # 5 conv tiles: 4 + 1, the smallest ragged last part
    assert L.hcir_stem_wgrad_parts(256, 224, 224) == 502  # 12544 conv tiles, 25 a part


@pytest.mark.parametrize("m,c", [(0, 64), (1, 64), (2, 64), (16, 64), (100, 32), (100, 96), (100, 128), (7, 0),
                                 (1 << 31, 64), (50176, 64), (100, 1 << 17), (3, 192)])
def test_stats_rejects_exactly_what_the_forward_rejects(L, m, c):
    dummy = ctypes.create_string_buffer(16)
    p = ctypes.addressof(dummy)
    N = None
    fwd_null = L.hcir_bn2d_fwd_nhwc_f16(N, m, c, N, N, 1e-5, 0.1, N, 0, N, N, N, N, N, N, 0, N)
    st_null = L.hcir_bn2d_stats_nhwc_f16(N, m, c, 1e-5, 0.1, N, N, N, N, N, 0, N)
    assert st_null == fwd_null
    # with every pointer given but no workspace, a shape with a kernel stops at the workspace check, in both
    fwd_ws = L.hcir_bn2d_fwd_nhwc_f16(p, m, c, p, p, 1e-5, 0.1, N, 0, N, N, p, p, p, N, 0, N)
    st_ws = L.hcir_bn2d_stats_nhwc_f16(p, m, c, 1e-5, 0.1, N, N, p, p, N, 0, N)
    assert st_ws == fwd_ws
    need = L.hcir_bn2d_workspace_bytes(m, c)
    assert (st_ws == WORKSPACE) == (need > 0) == (L.hcir_bn2d_chunks(m, c) > 0)
    if need:
        assert L.hcir_bn2d_stats_nhwc_f16(p, m, c, 1e-5, 0.1, N, N, p, p, p, need - 1, N) == WORKSPACE


def test_switch_defaults_and_state_dict(hcir_built):
    from hcir.backbone import SimCLR
    from hcir.main_backbone import SHAM2
    m = SHAM2("resnet18")
    assert m.hip_train_stem is False and SimCLR("resnet18").hip_train_stem is False
    keys = set(m.state_dict())
    m.hip_train_stem = True
    assert set(m.state_dict()) == keys and not any("hip_train" in k for k in keys)
    # a CPU tensor: no switch applies, the torch path runs
    m.hip_train = True
    m.train()
    f = m.extract_features(torch.randn(2, 3, 32, 32))
    assert f.requires_grad and tuple(f.shape) == (2, 512)


def test_stem_weight_cache_follows_the_parameter(hcir_built):
    from hcir import conv_train
    from hcir.resnet_engine import pack_stem_weight
    w = torch.nn.Parameter(torch.randn(64, 3, 7, 7, generator=torch.Generator().manual_seed(0)))
    (p0,) = conv_train.stem_weights.get(w)
    assert torch.equal(p0, pack_stem_weight(w)) and conv_train.stem_weights.get(w)[0] is p0
    with torch.no_grad():
        w.mul_(2.0)
    (p1,) = conv_train.stem_weights.get(w)
    assert p1 is not p0 and torch.equal(p1, pack_stem_weight(w))


def test_selection_rule_is_torchs_on_a_map_full_of_ties():
    """The rule hcir_stem_pool_relu_bwd_f16 implements (first extreme of c by the sign of rstd * gamma, mask by
    y > 0), restated in Python, against F.max_pool2d(F.relu(.)) autograd in float64: (2, 64, 15, 12), the windows
    hang over both far edges, c in multiples of 0.25 so that about a third of the windows tie, channels of
    positive, negative and zero gamma.  Exactly equal."""
    i = ref.pool_inputs(2, 15, 12, seed=3)
    s = i["rstd"] * i["gamma"]
    assert (s > 0).any() and (s < 0).any() and (s == 0).sum() == 3
    tied = ref.tied_fraction(i)
    print(f"tied windows {tied:.3f}, min |y| at a selected position {ref.min_selected_abs_y(i):.4f}")
    assert tied > 0.2
    assert ref.min_selected_abs_y(i) >= 1e-4
    g_auto, g_rule = ref.g64_autograd(i), ref.g_rule(i)
    assert (g_auto != 0).any()
    assert torch.equal(g_auto, g_rule), f"max difference {(g_auto - g_rule).abs().max().item()}"
