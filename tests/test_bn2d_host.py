"""Host side of the batch-statistics BatchNorm2d kernels (csrc/bn2d.hip, csrc/bn2d_plan.h, hcir/conv_train.py): the
row-chunk plan and its workspace, statuses decided from the shape alone before a pointer is looked at, the wrappers'
argument checks and the `hip_train_norm` switch's default.  No GPU."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hcir_bn2d_fwd_nhwc_f16", "hcir_bn2d_bwd_nhwc_f16", "hcir_bn2d_workspace_bytes", "hcir_bn2d_chunks")
HCIR_ERR_INVALID, HCIR_ERR_UNSUPPORTED, HCIR_ERR_WORKSPACE = -1, -2, -4
FIELDS = ["cv", "wv_log2", "slabs", "rpp", "chunks", "rows_per_chunk", "apply_blocks", "bytes"]
MS = [2, 3, 75, 196, 2352, 25088, 802816]
CS = [64, 256, 2048]


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libbn2d_plan_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "bn2d_plan_emul.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.emul_bn2d_plan.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    L.emul_bn2d_chunk_rows.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                       ctypes.c_void_p]
    return L


def _plan(emul, m, c):
    out = (ctypes.c_int64 * len(FIELDS))()
    assert emul.emul_bn2d_plan(m, c, out) == 0
    return dict(zip(FIELDS, out))


def _fwd(L, x, m, c, ws=None, wsb=0):
    p = ctypes.c_void_p(16)      # never read: every call below is refused before a launch
    return L.hcir_bn2d_fwd_nhwc_f16(x, m, c, p, p, 1e-5, 0.1, None, 0, None, None, p, p, p, ws, wsb, None)


def _bwd(L, dy, m, c, ws=None, wsb=0):
    p = ctypes.c_void_p(16)
    return L.hcir_bn2d_bwd_nhwc_f16(dy, p, None, m, c, p, p, p, p, None, p, p, ws, wsb, None)


def test_new_symbols_declared_and_exported(hcir_built):
    from hcir import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(hcir_built, name)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("m", MS)
def test_plan_chunks_cover_the_rows_once(hcir_built, emul, m, c):
    p = _plan(emul, m, c)
    assert p["chunks"] >= 1 and p["chunks"] == hcir_built.hcir_bn2d_chunks(m, c)
    # the documented workspace: chunks * C * 2 floats, the same number from the ABI and from the plan header
    assert p["bytes"] == p["chunks"] * c * 2 * 4 == hcir_built.hcir_bn2d_workspace_bytes(m, c)
    # lanes over the map: C / 8 vectors per row, 2^wv_log2 of them per wavefront, four wavefronts' rows per pass
    wv = 1 << p["wv_log2"]
    assert p["cv"] == c // 8 and p["cv"] % wv == 0 and p["slabs"] == p["cv"] // wv and p["rpp"] == 4 * 64 // wv
    assert wv == min(64, p["cv"])                         # C = 64: 8 whole rows per wavefront; C >= 512: 512 channels
    # the grid stays at the cap of about 8 workgroups per CU, and small maps are not cut below a few passes per chunk
    cap = emul.emul_bn2d_grid_cap()
    assert cap == 2048 and p["chunks"] * p["slabs"] <= cap and 1 <= p["apply_blocks"] * p["slabs"] <= cap
    assert p["rows_per_chunk"] % p["rpp"] == 0
    # the ranges tile [0, M): contiguous, in order, all full but possibly the last
    r0, r1 = ctypes.c_int64(), ctypes.c_int64()
    at = 0
    for k in range(p["chunks"]):
        emul.emul_bn2d_chunk_rows(m, c, k, ctypes.byref(r0), ctypes.byref(r1))
        assert r0.value == at and r1.value > r0.value
        if k < p["chunks"] - 1:
            assert r1.value - r0.value == p["rows_per_chunk"]
        else:
            assert r1.value - r0.value <= p["rows_per_chunk"]
        at = r1.value
    assert at == m


def test_plan_fills_the_chip_at_a_training_shape(hcir_built):
    # ResNet-50 layer1 at batch 256: at least four workgroups per CU (256 CUs) in the reductions; the smallest map: one
    assert hcir_built.hcir_bn2d_chunks(256 * 56 * 56, 256) >= 1024
    assert hcir_built.hcir_bn2d_chunks(256 * 56 * 56, 64) >= 1024
    assert hcir_built.hcir_bn2d_chunks(2, 64) == 1


@pytest.mark.parametrize("m,c,status", [
    (196, 96, HCIR_ERR_UNSUPPORTED),        # C % 64 != 0
    (196, 32, HCIR_ERR_UNSUPPORTED),        # C < 64
    (196, 0, HCIR_ERR_INVALID),
    (1, 64, HCIR_ERR_INVALID),              # one value per channel: torch refuses it in training too
    (0, 64, HCIR_ERR_INVALID),
])
def test_statuses_from_the_shape_alone(hcir_built, m, c, status):
    assert _fwd(hcir_built, None, m, c) == status
    assert _bwd(hcir_built, None, m, c) == status
    assert hcir_built.hcir_bn2d_chunks(m, c) == status
    assert hcir_built.hcir_bn2d_workspace_bytes(m, c) == 0


def test_null_pointers_and_short_workspace_on_a_supported_shape(hcir_built):
    L = hcir_built
    buf = ctypes.c_void_p(16)
    need = L.hcir_bn2d_workspace_bytes(196, 256)
    assert need > 0
    assert _fwd(L, None, 196, 256, buf, need) == HCIR_ERR_INVALID           # NULL x
    assert _bwd(L, None, 196, 256, buf, need) == HCIR_ERR_INVALID           # NULL dy
    assert _fwd(L, buf, 196, 256, buf, need - 1) == HCIR_ERR_WORKSPACE
    assert _bwd(L, buf, 196, 256, buf, need - 1) == HCIR_ERR_WORKSPACE
    assert _fwd(L, buf, 196, 256, None, need) == HCIR_ERR_WORKSPACE


def test_ops_raise_on_cpu_tensors_and_bad_arguments(hcir_built):
    from hcir import HcirError, ops
    x = torch.zeros(2, 7, 7, 64, dtype=torch.float16)
    v = torch.ones(64)
    with pytest.raises(HcirError, match="no CPU fallback"):
        ops.bn2d_fwd(x, v, v, 1e-5, 0.1)
    with pytest.raises(HcirError, match="no CPU fallback"):
        ops.bn2d_bwd(x, x, None, v, v, v)
    with pytest.raises(HcirError):
        ops.bn2d_chunks(196, 96)
    assert ops.bn2d_chunks(2, 64) == 1


def test_hip_train_norm_defaults_to_off(hcir_built):
    from hcir.backbone import SimCLR
    from hcir.main_backbone import SHAM2
    m = SHAM2("resnet18")
    assert m.hip_train_norm is False and m.hip_train is False
    s = SimCLR("resnet18")
    assert s.hip_train_norm is False and s.hip_train is False
    # on a CPU tensor neither switch applies: the torch path runs, differentiable
    m.hip_train = m.hip_train_norm = True
    a = m.train().extract_features(torch.randn(2, 3, 32, 32))
    assert a.requires_grad and tuple(a.shape) == (2, 512)


@pytest.mark.parametrize("kwargs", [dict(momentum=None), dict(affine=False), dict(track_running_stats=False)])
def test_bn_act_refuses_modules_without_a_kernel(hcir_built, kwargs):
    from hcir import HcirError
    from hcir.conv_train import bn_act_nhwc
    x = torch.zeros(2, 7, 7, 64, dtype=torch.float16)
    with pytest.raises(HcirError, match="bn_act_nhwc needs"):
        bn_act_nhwc(x, torch.nn.BatchNorm2d(64, **kwargs).train())
    with pytest.raises(HcirError, match="bn_act_nhwc needs"):
        bn_act_nhwc(x, torch.nn.BatchNorm2d(64).eval())
