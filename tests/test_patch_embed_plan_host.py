"""CPU tests of the hcir_patch_embed_fused host plan: csrc/patch_plan.h compiled for the host
(tests/patch_plan_emul.cpp).  The route decision at the shapes of tests/test_patch_embed_fused_gpu.py and on the far
side of every condition of the route, the tile counts, and the patch-row -> token-row remap against a Python loop.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16 = 0, 1
TILE128, BIG = 0, 1
FIELDS = ("route", "np", "t", "rows", "tn", "tm", "grid")


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libpatch_plan_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "patch_plan_emul.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.emul_patch_embed_plan.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_int32, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    L.emul_patch_token_row.argtypes = [ctypes.c_int64, ctypes.c_int32]
    L.emul_patch_token_row.restype = ctypes.c_int64
    return L


def plan(L, b, c, h, w, p, d, ldw, dt):
    out = np.zeros(len(FIELDS), np.int64)
    L.emul_patch_embed_plan(b, c, h, w, p, d, ldw, dt, out.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in out)))


# (b, c, h, w, p, d, ldw, dtype) -> (route, np, rows, tn, tm, grid)
CASES = [
    ((1, 3, 224, 224, 16, 768, 768, F16), (BIG, 196, 196, 3, 1, 3)),         # one ragged m-tile
    ((3, 3, 224, 224, 16, 768, 768, F16), (BIG, 196, 588, 3, 3, 9)),
    ((4, 3, 224, 224, 16, 768, 768, F16), (BIG, 196, 784, 3, 4, 12)),        # the last tile holds 16 rows
    ((50, 3, 32, 48, 16, 768, 768, F16), (BIG, 6, 300, 3, 2, 6)),            # 43 images per tile
    ((2, 3, 224, 224, 16, 1024, 768, F16), (BIG, 196, 392, 4, 2, 8)),
    ((880, 3, 224, 224, 16, 768, 768, F16), (BIG, 196, 172480, 3, 674, 256)),  # the benchmark: persistent, 7.9 rounds
    # the old route: P = 14, d = 384 (no whole 256-feature tile), fp32 tokens, padded weight rows, a channel count
    # whose tile span leaves 32-bit offsets
    ((2, 3, 224, 224, 14, 1024, 640, F16), (TILE128, 256, 512, 0, 0, 0)),
    ((2, 3, 224, 224, 16, 384, 768, F16), (TILE128, 196, 392, 0, 0, 0)),
    ((3, 3, 224, 224, 16, 768, 768, F32), (TILE128, 196, 588, 0, 0, 0)),
    ((3, 3, 224, 224, 16, 768, 832, F16), (TILE128, 196, 588, 0, 0, 0)),
    ((3, 4000, 224, 224, 16, 768, 4000 * 256, F16), (TILE128, 196, 588, 0, 0, 0)),
    ((3, 3, 224, 224, 8, 768, 192, F16), (TILE128, 784, 2352, 0, 0, 0)),
]


@pytest.mark.parametrize("shape,want", CASES, ids=["-".join(map(str, s)) for s, _ in CASES])
def test_route_and_tiles(emul, shape, want):
    got = plan(emul, *shape)
    route, npatch, rows, tn, tm, grid = want
    assert got == dict(route=route, np=npatch, t=npatch + 1, rows=rows, tn=tn, tm=tm, grid=grid)
    if route == BIG:
        b, d = shape[0], shape[5]
        assert got["tn"] * 256 == d and (got["tm"] - 1) * 256 < rows <= got["tm"] * 256
        assert got["grid"] == min(256, tn * tm) and b * got["t"] < 2 ** 31


def test_token_rows_are_bounded_to_32_bits(emul):
    """b * T just below / above what the kernel indexes in 32 bits (one image of one patch: T = 2)."""
    assert plan(emul, (2 ** 31 - 1 - 256) // 2, 3, 16, 16, 16, 768, 768, F16)["route"] == BIG
    assert plan(emul, (2 ** 31 - 256) // 2 + 1, 3, 16, 16, 16, 768, 768, F16)["route"] == TILE128


@pytest.mark.parametrize("b,npatch", [(1, 196), (3, 196), (4, 196), (50, 6), (7, 1), (5, 257)])
def test_row_remap_against_a_loop(emul, b, npatch):
    """GEMM row m = bi * np + pi -> token row bi * T + 1 + pi: every patch row once, class rows (bi * T) never."""
    want, m = [], 0
    for bi in range(b):
        for pi in range(npatch):
            want.append(bi * (npatch + 1) + 1 + pi)
            assert emul.emul_patch_token_row(m, npatch) == want[-1]
            m += 1
    assert sorted(set(want)) == want and not set(want) & {bi * (npatch + 1) for bi in range(b)}
    assert want[-1] == b * (npatch + 1) - 1


def test_route_query_of_the_library_agrees(emul, hcir_built):
    """hcir_patch_embed_route (the built library; no GPU needed) returns the plan's route; bad sizes are invalid."""
    for shape, _ in CASES:
        assert hcir_built.hcir_patch_embed_route(*shape) == plan(emul, *shape)["route"]
    assert hcir_built.hcir_patch_embed_route(0, 3, 224, 224, 16, 768, 768, F16) == -1
    assert hcir_built.hcir_patch_embed_route(1, 3, 225, 224, 16, 768, 768, F16) == -1
