"""GPU: the persistent GEMM kernels after their per-tile address bookkeeping moved to scalars (gemm_stage_addr.h):
tile-invariant lane offsets on wave-uniform bases, a clamped general form on ragged tiles only, one tile origin per
tile handed from the issuer to the epilogue.

Every element of every output against oracle.gemm's float64 reference through its per-element bound (err / bound <= 1,
the helper of tests/test_gemm_gpu.py), sentinel rows and pad columns bit-unchanged, the route ASKED of the library and
asserted.  Shapes, smallest at which this can go wrong:
  * SMALL_M: one k-step per tile (the issuer moves on every step), one row in the last tile, 1279 / 1280 rows, n-tiles
    in groups of 3 and of 6, twelve k-steps.  At these sizes gemm_plan.h sends ONLY the dual-GELU form to the
    256 x 256 kernel (it stays there at every shape); the other epilogues take the 128 x 192 kernel, which runs the
    same issuer at its own geometry.  Both are asserted.
  * TALL: the same features with enough rows (>= 180 tiles) that EVERY epilogue is on the 256 x 256 kernel, one of
    them with two tiles per workgroup at one k-step per tile (the issuer two tiles ahead of the epilogue), the
    smallest M that N = 256 sends to the tail split, and hcir_gemm_f16_ln_rows with more tiles than workgroups (the
    only launch that gives the 128 x 192 kernel a second tile).
Fast path against general path in one build: the rows of an M-row launch that lie in its last, FULL tile equal, bit for
bit, the same rows of the (M - 1)-row launch on the same operands, where that tile is ragged and takes the clamped
form (tests/test_vit_ends_gpu.py compares launches the same way).  The float64 bound is the safety net.
"""
import os
import sys

import pytest
import torch

from oracle import gemm as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_gpu as older  # noqa: E402  (Out: sentinels; the per-element check is og.ratio, as there)

pytestmark = pytest.mark.gpu

KINDS = ("bias_f16", "stats", "ln_bias_f16", "ln_gelu_f16", "dual")
ROUTE_EPI = {"bias_f16": 0, "stats": 6, "ln_bias_f16": 0, "ln_gelu_f16": 1, "dual": og.ROUTE_EPI_DUAL}

# (m, n, k): the sizes the 256 x 256 kernel reaches with the dual form only
SMALL_M = [(1024, 256, 64), (1025, 256, 128), (1279, 512, 192), (1280, 512, 192), (1300, 1536, 64), (1300, 3072, 64),
           (1112, 768, 768)]
# (m, n, k) -> 256 x 256 tiles; every epilogue on the 256 x 256 kernel
TALL = [(46080, 256, 64),      # 180 tiles of one k-step
        (46081, 256, 128),     # 181, the last holds one row
        (98305, 256, 64),      # 385 of one k-step: two tiles per workgroup, the last holds one row
        (23039, 512, 192), (23040, 512, 192),
        (7700, 1536, 64),      # 6 x 31, n-tiles in groups of 3, 20 rows in the last row of tiles
        (3900, 3072, 64),      # 12 x 16, groups of 6, 60 rows
        (15400, 768, 768)]     # 3 x 61, twelve k-steps, 40 rows
PAIRS = {(1279, 512, 192): (1280, 512, 192), (23039, 512, 192): (23040, 512, 192), (1151, 512, 192): (1152, 512, 192)}


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    return hcir_built


@pytest.fixture(scope="module")
def problems():
    """(m, n, k) -> operands on the device with their float64 S and A, made once.  The short side of a PAIR is the
    first m rows of the long side's problem: the same operands in both launches."""
    cache = {}

    def get(shape):
        m, n, k = shape
        full = PAIRS.get(shape, shape)
        if full not in cache:
            p = {key: v.cuda() for key, v in og.make_problem("plain", *full).items()}
            p["acc"] = og.acc_f64(p["a"], p["w"])
            cache[full] = p
        p = dict(cache[full])
        if full != shape:
            for key in ("a", "resid", "stats"):
                p[key] = p[key][:m]
            p["acc"] = og.Acc(p["acc"].s[:m], p["acc"].a[:m], k)
        p["m"], p["n"], p["k"] = m, n, k
        return p
    return get


def route(L, shape, kind):
    rows = torch.full((1,), -1, dtype=torch.int64)
    r = L.hcir_gemm_route(*shape, ROUTE_EPI[kind], rows.data_ptr())
    return r, int(rows[0])


def launch(L, p, kind, pitch=False):
    """One launch -> ({name: err / bound over every element}, [output tensors]); sentinels checked."""
    m, n, k = p["m"], p["n"], p["k"]
    lda, ldw = (k + 8, k + 16) if pitch else (k, k)
    ldo = n + 8                                     # eight pad columns behind every output row
    a, w = (older.pitched(p["a"], lda), older.pitched(p["w"], ldw)) if pitch else (p["a"], p["w"])
    st = torch.cuda.current_stream().cuda_stream
    bias = p["bias"].data_ptr()
    if kind == "dual":
        out, out2 = older.Out(m, n, ldo, torch.float16), older.Out(m, n, ldo, torch.float16)
        assert L.hcir_gemm_f16_gelu_dual(a.data_ptr(), lda, w.data_ptr(), ldw, bias, m, n, k, out.ptr(), out2.ptr(), ldo,
                                         st) == 0
        refs = og.epilogue_f64("dual", p["acc"], bias=p["bias"])
        return ({"pre": og.ratio(out.check(), *refs[0]), "act": og.ratio(out2.check(), *refs[1])},
                [out.t.clone(), out2.t.clone()])
    if kind in ("ln_bias_f16", "ln_gelu_f16"):
        out = older.Out(m, n, ldo, torch.float16)
        assert L.hcir_gemm_f16_fused(a.data_ptr(), lda, w.data_ptr(), ldw, bias, None, m, n, k, ROUTE_EPI[kind],
                                     out.ptr(), ldo, p["stats"].data_ptr(), p["c1"].data_ptr(), None, st) == 0
        (ref, bound), = og.epilogue_f64(kind, p["acc"], bias=p["bias"], stats=p["stats"], c1=p["c1"])
        return {"out": og.ratio(out.check(), ref, bound)}, [out.t.clone()]
    if kind == "stats":
        resid = p["resid"].half()
        nsl = L.hcir_gemm_stats_slices(n)
        out = older.Out(m, n, ldo, torch.float16, resid)
        part = older.Out(nsl * m, 2, 2, torch.float32)
        assert L.hcir_gemm_f16_fused(a.data_ptr(), lda, w.data_ptr(), ldw, bias, None, m, n, k, 6, out.ptr(), ldo, None,
                                     None, part.ptr(), st) == 0
        (ref, bound), = og.epilogue_f64("resid_f16", p["acc"], bias=p["bias"], scale=None, resid=resid)
        rows = out.check()
        sl = part.check().view(nsl, m, 2)
        mean_p, m2_p, d_mean_p, d_m2_p = og.slice_stats_f64(rows)   # of the fp16 rows the kernel stored
        return ({"out": og.ratio(rows, ref, bound), "slice_mean": og.ratio(sl[..., 0], mean_p, d_mean_p),
                 "slice_m2": og.ratio(sl[..., 1], m2_p, d_m2_p)}, [rows.clone(), sl.clone()])
    assert kind == "bias_f16"
    out = older.Out(m, n, ldo, torch.float16)
    assert L.hcir_gemm_f16(a.data_ptr(), lda, w.data_ptr(), ldw, bias, None, m, n, k, 0, out.ptr(), ldo, st) == 0
    (ref, bound), = og.epilogue_f64(kind, p["acc"], bias=p["bias"])
    return {"out": og.ratio(out.check(), ref, bound)}, [out.t.clone()]


def check(L, problems, shape, kind, want_route, pitch=False):
    r, m1 = route(L, shape, kind)
    assert r == want_route, (shape, kind, r)
    ratios, outs = launch(L, problems(shape), kind, pitch)
    print(f"\ngemm-tile {shape} {kind}{' pitched' if pitch else ''} route {r}: " +
          " ".join(f"{key} {v:.3f}" for key, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (shape, kind, ratios)
    return outs, m1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SMALL_M, ids=str)
def test_small_m_shapes(L, problems, shape, kind):
    """The dual form on the 256 x 256 kernel, the others on the 128 x 192 kernel (fewer than 180 tiles of 256 x 256)."""
    m, n, _ = shape
    assert -(-m // 256) * (n // 256) < 180
    check(L, problems, shape, kind, og.ROUTE_BIG if kind == "dual" else og.ROUTE_MID)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", TALL, ids=str)
def test_every_epilogue_on_the_256_kernel(L, problems, shape, kind):
    _, m1 = check(L, problems, shape, kind, og.ROUTE_BIG)
    assert m1 == shape[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1279, 512, 192), (7700, 1536, 64)], ids=str)
def test_pitched_rows(L, problems, shape, kind):
    """lda = k + 8, ldw = k + 16: a ragged last tile on both kernels, the n-grouped walk on the 256 x 256 kernel."""
    tall = shape[0] > 2000
    check(L, problems, shape, kind, og.ROUTE_BIG if (tall or kind == "dual") else og.ROUTE_MID, pitch=True)


# (short shape, tile rows, kind): 1279 / 1280 reach the 256 x 256 kernel with the dual form only, 23039 / 23040 with
# every form; 1151 / 1152 (six whole tiles of 192 rows) are on the 128 x 192 kernel with every form but the dual
BIT_CASES = ([((1279, 512, 192), 256, "dual")] + [((23039, 512, 192), 256, kind) for kind in KINDS] +
             [((1151, 512, 192), 192, kind) for kind in KINDS if kind != "dual"])


@pytest.mark.parametrize("short,tile,kind", BIT_CASES, ids=str)
def test_full_tile_equals_the_same_tile_ragged(L, problems, short, tile, kind):
    """The last tile of M rows is full (lane offsets on scalar bases); with M - 1 rows it is ragged (clamped offsets
    at issue time).  Its first tile - 1 rows must come out bit-equal, statistics slices included."""
    full = PAIRS[short]
    m = full[0]
    assert m % tile == 0
    want = og.ROUTE_MID if tile == 192 else og.ROUTE_BIG
    outs_full, _ = check(L, problems, full, kind, want)
    outs_short, _ = check(L, problems, short, kind, want)
    for x, y in zip(outs_full, outs_short):
        if x.dim() == 3:      # statistics slices [n / 64, m, 2]
            x, y = x[:, m - tile:m - 1], y[:, m - tile:m - 1]
            as_int = torch.int32
        else:
            x, y = x[m - tile:m - 1], y[m - tile:m - 1]
            as_int = torch.int16
        assert x.shape == y.shape and x.numel() > 0
        assert torch.equal(x.contiguous().view(as_int), y.contiguous().view(as_int)), (short, kind)


def test_smallest_split_and_smallest_mid_at_n_256(L, problems):
    """N = 256, K = 64: the first M on the 128 x 192 kernel is 1024 (below it: the 128 x 128 kernel) and the first M
    on the tail split is 65537 (256 whole tiles, one row behind them), found by asking the route."""
    assert route(L, (1023, 256, 64), "bias_f16")[0] == og.ROUTE_SMALL
    assert route(L, (1024, 256, 64), "bias_f16")[0] == og.ROUTE_MID
    first = next(m for m in range(179 * 256 + 1, 70000) if route(L, (m, 256, 64), "bias_f16")[0] == og.ROUTE_SPLIT)
    assert first == 65537 and route(L, (first, 256, 64), "bias_f16") == (og.ROUTE_SPLIT, 65536)
    for kind in ("bias_f16", "stats", "ln_bias_f16", "ln_gelu_f16"):
        check(L, problems, (first, 256, 64), kind, og.ROUTE_SPLIT)
    check(L, problems, (first, 256, 64), "dual", og.ROUTE_BIG)
    # (1024, 256, 64) on the 128 x 192 kernel: test_small_m_shapes


@pytest.mark.parametrize("k", [64, 192])
def test_ln_rows_with_more_tiles_than_workgroups(L, problems, k):
    """hcir_gemm_f16_ln_rows launches the 128 x 192 kernel whatever the size: 2 x 301 tiles on 512 workgroups, the
    last row of tiles ragged (23 rows) - the 128 x 192 kernel's only way to a second tile per workgroup."""
    m, n = 300 * 192 + 23, 256
    p = problems((m, n, k))
    ldo = n + 8
    out = older.Out(m, n, ldo, torch.float16)
    assert L.hcir_gemm_f16_ln_rows(p["a"].data_ptr(), k, p["w"].data_ptr(), k, p["bias"].data_ptr(), m, n, k, out.ptr(),
                                   ldo, p["stats"].data_ptr(), p["c1"].data_ptr(),
                                   torch.cuda.current_stream().cuda_stream) == 0
    (ref, bound), = og.epilogue_f64("ln_bias_f16", p["acc"], bias=p["bias"], stats=p["stats"], c1=p["c1"])
    r = og.ratio(out.check(), ref, bound)
    print(f"\ngemm-tile ln_rows ({m}, {n}, {k}): out {r:.3f}")
    assert r <= 1.0
