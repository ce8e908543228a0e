"""Host side of the batch-statistics BatchNorm2d kernels (csrc/bn2d.hip, csrc/bn2d_plan.h, hcir/conv_train.py): the
row-chunk plan and its workspace, statuses decided from the shape alone before a pointer is looked at, the wrappers'
argument checks and the `hip_train_norm` switch's default.  No GPU.

The second half is about oracle.bn2d, which tests/test_bn2d_elements_gpu.py holds the kernels to: its plan equals the
compiled header field for field; the suite's older shapes all take the small-map branch (at most 4 passes per chunk,
one apply trip, one chunk per finalize lane), no training batch does, the CAPPED and STRIDED shapes do not; the bounds
are honest (the fp32 emulation of the reduction order stays within a quarter of the statistics bounds and within the
sum bounds on every family and shape) and sharp (each listed kernel mistake, applied to the float64 chain and put
through the checks of the GPU tests, exceeds a bound 10-fold, or breaks the exact-sum / hot-row checks).  Both tables
are printed (pytest -s; profiles/bn2d_bounds.txt keeps a copy).  No listed mistake stays below the 10 x bar
(BELOW_BAR is empty; the mechanism of tests/test_rowops_host.py is kept)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from oracle import bn2d as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_bn2d_gpu as older  # noqa: E402  (the shape lists the older GPU tests run)
NEW = ("hcir_bn2d_fwd_nhwc_f16", "hcir_bn2d_bwd_nhwc_f16", "hcir_bn2d_workspace_bytes", "hcir_bn2d_chunks")
HCIR_ERR_INVALID, HCIR_ERR_UNSUPPORTED, HCIR_ERR_WORKSPACE = -1, -2, -4
FIELDS = ["cv", "wv_log2", "slabs", "rpp", "chunks", "rows_per_chunk", "apply_blocks", "bytes"]
MS = [2, 3, 75, 196, 2352, 25088, 802816, 328149, 82369, 41209, 20535, 10309, 37303, 22445, 13467, 11163]
CS = [64, 128, 192, 256, 320, 384, 512, 1024, 2048]
BELOW_BAR = ()


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
    # the header's rule: 512 channels of one row when C % 512 == 0, else the largest of 32, 16, 8 vectors that divides
    # C / 8 (C = 64: 8 whole rows per wavefront; 192 and 320: 8 vectors over 3 and 5 slabs; 384: 16 over 3)
    assert wv == (64 if p["cv"] % 64 == 0 else max(w for w in (32, 16, 8) if p["cv"] % w == 0))
    assert p["slabs"] == {64: 1, 128: 1, 192: 3, 256: 1, 320: 5, 384: 3, 512: 1, 1024: 2, 2048: 4}[c]
    # the restatement the GPU tests assert their branches through: field for field
    q = ob.plan(m, c)
    assert all(getattr(q, k) == p[k] for k in FIELDS[:-1]), (q, p)
    assert q.chunk_passes * q.rpp == q.rows_per_chunk and q.last_rows == m - (q.chunks - 1) * q.rows_per_chunk
    assert q.trips == -(-(-(-m // q.rpp)) // q.apply_blocks) and q.per == -(-q.chunks // 64)
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


# ---------------------------------------------------------------------------------------------------------------
# oracle.bn2d: which branch each shape reaches, and bounds that are honest and sharp
# ---------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2)
SHARP_SHAPES = [(3, 5, 5, 64), (3, 67, 67, 320), (61, 13, 13, 2048), (101, 57, 57, 64)]


def _trunk_shapes(batch, size):
    """[M, C] of every body BatchNorm2d of ResNet-18 and ResNet-50 at batch x 3 x size x size"""
    out = set()
    side = size // 4
    for k, width in enumerate((64, 128, 256, 512)):
        m_in = batch * side * side
        side = side if k == 0 else side // 2
        m_out = batch * side * side
        out |= {(m_in, width), (m_out, width), (m_out, 4 * width)}
    return sorted(out)


def _small(p):
    return p.chunk_passes <= 4 and p.trips == 1 and p.per == 1 and not p.clamped


def test_which_branches_the_shapes_reach():
    """the suite's older shapes all take the small-map branch, no training batch does, the new shapes do not"""
    assert ob.SMALL_SHAPES == older.G1_SHAPES and (1, 56, 56, 64) in older.small_map_shapes()
    for shape in older.small_map_shapes():           # G1 to G5 of tests/test_bn2d_gpu.py, from its own lists
        assert _small(ob.plan(ob.rows_of(shape), shape[3])), shape
    assert set(older.G6_SHAPES) <= set(ob.CAPPED_SHAPES + ob.STRIDED_SHAPES)
    for m, c in _trunk_shapes(4, 64):
        assert _small(ob.plan(m, c)), (m, c)
    for shape in ob.CAPPED_SHAPES:
        p = ob.plan(ob.rows_of(shape), shape[3])
        assert p.clamped and p.chunk_passes == 6 and p.trips == 6 and p.per >= 2, shape
        assert p.last_rows < p.rows_per_chunk
        assert 20e6 < ob.rows_of(shape) * shape[3] < 22e6
    for shape in ob.STRIDED_SHAPES:
        p = ob.plan(ob.rows_of(shape), shape[3])
        assert not p.clamped and p.chunk_passes == 4 and p.trips == 2 and p.per >= 2, shape
        assert p.last_rows < p.rows_per_chunk
    assert [ob.plan(ob.rows_of(s), s[3]).slabs for s in ob.STRIDED_SHAPES] == [1, 3, 5, 3]
    assert [ob.plan(ob.rows_of(s), s[3]).slabs for s in ob.CAPPED_SHAPES] == [1, 1, 1, 2, 4]
    assert [ob.plan(ob.rows_of(s), s[3]).last_rows for s in ob.CAPPED_SHAPES] == [21, 1, 1, 15, 13]
    assert [ob.plan(ob.rows_of(s), s[3]).chunks for s in ob.CAPPED_SHAPES] == [1710, 1717, 1718, 856, 430]
    assert set(ob.PROBE_SHAPES) <= set(ob.CAPPED_SHAPES + ob.STRIDED_SHAPES)
    # a real step (batch 256): every layer strides the apply grid and merges several chunks per finalize lane; the
    # chunk count is clamped wherever a quarter of the passes exceeds the cap: everywhere but the 7 x 7 maps at C = 512
    # and the 14 x 14 maps at C = 256 (ResNet-18 layer4 and layer3, ResNet-50's bottleneck widths there), which run
    # 4 passes per chunk like the STRIDED shapes
    unclamped = {(12544, 512): (4, 2, 13), (50176, 256): (4, 4, 25)}
    for m, c in _trunk_shapes(256, 224):
        p = ob.plan(m, c)
        assert p.trips >= 2 and p.per >= 2 and not _small(p), (m, c)
        if (m, c) in unclamped:
            assert not p.clamped and (p.chunk_passes, p.trips, p.per) == unclamped[(m, c)], (m, c, p)
        else:
            assert p.clamped and p.chunk_passes >= 5, (m, c, p)
    p = ob.plan(802816, 64)
    assert (p.chunks, p.chunk_passes, p.trips, p.per) == (1930, 13, 13, 31)
    assert (ob.plan(12544, 2048).chunk_passes, ob.plan(12544, 2048).trips) == (7, 7)


@pytest.fixture(scope="module")
def bounds_table():
    rows = []
    yield rows
    print("\nbn2d-emu: fp32 emulation of the reduction order, worst err / bound per shape and family "
          "(statistics must stay <= 0.25, sums <= 1)")
    for r in rows:
        print(r)


def _problem(family, shape, n, seed=0):
    return ob.make_problem(family, ob.rows_of(shape), n, seed=seed + shape[3] + shape[0])


def _channels(shape):
    """the shape's own C up to 5 M elements (every small and STRIDED shape), else as many channels as 5 M elements
    hold (the order of the reduction is the same for every channel)"""
    return min(shape[3], max(16, 5_000_000 // ob.rows_of(shape)))


@pytest.mark.parametrize("shape", ob.SMALL_SHAPES + ob.STRIDED_SHAPES + ob.CAPPED_SHAPES, ids=str)
def test_emulation_within_a_quarter_of_the_statistics_bounds_and_within_the_sum_bounds(shape, bounds_table):
    """every family over SEEDS, at the shape's own channel count (_channels): the rule that fixes oracle.bn2d.STAT"""
    p = ob.plan(ob.rows_of(shape), shape[3])
    assert _channels(shape) == shape[3] or shape in ob.CAPPED_SHAPES
    for family, seed in ((f, s) for f in ob.FAMILIES for s in SEEDS):
        prob = _problem(family, shape, _channels(shape), seed)
        x = prob["x"]
        mean, var = ob.stats_f64(x)
        b_mean, b_var = ob.stat_bounds(mean, var)
        e_mean, e_var, e_rstd = ob.emulate_stats(x, p)
        w = {"mean": ob.ratio(e_mean, mean, b_mean), "var": ob.ratio(e_var, var, b_var),
             "rstd": ob.ratio(e_rstd, ob.rstd_f64(var), ob.rstd_bound(var, b_var))}
        for relu in (False, True):
            g = ob.masked(prob["dy"], prob["resid"] if relu else None)
            dbeta, b_dbeta, dgamma, b_dgamma, _ = ob.sums_f64(g, x, e_mean, e_rstd, p.depth)
            e_dbeta, e_dgamma = ob.emulate_sums(g, x, e_mean, e_rstd, p)
            w[f"dbeta/relu{int(relu)}"] = ob.ratio(e_dbeta, dbeta, b_dbeta)
            w[f"dgamma/relu{int(relu)}"] = ob.ratio(e_dgamma, dgamma, b_dgamma)
        bounds_table.append(f"bn2d-emu {str(shape):22s} {family:14s} seed {seed} " +
                            " ".join(f"{k} {v:.4f}" for k, v in w.items()))
        assert all(v <= (0.25 if k in ("mean", "var", "rstd") else 1.0) for k, v in w.items()), (shape, family, w)


def _exact_breaks(shape, mistake, n=8):
    """does the mistake, applied to the float64 chain, fail the exact-sum or the hot-row checks of the GPU tests?"""
    m = ob.rows_of(shape)
    p = ob.plan(m, shape[3])
    for with_mask in (False, True):
        prob = ob.exact_problem(m, n, with_mask)
        dbeta, dgamma = ob.exact_sums(prob)
        assert 6 * m < 2 ** 24                       # |dy| <= 2, |x| <= 3: every partial sum is an exact fp32 integer
        out = ob.chain_f64(prob, p, False, False, mistake, given=(prob["mean"], prob["rstd"]))
        if not (torch.equal(out["dbeta"], dbeta.double()) and torch.equal(out["dgamma"], dgamma.double())):
            return True
    base = ob.exact_problem(m, n, False)
    zeros = dict(resid=torch.zeros(m, n), gamma=torch.ones(n), beta=torch.zeros(n), rm=torch.zeros(n), rv=torch.ones(n))
    mean, rstd = ob.hot_stats(m)
    for r in ob.probe_rows(m, p):
        out = ob.chain_f64(dict(zeros, x=ob.hot_x(m, n, r), dy=base["dy"]), p, False, False, mistake)
        if not ((out["save_mean"] - mean).abs().max() <= ob.HOT_TOL * mean and
                (out["save_rstd"] - rstd).abs().max() <= ob.HOT_TOL * rstd):
            return True
        dy = ob.hot_dy(m, n, r)
        out = ob.chain_f64(dict(base, dy=dy), p, False, False, mistake, given=(base["mean"], base["rstd"]))
        want = (dy[r] * base["x"][r]).double()
        if not (torch.equal(out["dbeta"], dy[r].double()) and torch.equal(out["dgamma"], want)):
            return True
    return False


@pytest.fixture(scope="module")
def mistake_factors():
    """{mistake: {shape: (largest err / bound over the families and outputs, seen by the exact checks or None)}}"""
    table = {}
    for shape in SHARP_SHAPES:
        m = ob.rows_of(shape)
        p = ob.plan(m, shape[3])
        assert not _exact_breaks(shape, None)
        per = {}
        for family in ob.FAMILIES:
            prob = _problem(family, shape, 8)
            ref = ob.check_outputs(prob, p, True, True, ob.chain_f64(prob, p, True, True))
            assert max(ref.values()) <= 1e-6, ref          # the chain itself: float64 rounding against the bounds
            for mistake in ob.MISTAKES:
                if (mistake == ob.TRIP and p.trips == 1) or (mistake == ob.COUNT and p.chunks == 1):
                    continue                        # one trip, one chunk: the mistake has nothing to change
                w = ob.check_outputs(prob, p, True, True, ob.chain_f64(prob, p, True, True, mistake), truth=False)
                per.setdefault(mistake, {})[family] = max(w.values())
        for mistake, fam in per.items():
            worst = max(fam.values())
            exact = _exact_breaks(shape, mistake) if worst < 10.0 or mistake == ob.LOST else None
            table.setdefault(mistake, {})[shape] = (fam, exact)
    print("\nbn2d-mut: kernel mistakes applied to the float64 chain, largest err / bound per family; where the float "
          "bounds see less than 10 x, whether the exact-sum / hot-row checks break")
    for mistake, shapes in table.items():
        for shape, (fam, exact) in shapes.items():
            print(f"bn2d-mut  {mistake:62s} {str(shape):20s} " + "  ".join(f"{k} {v:.3g}" for k, v in fam.items()) +
                  ("" if exact is None else f"   exact checks break: {exact}") +
                  ("   BELOW THE 10x BAR" if mistake in BELOW_BAR else ""))
    return table


def test_every_mistake_exceeds_a_bound_tenfold(mistake_factors):
    assert set(mistake_factors) == set(ob.MISTAKES) and len(ob.MISTAKES) == 8
    for mistake, shapes in mistake_factors.items():
        best = max(max(fam.values()) for fam, _ in shapes.values())
        if mistake in BELOW_BAR:
            assert best > 1.0, (mistake, best)
        else:
            assert best >= 10.0, (mistake, best)


GEOMETRY = (ob.LOST, ob.COUNT, ob.TRIP, ob.INVM)        # mistakes a plan branch can hide: held at every shape


def test_no_mistake_is_unseen_by_both_the_bounds_and_the_exact_checks(mistake_factors):
    """A mistake of the row geometry is seen at every shape it can occur at: 10 x a float bound, or a broken exact-sum
    / hot-row check (one lost row among 3 x 10^5 moves the mean by 3 ulps: only the exact checks see it).  The others
    are arithmetic that no branch hides; their effect may shrink with M below any bound that admits honest rounding
    (the biased running_var: momentum var / M, 3 ulps at M = 328149; 25 - 50 x the bound at M <= 13467)."""
    for mistake, shapes in mistake_factors.items():
        for shape, (fam, exact) in shapes.items():
            if mistake in GEOMETRY:
                assert max(fam.values()) >= 10.0 or exact, (mistake, shape, fam, exact)
        assert any(max(fam.values()) >= 10.0 or exact for fam, exact in shapes.values()), (mistake, shapes)
    # a lost row: 1 / M of the mean, 5 - 20 x the bound only where |x[r]| > sigma; exact at every shape
    assert all(exact is True for _, exact in mistake_factors[ob.LOST].values())


def test_reference_pieces_are_consistent():
    """the float64 chain against F.batch_norm's own float64 autograd, the closed forms of the hot-row map, and the
    propagated bounds not below the elementwise ones"""
    shape = (3, 5, 5, 64)
    m, p = ob.rows_of(shape), ob.plan(75, 64)
    prob = _problem("random_buffers", shape, 16)
    for relu, resid in ((True, True), (False, False)):
        ref = ob.chain_f64(prob, p, relu, resid)
        truth = ob.truth_f64(prob["x"], prob["resid"] if resid else None, prob["dy"], prob["gamma"], prob["beta"],
                             (ref["y"] > 0) if relu else None, p.depth)
        r = prob["resid"] if resid else None
        own = {"y": ob.fwd_f64(prob["x"], ref["save_mean"], ref["save_rstd"], prob["gamma"], prob["beta"], r, relu)[1],
               "dx": ob.dx_f64(ob.masked(prob["dy"], ref["y"] if relu else None), prob["x"], ref["save_mean"],
                               ref["save_rstd"], prob["gamma"], ref["dgamma"], ref["dbeta"], m)[1]}
        for k in ("y", "dx"):
            assert (truth[k][0] - ref[k]).abs().max() <= 1e-11
            assert (truth[k][1] >= own[k] * (1 - 1e-9)).all()
    rm, rv = prob["rm"].double().clone(), prob["rv"].double().clone()
    torch.nn.functional.batch_norm(prob["x"].double(), rm, rv, None, None, True, ob.MOMENTUM, ob.EPS)
    ref = ob.chain_f64(prob, p, False, False)
    assert (rm - ref["running_mean"]).abs().max() <= 1e-12 and (rv - ref["running_var"]).abs().max() <= 1e-12
    mean, var = ob.stats_f64(ob.hot_x(m, 4, 7))
    want = ob.hot_stats(m)
    assert (mean - want[0]).abs().max() <= 1e-12 and (ob.rstd_f64(var) - want[1]).abs().max() <= 1e-12
    assert ob.probe_rows(328149, ob.plan(328149, 64)) == [0, 31, 32, 191, 192, 65535, 65536, 328128, 328148]
