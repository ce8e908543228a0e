"""CPU tests of the hcir_sim_topk host plan: csrc/sim_plan.h compiled for the host (tests/sim_plan_emul.cpp).

Which flow a call takes, its kernel geometry, prefix, grids and candidate capacity are only visible on a GPU as speed: a
wrong grid or prefix still gives exact answers.  PLANS pins them for a table of shapes with at least one shape on each
side of every branch point of sim_topk_plan.  The expected values were recorded from the launches of the commit BEFORE
the plan became a struct (its hcir_sim_topk with every kernel launch replaced by a printer of kernel, grid and
arguments), not from sim_plan.h.

Three guards of the plan cannot fail for any gallery that has a prefix at all (ng >= 32768), so no shape sits on their
far side: the candidate prefix is at most max(8192, ng / 8) rows rounded up to 256 (`S < ng`), it is at least 8192
rows = 32 units >= 4 * 4 groups (the `4 * G` tile minimum), and the list prefix is at most max(8192, ng / 16) rows
(`ng - prefix >= 4096` above 128 queries).  The shapes with ng = 32768 are the closest; test_candidate_guard calls the
candidate planner directly below that size."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _topk_route_shapes import INSTANTIATIONS, ROUTE_SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["flow", "kp", "qb", "gm", "npass", "S", "grid_a", "grid_b", "fallback_phases", "phase_a_done", "G", "cand_qb",
          "cand_grid_a", "cand_grid_b", "select", "cand_cap", "cand_alloc", "big_grid_x", "big_grid_y", "bytes"]
SINGLE, TWO_PHASE, CANDIDATE, BIG_TILE, MULTIPASS = range(5)                 # SimFlow
SEL_NONE, SEL_WAVE_SMALL, SEL_WAVE, SEL_FOUR_WAVES = range(4)                # SimSelect
F32, F16, BF16 = range(3)

# ((nq, ng, d, k, dtype, norms present), (FIELDS...))
PLANS = [
    # 1 M x 768 fp16, k = 16 over the query count: 32 | 33 (candidate flow | list flow on 128-row tiles, 768 workgroups),
    # 64 | 65 (-> 128 queries per workgroup), 128 | 129 (-> big-tile flow)
    ((32, 1000000, 768, 16, 1, 0), (2, 16, 32, 256, 1, 125184, 489, 512, 2, 1, 1, 32, 489, 512, 1, 448, 960, 0, 0, 3396864)),
    ((33, 1000000, 768, 16, 1, 0), (1, 16, 64, 128, 1, 62592, 489, 768, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 3503616)),
    ((64, 1000000, 768, 16, 1, 0), (1, 16, 64, 128, 1, 62592, 489, 768, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 6793216)),
    ((65, 1000000, 768, 16, 1, 0), (1, 16, 128, 128, 1, 62592, 489, 512, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 6900480)),
    ((128, 1000000, 768, 16, 1, 0), (1, 16, 128, 128, 1, 62592, 489, 512, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 13586176)),
    ((129, 1000000, 768, 16, 1, 0), (3, 16, 128, 128, 1, 62592, 256, 256, 2, 1, 0, 0, 0, 0, 0, 960, 960, 256, 1, 13693440)),
    ((220, 1000000, 768, 16, 1, 0), (3, 16, 128, 128, 1, 62592, 256, 256, 2, 1, 0, 0, 0, 0, 0, 960, 960, 256, 1, 23351296)),
    # above 128 queries the big-tile flow needs fp16 / bf16, d % 64 == 0, no norms, k <= 16
    ((220, 1000000, 768, 16, 0, 0), (1, 16, 128, 128, 1, 62592, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 23351296)),
    ((220, 1000000, 72, 16, 1, 0), (1, 16, 128, 128, 1, 62592, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 23351296)),
    ((220, 1000000, 768, 16, 1, 1), (1, 16, 128, 128, 1, 62592, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 23351296)),
    ((220, 1000000, 768, 17, 2, 0), (1, 32, 128, 128, 1, 62592, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 45006336)),
    ((880, 1000000, 768, 10, 2, 0), (3, 16, 128, 128, 1, 62592, 72, 72, 2, 1, 0, 0, 0, 0, 0, 960, 960, 64, 4, 93403392)),
    ((300, 1250000, 1024, 1, 1, 0), (3, 16, 128, 128, 1, 78208, 168, 168, 2, 1, 0, 0, 0, 0, 0, 960, 960, 128, 2, 31842304)),
    ((1, 1000000, 768, 10, 1, 0), (2, 16, 32, 256, 1, 125184, 489, 512, 2, 1, 1, 32, 489, 512, 1, 448, 960, 0, 0, 107520)),
    # 1.25 M x 1024 over k: 16 | 17 (one floor -> group floors, 3008-slot buffers), 32 | 33 (-> 64-entry fallback lists),
    # 64 | 65 (-> two passes)
    ((32, 1250000, 1024, 17, 1, 0), (2, 32, 32, 256, 1, 32256, 512, 0, 1, 0, 2, 32, 126, 512, 3, 3008, 3008, 0, 0, 7070976)),
    ((32, 1250000, 1024, 32, 1, 0), (2, 32, 32, 256, 1, 32256, 512, 0, 1, 0, 2, 32, 126, 512, 3, 3008, 3008, 0, 0, 7070976)),
    ((32, 1250000, 1024, 33, 1, 0), (2, 64, 32, 256, 1, 48128, 512, 0, 1, 0, 3, 32, 188, 512, 3, 3008, 3008, 0, 0, 13370624)),
    ((64, 1250000, 1024, 50, 1, 0), (2, 64, 32, 256, 1, 65792, 256, 0, 1, 0, 4, 64, 512, 768, 3, 3008, 3008, 0, 0, 26740736)),
    ((64, 1250000, 1024, 64, 0, 0), (2, 64, 32, 256, 1, 65792, 256, 0, 1, 0, 4, 64, 512, 768, 3, 3008, 3008, 0, 0, 26740736)),
    ((64, 1250000, 1024, 65, 1, 0), (4, 64, 32, 256, 2, 1250000, 256, 0, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 25692160)),
    ((128, 1250000, 1024, 50, 2, 0), (2, 64, 32, 256, 1, 65792, 128, 0, 1, 0, 4, 128, 512, 512, 3, 3008, 3008, 0, 0, 53481216)),
    ((129, 1250000, 1024, 50, 1, 0), (1, 64, 32, 256, 1, 16384, 64, 96, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 51786240)),
    ((33, 1250000, 1024, 17, 1, 0), (2, 32, 64, 256, 1, 32256, 512, 0, 1, 0, 2, 64, 252, 768, 3, 3008, 3008, 0, 0, 7292416)),
    ((65, 1250000, 1024, 32, 1, 0), (2, 32, 128, 128, 1, 32128, 512, 0, 1, 0, 2, 128, 251, 512, 3, 3008, 3008, 0, 0, 14363392)),
    # ng 32767 | 32768: the smallest gallery with a prefix, in the list, candidate (one floor, group floors) and big flow
    ((64, 32767, 768, 10, 1, 0), (0, 16, 64, 128, 1, 32767, 256, 0, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 6793216)),
    ((64, 32768, 768, 10, 1, 0), (1, 16, 64, 128, 1, 8192, 64, 192, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 6793216)),
    ((32, 32767, 768, 16, 1, 0), (0, 16, 32, 256, 1, 32767, 128, 0, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 3396864)),
    ((32, 32768, 768, 16, 1, 0), (2, 16, 32, 256, 1, 8192, 32, 96, 2, 1, 1, 32, 32, 96, 1, 448, 960, 0, 0, 3396864)),
    ((32, 32768, 64, 50, 1, 0), (2, 64, 32, 256, 1, 8192, 128, 0, 1, 0, 4, 32, 32, 128, 3, 3008, 3008, 0, 0, 13370624)),
    ((220, 32768, 768, 16, 1, 0), (3, 16, 128, 128, 1, 8192, 64, 192, 2, 1, 0, 0, 0, 0, 0, 960, 960, 96, 1, 23351296)),
    ((1, 500, 64, 1, 0, 0), (0, 16, 32, 256, 1, 500, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 107520)),
    ((20, 8192, 72, 100, 0, 1), (4, 64, 32, 256, 2, 8192, 32, 0, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 8029440)),
    ((880, 1000000, 768, 642, 1, 0), (4, 64, 32, 256, 11, 1000000, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 353263872)),
    ((20, 300000, 768, 16, 2, 1), (2, 16, 32, 256, 1, 37632, 147, 512, 2, 1, 1, 32, 147, 512, 1, 448, 960, 0, 0, 2123520)),
    # 38 * (rows behind the prefix / prefix rows + 1) <= 64 * 7: 418 | 456 (448-slot buffers and the 8-slot select | 960, 16)
    ((32, 1500000, 768, 16, 1, 0), (2, 16, 32, 256, 1, 131072, 512, 512, 2, 1, 1, 32, 512, 512, 1, 448, 960, 0, 0, 3396864)),
    ((32, 1600000, 768, 16, 1, 0), (2, 16, 32, 256, 1, 131072, 512, 512, 2, 1, 1, 32, 512, 512, 2, 960, 960, 0, 0, 3396864)),
    ((128, 70000, 1024, 33, 0, 0), (2, 64, 32, 256, 1, 8192, 128, 0, 1, 0, 3, 128, 64, 512, 3, 3008, 3008, 0, 0, 53481216)),
    ((65, 131072, 768, 10, 1, 0), (1, 16, 128, 128, 1, 8192, 64, 512, 0, 0, 0, 0, 0, 0, 0, 0, 960, 0, 0, 6900480)),
]


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libsim_plan_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "sim_plan_emul.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.emul_sim_topk_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.emul_sim_workspace_layout.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    L.emul_sim_plan_candidate.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    L.emul_geom.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_merge_route.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    L.emul_merge_launches.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return L


def plan(L, nq, ng, d, k, dtype, norms):
    out = np.zeros(len(FIELDS), np.int64)
    L.emul_sim_topk_plan(nq, ng, d, k, dtype, norms, norms, out.ctypes.data)
    return dict(zip(FIELDS, (int(v) for v in out)))


@pytest.mark.parametrize("shape,want", PLANS, ids=["-".join(map(str, s)) for s, _ in PLANS])
def test_plan_of_pinned_shapes(emul, shape, want):
    got = plan(emul, *shape)
    assert got == dict(zip(FIELDS, want))


def test_table_has_both_sides_of_every_branch_point():
    flows = {w[0] for _, w in PLANS}
    assert flows == {SINGLE, TWO_PHASE, CANDIDATE, BIG_TILE, MULTIPASS}
    nqs, ks, ngs = {s[0] for s, _ in PLANS}, {s[3] for s, _ in PLANS}, {s[1] for s, _ in PLANS}
    assert {32, 33, 64, 65, 128, 129} <= nqs and {16, 17, 32, 33, 64, 65} <= ks and {32767, 32768} <= ngs
    many = [(s, dict(zip(FIELDS, w))) for s, w in PLANS if s[0] > 128 and s[3] <= 16 and s[1] >= 32768]
    assert {w["flow"] for s, w in many if s[4] == F32} == {TWO_PHASE}
    assert {w["flow"] for s, w in many if s[2] % 64} == {TWO_PHASE}
    assert {w["flow"] for s, w in many if s[5]} == {TWO_PHASE}
    assert {w["flow"] for s, w in many if s[4] != F32 and s[2] % 64 == 0 and not s[5]} == {BIG_TILE}
    selects = {dict(zip(FIELDS, w))["select"] for _, w in PLANS}
    assert selects == {SEL_NONE, SEL_WAVE_SMALL, SEL_WAVE, SEL_FOUR_WAVES}
    caps = {dict(zip(FIELDS, w))["cand_cap"] for _, w in PLANS}
    assert caps == {0, 64 * 7, 960, 3008}
    fallbacks = {(w[FIELDS.index("fallback_phases")], w[FIELDS.index("phase_a_done")]) for _, w in PLANS}
    assert fallbacks == {(0, 0), (1, 0), (2, 1)}


def test_workspace_bytes_match_the_library(emul, hcir_built):
    """The plan's byte count is what hcir_sim_topk_workspace_bytes hands out (no dependence on d, dtype or norms)."""
    for shape, want in PLANS:
        nq, ng, d, k, dtype, norms = shape
        assert hcir_built.hcir_sim_topk_workspace_bytes(nq, ng, d, k, dtype) == want[-1] == plan(emul, *shape)["bytes"]
    rng = np.random.default_rng(0)
    for _ in range(300):
        nq, ng = int(rng.integers(1, 1200)), int(rng.integers(1, 3_000_000))
        k, d, dtype = int(rng.integers(1, 1025)), 8 * int(rng.integers(1, 200)), int(rng.integers(0, 3))
        assert hcir_built.hcir_sim_topk_workspace_bytes(nq, ng, d, k, dtype) == plan(emul, nq, ng, d, k, dtype, 0)["bytes"]
    assert hcir_built.hcir_sim_topk_workspace_bytes(0, 100, 64, 1, 0) == 0
    assert hcir_built.hcir_sim_topk_workspace_bytes(1, 100, 64, 0, 0) == 0


def test_workspace_layout(emul):
    """Buffers in carving order, 256-byte aligned, disjoint, each as large as its users need."""
    for nq, kp, alloc in [(1, 16, 960), (32, 16, 960), (33, 32, 3008), (128, 64, 3008), (880, 16, 960), (7, 64, 960)]:
        o = np.zeros(12, np.int64)
        emul.emul_sim_workspace_layout(nq, kp, alloc, o.ctypes.data)
        o = [int(v) for v in o]
        flag, o = o[10], o[:10] + o[11:]
        assert flag == o[9] + 4 * nq and flag + 4 <= o[10]          # the overflow flag sits behind the nq counters
        assert o[0] == 0 and all(v % 256 == 0 for v in o) and o == sorted(o)
        parts = emul.emul_max_parts()
        need = [parts * nq * kp * 4] * 2 + [nq * kp * 4] * 2 + [4 * nq * 4, nq * 4, nq * 4] + [alloc * nq * 4] * 2 + \
               [(nq + 1) * 4]
        for i, n in enumerate(need):
            assert 0 <= o[i + 1] - o[i] - n < 256, (nq, kp, alloc, i)


def test_geometry_table(emul):
    """kMaxParts covers every grid the table allows; rows exist exactly for the instantiated kernels."""
    gm, wg = ctypes.c_int32(), ctypes.c_int32()
    rows = {}
    for kp in (16, 32, 64):
        for qb in (32, 64, 128):
            if emul.emul_geom(kp, qb, ctypes.byref(gm), ctypes.byref(wg)):
                rows[kp, qb] = (gm.value, wg.value)
    assert set(rows) == {(16, 32), (16, 64), (16, 128), (32, 32), (32, 64), (32, 128), (64, 32)}
    assert rows[16, 64] == (128, 768) and rows[16, 32] == (256, 512) and rows[16, 128] == (128, 512)
    assert emul.emul_max_parts() == max(w for _, w in rows.values()) == 768
    assert not emul.emul_geom(64, 64, ctypes.byref(gm), ctypes.byref(wg))
    for shape, want in PLANS:
        w = dict(zip(FIELDS, want))
        assert (w["gm"], max(w["grid_a"], w["grid_b"]) <= rows[w["kp"], w["qb"]][1]) == (rows[w["kp"], w["qb"]][0], True)
        assert max(w["cand_grid_a"], w["cand_grid_b"], w["grid_a"], w["grid_b"]) <= emul.emul_max_parts()


def test_candidate_guard(emul):
    """`S < ng` of the candidate planner: a gallery no longer than the 8192-row minimum prefix is refused and the
    plan is left alone; one row more is planned."""
    S = ctypes.c_int64()
    for nq, k in ((1, 1), (32, 16), (64, 50), (128, 64)):
        for ng in (500, 8191, 8192):
            assert emul.emul_sim_plan_candidate(nq, ng, k, ctypes.byref(S)) == 0 and S.value == -1
        assert emul.emul_sim_plan_candidate(nq, 8193, k, ctypes.byref(S)) == 1 and S.value == 8192


# ---- merge routing (sim_merge_route): which kernel of csrc/topk_merge.h a launch gets, and that it can hold its lists
MERGE_NONE, MERGE_FOUR_WAVES, MERGE_WAVE, MERGE_SELECT = range(4)            # SimMergeKind
MERGE_KERNEL = {MERGE_FOUR_WAVES: "merge32q", MERGE_WAVE: "merge32", MERGE_SELECT: "merge_sel"}
SELECT_KERNEL = {SEL_WAVE_SMALL: ("select", 8), SEL_WAVE: ("select", 16), SEL_FOUR_WAVES: ("select4", 13)}


def merge_launches(L, nq, ng, d, k, dtype, norms):
    """[(total lists, kout, groups, kind, lpl, capacity)] of every merge launch of the call, fallback included"""
    out = np.zeros((16, 6), np.int32)
    n = L.emul_merge_launches(nq, ng, d, k, dtype, norms, norms, out.ctypes.data, 16)
    assert 1 <= n <= 16
    return [tuple(int(v) for v in row) for row in out[:n]]


def routes_reached(L, nq, ng, d, k, dtype=F32, norms=0):
    r = {(MERGE_KERNEL[kind], lpl) for _, _, _, kind, lpl, _ in merge_launches(L, nq, ng, d, k, dtype, norms)}
    sel = plan(L, nq, ng, d, k, dtype, norms)["select"]
    return r | ({SELECT_KERNEL[sel]} if sel != SEL_NONE else set())


def test_merge_route_table(emul):
    """sim_merge_route on both sides of each of its thresholds: 256 lists per lane slot of the four-wave kernel up to
    1024, kout 16 | 17, groups."""
    def route(total, kout, groups):
        o = np.zeros(3, np.int32)
        emul.emul_merge_route(total, kout, groups, o.ctypes.data)
        return tuple(int(v) for v in o)
    for total, lpl in ((1, 1), (256, 1), (257, 2), (512, 2), (513, 3), (768, 3), (769, 4), (961, 4), (1024, 4)):
        assert route(total, 16, 1) == route(total, 1, 0) == (MERGE_FOUR_WAVES, lpl, 256 * lpl)
    assert route(1025, 16, 1) == route(4, 17, 1) == route(576, 64, 1) == (MERGE_WAVE, 9, 576)
    assert route(577, 17, 1)[2] < 577                      # more lists than any kernel holds: the launcher refuses
    assert route(512, 16, 2) == (MERGE_SELECT, 9, 1152) and route(512, 16, 4) == (MERGE_SELECT, 9, 2304)
    assert route(512, 17, 2) == (MERGE_NONE, 0, 0)


def test_every_merge_launch_holds_its_lists(emul):
    """Sweep of shapes over every branch point of the plan: each merge launch the flow and its gated fallback make
    goes to a kernel with at least as many list slots as the launch has lists (a smaller one would silently drop lists
    and return wrong neighbours).  No launch needs more than 576 lists with kout > 16 - the one-wave kernel with 16
    lists per lane is not needed - and only the selection merge sees groups."""
    ngs = [37, 500, 1000, 4099, 8192, 8193, 20000, 32767, 32768, 40000, 60000, 90000, 120000, 131072, 131073, 300000,
           500000, 1000000, 1250000, 1500000, 1600000, 2000000]
    shapes = launches = 0
    seen = set()
    for nq in (1, 32, 33, 64, 65, 128, 129, 300, 880):
        for k in (1, 10, 16, 17, 32, 33, 50, 64, 65, 100, 642):
            for ng in ngs:
                if k > ng:
                    continue
                for dtype in (F32, F16, BF16):
                    for norms in (0, 1):
                        for d in (768, 72):
                            shapes += 1
                            for total, kout, groups, kind, lpl, cap in merge_launches(emul, nq, ng, d, k, dtype, norms):
                                launches += 1
                                assert kind != MERGE_NONE and cap >= total, (nq, ng, d, k, dtype, norms, total, kout)
                                assert not (total > 576 and kout > 16), (nq, ng, d, k, dtype, norms, total, kout)
                                assert 1 <= kout <= 64 and (groups > 1) == (kind == MERGE_SELECT)
                                if kind == MERGE_SELECT:
                                    assert kout == 16 and 2 <= groups <= 4
                                seen.add((MERGE_KERNEL[kind], lpl))
    assert shapes > 20000 and launches > shapes
    assert seen == {r for r in INSTANTIATIONS if r[0].startswith("merge")}


def test_route_shapes_reach_every_instantiation(emul):
    """The coverage table of the GPU test test_topk_merge_routes: each shape reaches exactly the routes written next
    to it, and together they reach every merge and select instantiation in the build."""
    union = set()
    for (nq, ng, d, k), want, _ in ROUTE_SHAPES:
        got = routes_reached(emul, nq, ng, d, k)
        assert got == want, ((nq, ng, d, k), got)
        union |= got
    assert union == INSTANTIATIONS


def test_instantiations_are_those_in_the_source():
    """INSTANTIATIONS against the launches written in csrc/sim_topk.hip (template arguments by name)."""
    import re
    consts = {"kMergeLPL": 9, "kSelLPLSmall": 8, "kCandLPL": 16, "kSel4LPL": 13}
    src = open(os.path.join(ROOT, "hair-centric-image-retrieval_amd", "csrc", "sim_topk.hip")).read()
    found = {(name, consts.get(arg) or int(arg))
             for name, arg in re.findall(r"hipLaunchKernelGGL\(topk_(merge32q|merge32|merge_sel|select4|select)_kernel<(\w+)>", src)}
    assert found == INSTANTIATIONS
