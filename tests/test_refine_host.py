"""oracle.refine and the case table of tests/_refine_cases.py, which tests/test_refine_gpu.py and
tests/test_gallery_gpu.py hold hcir_topk_refine_f32 and the certificate of ResidentGallery.search to.  No GPU.

The reference is right: refine_ref agrees bit for bit with a brute-force sort over every score of the gallery, on every
case.  The table can see: every entry of oracle.refine.MISTAKES, built into the reference or into the fp32 emulation
of E_i, fails at least one case, the recovery probe or a planted gallery.  The planted galleries are what they claim:
their preconditions hold in float64 by the stated margin.  Last, the argument checks of hcir_topk_refine_f32 refuse on
the host, before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_cases as rc  # noqa: E402
from oracle import refine as orf  # noqa: E402

SPECS = rc.specs()
HCIR_ERR_INVALID = -1


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(spec):
        key = rc.spec_id(spec)
        if key not in cache:
            cache[key] = rc.build(spec)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def probes():
    return {fam: orf.probe_make(*orf.probe_query(fam)) for fam in orf.PROBE_FAMILIES}


@pytest.fixture(scope="module")
def planted():
    return {kind: orf.plant(kind) for kind in ("query", "gallery")}


def test_the_table_covers_what_it_must():
    shapes = [(s["nq"], s["d"], s["kc"], s["k"]) for s in SPECS]
    assert {s[0] for s in shapes} >= {1, 3, 4, 5, 130}
    assert {s[1] for s in shapes} >= {8, 24, 40, 72, 256, 768, 2048}
    assert {s[2] for s in shapes} >= {1, 2, 16, 17, 63, 64}
    assert any(s[3] == 1 for s in shapes) and any(s[3] == s[2] for s in shapes) and any(1 < s[3] < s[2] for s in shapes)
    combos = {(s["idx_base"], s["use_qn"], s["use_gn"]) for s in SPECS if s["name"] == "combo"}
    assert len(combos) == 12 and len({rc.spec_id(s) for s in SPECS}) == len(SPECS)
    assert max(s["ng"] for s in SPECS) <= 4096


def test_the_table_holds_exact_equalities(cases):
    """queries with t + err == vk in real numbers, among the small cases the GPU test runs for them"""
    small = [cases(s) for s in SPECS if s["nq"] <= 5 and s["d"] <= 768]
    assert sum(int(c["equal"].sum()) for c in small) >= 10
    for c in small:                                                # and the lists stay sorted
        assert (c["cand_val"][:, 1:] <= c["cand_val"][:, :-1]).all()


@pytest.mark.parametrize("spec", SPECS, ids=rc.spec_id)
def test_refine_ref_is_the_brute_force_sort(spec, cases):
    case = cases(spec)
    ref = orf.refine_ref(err=case["err"], **rc.ref_args(case))
    assert orf.same_bits(ref, orf.brute_force(err=case["err"], **rc.ref_args(case)))
    val, idx, cert = ref
    kc, k = case["cand_idx"].shape[1], case["k"]
    given = case["cand_idx"][:, :k]
    if kc > 2 and spec["empty"] == 0 and not spec["nan"]:
        assert (idx != given).any(), "the candidates come in exact order: nothing to permute"
    if case["dup"] is not None and kc >= 2 and k >= kc - spec["empty"]:
        lo, hi = case["dup"][0] + case["idx_base"], case["dup"][1] + case["idx_base"]
        for row in idx:                                            # equal rows: the smaller index first, and adjacent
            p = list(row)
            assert p.index(hi) == p.index(lo) + 1
    decided = case["decided"] & ~case["equal"]
    if decided.sum() >= 2:
        assert set(cert[decided]) == {0, 1}
    assert (cert[case["equal"]] == 0).all()
    if spec["nan"] == "short":
        assert (case["cand_idx"][:, -1] >= 0).all() and (cert == 0).all() and (idx[:, -1] == -1).all()
    if spec["nan"]:
        assert not (idx == case["nan_row"] + case["idx_base"]).any() and not np.isnan(val).any()
    for err, want in rc.decision_runs(case):
        got = orf.refine_ref(err=err, **rc.ref_args(case))[2]
        assert (got[want >= 0] == want[want >= 0]).all()


def test_every_mistake_is_caught(cases, probes, planted):
    caught = {m: [] for m in orf.MISTAKES}
    for spec in SPECS:
        case = cases(spec)
        ref = orf.refine_ref(err=case["err"], **rc.ref_args(case))
        for m in orf.MISTAKES:
            if m not in orf.E_MISTAKES and not orf.same_bits(ref, orf.refine_ref(err=case["err"], mistake=m,
                                                                                  **rc.ref_args(case))):
                caught[m].append(rc.spec_id(spec))
    for fam, p in probes.items():
        for m in orf.E_MISTAKES:
            cert = orf.refine_ref(p["q"], p["g"], p["cand_idx"], p["cand_val"], orf.PROBE_K, consts=p["consts"],
                                  mistake=m)[2]
            b = orf.probe_bracket(p, cert)
            if not (b["inside"] and b["monotone"] and b["sound"] and b["tight"]):
                caught[m].append("probe " + fam)
    for kind, p in planted.items():
        f = orf.plant_facts(p)
        for m in orf.E_MISTAKES:                                   # a kernel with this E_i certifies a list without A
            e = orf.ei_kernel32(p["q"], orf.err_bound64(p["q"], p["g"])[1], m)[orf.PLANTED_QUERY]
            if np.float32(f["t"]) + e < np.float32(f["vk"]):
                caught[m].append("planted " + kind)
    print("\nrefine-mistakes: the cases that see each one")
    for m in orf.MISTAKES:
        print(f"refine-mistake {m:42s} {len(caught[m]):3d}  {', '.join(caught[m][:3])}")
    assert all(caught.values()), [m for m in caught if not caught[m]]
    assert "planted query" in caught[orf.NO_QTERM] and "planted gallery" in caught[orf.NO_GTERM]
    assert any(c.startswith("probe") for c in caught[orf.NO_FACTOR])


@pytest.mark.parametrize("family", orf.PROBE_FAMILIES)
def test_probe_recovers_the_emulated_bound(family, probes):
    """the fp32 emulation of the kernel's E_i lies inside the derived bounds, and the probe finds it"""
    p = probes[family]
    cert = orf.refine_ref(p["q"], p["g"], p["cand_idx"], p["cand_val"], orf.PROBE_K, consts=p["consts"])[2]
    b = orf.probe_bracket(p, cert)
    assert b["inside"] and b["monotone"] and b["sound"] and b["tight"], b
    e = float(orf.ei_kernel32(p["q"][:1], p["consts"])[0])
    assert b["lo"] <= e < b["hi"]
    assert abs(float(p["vk"])) < p["e64"] * 2.0 ** -8              # ulp(vk) does not limit the grid
    assert b["resolution"] < p["e64"] * 2.0 ** -20
    if family == "fp16 exact":
        assert (orf.f16(p["q"][0]) == p["q"][0]).all()
    if family == "below fp16":
        assert (orf.f16(p["q"][0]) == 0).all() and np.abs(p["q"][0]).max() > 0


@pytest.mark.parametrize("kind", ["query", "gallery"])
def test_planted_gallery_preconditions(kind, planted):
    p = planted[kind]
    f = orf.plant_facts(p)
    print(f"\nrefine-planted {kind:8s} E64 {f['e64']:.3e}  E_mutant {f['e_mut']:.3e}  err(A) {f['err_a']:.3e}  "
          f"window {f['window']:.3e}  t {f['t']:.7f}  vk {f['vk']:.7f}")
    assert all(f["holds"].values()), f["holds"]
    g, q = p["g"], p["q"][orf.PLANTED_QUERY]
    assert g.shape[1] == orf.PLANT_D and 16 < g.shape[0] <= 640
    if kind == "query":
        assert (orf.f16(g) == g).all() and not (orf.f16(q) == q).all()
        assert orf.err_bound64(q[None], g)[1][0] == 0.0            # eg
    else:
        assert (orf.f16(q) == q).all() and not (orf.f16(g[p["a"]]) == g[p["a"]]).all()


def test_argument_checks_refuse_before_any_launch(hcir_built):
    """null device pointers would fault if anything were launched or dereferenced; every call returns INVALID"""
    L = hcir_built
    consts = (ctypes.c_float * 4)(0, 1, 1, 1e-6)
    one = 4096                                                      # a non-null pointer that is never followed

    def call(nq=4, d=8, kc=4, k=2, err=one, mc=None):
        return L.hcir_topk_refine_f32(one, nq, one, 100, d, one, one, kc, k, 0, None, None, err, mc, one, one, one, None)

    assert call(d=12) == HCIR_ERR_INVALID
    assert call(kc=65, k=2) == HCIR_ERR_INVALID
    assert call(kc=4, k=5) == HCIR_ERR_INVALID
    assert call(err=None, mc=None) == HCIR_ERR_INVALID
    assert call(nq=0) == HCIR_ERR_INVALID and call(nq=-3) == HCIR_ERR_INVALID
    assert call(err=None, mc=consts, d=4) == HCIR_ERR_INVALID
