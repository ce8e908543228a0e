"""GPU parity of the "exact by verification" search (hcir.gallery.ResidentGallery):
results must be BIT-IDENTICAL to the exact fp32 scan / the C oracle, whether a query is certified
from the fp16-mirror candidates or falls back to the full fp32 scan.

The second half holds the certificate itself: the bound E_i over every (query, row) pair, not only the picked ones,
against the real-number bound of oracle.refine; the mirror's four constants; two planted galleries (oracle.refine.plant)
on which an E_i without its query term or its gallery term certifies a top-5 that misses a row; a mirror that
overflows; the mirror's dtype.  The refine kernel alone: tests/test_refine_gpu.py.  Figures: profiles/refine_bounds.txt."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import knn as oknn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _unit(shape, seed):
    x = np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("nq,ng,d,k", [(70, 60000, 768, 10), (5, 3000, 64, 5), (130, 40000, 256, 14), (3, 10, 8, 3)])
def test_filtered_search_is_exact(nq, ng, d, k):
    from hcir.gallery import ResidentGallery
    q, g = _unit((nq, d), 1), _unit((ng, d), 2)
    gal = ResidentGallery(torch.from_numpy(g).cuda(), idx_base=7)
    val, idx = gal.search(torch.from_numpy(q).cuda(), k)
    rv, ri = oknn.cosine_topk(q, g, k, idx_base=7)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)
    ev, ei = gal.search_exact(torch.from_numpy(q).cuda(), k)
    assert torch.equal(ei, idx) and torch.equal(ev, val)
    if ng > 16:
        assert gal.stats["queries"] == nq
        assert gal.stats["fallback_queries"] <= max(2, nq // 10)   # random data: almost all certified


def test_filtered_search_adversarial_near_duplicates():
    """Hundreds of gallery rows within 1e-5 of each other around the top of every query's ranking: the
    fp16 mirror cannot separate them, certification must fail and the fallback must restore exactness."""
    from hcir.gallery import ResidentGallery
    rng = np.random.default_rng(3)
    d, ng = 256, 20000
    g = _unit((ng, d), 4)
    q = _unit((12, d), 5)
    for i in range(6):                      # queries 0..5 get a cloud of 200 near-duplicate best matches
        base = q[i] + 0.05 * rng.standard_normal(d).astype(np.float32)
        rows = rng.choice(ng, 200, replace=False)
        g[rows] = base + 1e-5 * rng.standard_normal((200, d)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g[4321] = g[77]                          # exact duplicate rows: tie -> smaller index
    gal = ResidentGallery(torch.from_numpy(g).cuda())
    val, idx = gal.search(torch.from_numpy(q).cuda(), 10)
    rv, ri = oknn.cosine_topk(q, g, 10)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)
    assert gal.stats["fallback_queries"] >= 6     # the clouds cannot be certified
    assert gal.stats["fallback_queries"] < 12     # the ordinary queries are


def test_error_bound_holds():
    """The bound E_i used for certification really bounds |exact fp32 chain - fp16-mirror score|."""
    from hcir import ops
    from hcir.gallery import ResidentGallery
    q, g = _unit((16, 768), 6), _unit((5000, 768), 7)
    gal = ResidentGallery(torch.from_numpy(g).cuda())
    qd = torch.from_numpy(q).cuda()
    q16 = qd.half()
    err = gal.err_bound(qd, q16).cpu().numpy()
    s16, i16 = ops.sim_topk(q16, gal.mirror, 16)
    exact = oknn.scores(q, g)                                   # fp32 chain, all pairs
    picked = np.take_along_axis(exact, i16.cpu().numpy(), axis=1)
    diff = np.abs(picked - s16.cpu().numpy())
    assert (diff <= err[:, None]).all()
    assert err.max() < 2e-3 and diff.max() < err.max()          # and it is not vacuous


def test_in_kernel_bound_matches_python_bound():
    """hcir_topk_refine_f32 derives E_i itself from the mirror constants; it must certify exactly the
    queries the documented (python) bound certifies."""
    from hcir import _lib, ops
    from hcir.gallery import FILTER_KC, ResidentGallery
    q, g = _unit((64, 256), 10), _unit((20000, 256), 11)
    g[100:400] = g[50] + 2e-4 * np.random.default_rng(0).standard_normal((300, 256)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    q[:8] = g[50] + 0.02 * np.random.default_rng(1).standard_normal((8, 256)).astype(np.float32)
    gal = ResidentGallery(torch.from_numpy(g).cuda())
    qd = torch.from_numpy(q).cuda()
    q16 = qd.half()
    cval, cidx = ops.sim_topk(q16, gal.mirror, FILTER_KC)
    outs = []
    for err in (gal.err_bound(qd, q16), None):
        val = torch.empty((64, 10), device="cuda")
        idx = torch.empty((64, 10), dtype=torch.int64, device="cuda")
        cert = torch.empty(64, dtype=torch.int32, device="cuda")
        assert _lib.lib().hcir_topk_refine_f32(
            qd.data_ptr(), 64, gal.g32.data_ptr(), 20000, 256, cidx.data_ptr(), cval.data_ptr(), FILTER_KC, 10, 0,
            None, None, None if err is None else err.data_ptr(), None if err is not None else gal._consts,
            val.data_ptr(), idx.data_ptr(), cert.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        outs.append((val.cpu(), idx.cpu(), cert.cpu()))
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][1], outs[1][1])
    assert 0 < int((outs[1][2] == 0).sum()) < 64      # the planted cloud defeats some queries, not all


def test_sharded_gallery_uses_resident():
    from hcir.dist import ShardedGallery
    from hcir.gallery import ResidentGallery
    q, g = _unit((33, 128), 8), _unit((30000, 128), 9)
    gd = torch.from_numpy(g).cuda()
    sg = ShardedGallery(gd, 100, resident=ResidentGallery(gd, 100))
    val, idx = sg.search(torch.from_numpy(q).cuda(), 10)
    rv, ri = oknn.cosine_topk(q, g, 10, idx_base=100)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)


# ---------------------------------------------------------------------------------------------------------------
# the certificate end to end: the bound over every (query, row) pair, the mirror's constants, two planted galleries
# where a too-small E_i returns a wrong top-k, a mirror that overflows, the mirror's dtype
# ---------------------------------------------------------------------------------------------------------------
BOUND_FAMILIES = ("unit d8", "unit d768", "unit d2048", "mixed norms", "heavy tails", "fp16 subnormal",
                  "planted query", "planted gallery")
BOUND_ROWS = []


@pytest.fixture(scope="module")
def bound_table():
    yield BOUND_ROWS
    print("\nrefine-bound: max |fp32 chain - mirror score| / E64 over every (query, row) pair, per family")
    for r in BOUND_ROWS:
        print(r)


@pytest.fixture(scope="module")
def planted():
    from oracle import refine as orf
    return {kind: orf.plant(kind) for kind in ("query", "gallery")}


def _bound_family(name, planted):
    """-> (q, g) fp32, at most 640 rows"""
    rng = np.random.default_rng(len(name) + 100)
    if name.startswith("planted"):
        p = planted[name.split()[1]]
        return p["q"], p["g"]
    if name.startswith("unit"):
        d = int(name.split("d")[1])
        return _unit((16, d), 21), _unit((640, d), 22)
    d = 256
    q, g = rng.standard_normal((16, d)), rng.standard_normal((640, d))
    if name == "mixed norms":
        g *= 10.0 ** rng.uniform(-3, 2, (640, 1)) / np.sqrt(d)
        q *= 10.0 ** rng.uniform(-3, 2, (16, 1)) / np.sqrt(d)
    elif name == "heavy tails":
        q, g = rng.standard_t(2, (16, d)), rng.standard_t(2, (640, d))
    elif name == "fp16 subnormal":
        q, g = q * 2e-5, g * 2e-5                                  # below 2^-14 = 6.1e-5: fp16 keeps multiples of 2^-24
    return q.astype(np.float32), g.astype(np.float32)


def _mirror_scores(q16, mirror):
    """the filter's score of every pair: sim_topk over 64-row slices with k = the rows of the slice, scattered back"""
    from hcir import ops
    nq, ng = q16.shape[0], mirror.shape[0]
    s16 = torch.full((nq, ng), float("nan"), device="cuda")
    for s in range(0, ng, 64):
        rows = min(64, ng - s)
        val, idx = ops.sim_topk(q16, mirror[s:s + rows], rows)
        assert (torch.sort(idx, dim=1).values == torch.arange(rows, device="cuda")).all()
        s16[:, s:s + rows].scatter_(1, idx, val)
    return s16.cpu().numpy()


@pytest.mark.parametrize("family", BOUND_FAMILIES)
def test_error_bound_holds_for_every_pair(family, planted, bound_table):
    """|fp32 chain - mirror score| <= E64_i for EVERY row, the ones the filter did not pick included: the certificate
    is a statement about those.  E64 is the real-number bound (oracle.refine.err_bound64: no 1.01, no 1e-7) from the
    mirror the device made, and what the search uses is no smaller."""
    from hcir.gallery import ResidentGallery
    from oracle import refine as orf
    q, g = _bound_family(family, planted)
    assert g.shape[0] <= 640
    gal = ResidentGallery(torch.from_numpy(g).cuda())
    qd = torch.from_numpy(q).cuda()
    q16 = qd.half()
    mirror = gal.mirror.cpu().numpy()
    assert np.array_equal(mirror, g.astype(np.float16)) and np.array_equal(q16.cpu().numpy(), q.astype(np.float16))
    s16 = _mirror_scores(q16, gal.mirror)
    chain = oknn.scores(q, g)
    e64, c64 = orf.err_bound64(q, g, mirror)
    diff = np.abs(chain.astype(np.float64) - s16.astype(np.float64))
    ratio = (diff / e64[:, None]).max()
    BOUND_ROWS.append(f"refine-bound {family:16s} nq {q.shape[0]:3d} ng {g.shape[0]:4d} d {g.shape[1]:5d}  "
                      f"max |diff| / E64 {ratio:.4f}  E64 {e64.min():.3e} .. {e64.max():.3e}")
    assert np.isfinite(s16).all()
    assert (diff <= e64[:, None]).all(), ratio
    used = gal.err_bound(qd, q16).cpu().numpy().astype(np.float64)
    assert (e64 <= used).all()
    # the four constants of the mirror: any-order fp32 summation of non-negative terms and the root
    rel = (g.shape[1] + 2) * 2.0 ** -24
    for name, got, want in zip(("eg", "g16max", "g32max", "gamma"), (gal._eg, gal._g16max, gal._g32max, gal._gamma), c64):
        assert abs(got - want) <= rel * want, (name, got, want)
    assert [np.float32(c) for c in gal._consts] == [np.float32(c) for c in (gal._eg, gal._g16max, gal._g32max, gal._gamma)]


@pytest.mark.parametrize("kind", ["query", "gallery"])
def test_planted_gallery_is_not_certified_and_exact(kind, planted):
    """A kernel whose E_i lacks the ||q - q~|| g16max term (kind "query") or the ||q|| eg term ("gallery") certifies
    the planted query and returns the neutral row in place of the true 5th neighbour (oracle.refine.plant)."""
    from hcir import ops
    from hcir.gallery import FILTER_KC, ResidentGallery
    from oracle import refine as orf
    p = planted[kind]
    f = orf.plant_facts(p)
    assert all(f["holds"].values()), f["holds"]
    i, k = orf.PLANTED_QUERY, orf.PLANT_K
    gal = ResidentGallery(torch.from_numpy(p["g"]).cuda(), idx_base=7)
    qd = torch.from_numpy(p["q"]).cuda()
    cval, cidx = ops.sim_topk(qd.half(), gal.mirror, FILTER_KC)
    cidx, cval = cidx.cpu().numpy()[i], cval.cpu().numpy()[i]
    assert np.array_equal(np.sort(cidx), p["filter16"]) and p["a"] not in cidx          # the filter misses row A
    assert abs(float(cval[-1]) - f["t"]) < 1e-6 and cval[-1] + f["e_mut"] < f["vk"] <= cval[-1] + f["e64"]
    pending = gal.search_begin(qd, k)
    assert pending.cert is not None and int(pending.cert[i]) == 0, "the planted query was certified"
    val, idx = pending.finish()
    rv, ri = oknn.cosine_topk(p["q"], p["g"], k, idx_base=7)
    assert ri[i, k - 1] == p["a"] + 7
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)
    assert gal.stats["fallback_queries"] >= 1


def test_mirror_overflow_falls_back():
    """one finite element above the fp16 range: the mirror holds an inf, E_i is not finite, no query is certified"""
    from hcir.gallery import ResidentGallery
    q, g = _unit((9, 64), 31), _unit((3000, 64), 32)
    g[1234, 5] = 70000.0
    gal = ResidentGallery(torch.from_numpy(g).cuda())
    assert torch.isinf(gal.mirror[1234, 5])
    val, idx = gal.search(torch.from_numpy(q).cuda(), 5)
    rv, ri = oknn.cosine_topk(q, g, 5)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)
    assert gal.stats["queries"] == 9 and gal.stats["fallback_queries"] == 9


def test_mirror_dtype():
    """the kernel's E_i is that of an fp16 rounding: any other mirror is refused; no mirror searches exactly"""
    from hcir import HcirError
    from hcir.gallery import ResidentGallery
    q, g = _unit((5, 64), 33), _unit((500, 64), 34)
    gd = torch.from_numpy(g).cuda()
    for dt in (torch.bfloat16, torch.float32, torch.float64):
        with pytest.raises(HcirError):
            ResidentGallery(gd, mirror=dt)
    gal = ResidentGallery(gd, mirror=None)
    assert gal.mirror is None
    val, idx = gal.search(torch.from_numpy(q).cuda(), 5)
    rv, ri = oknn.cosine_topk(q, g, 5)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)
