"""oracle.head_loss and oracle.transform.positive_transform_f64, which tests/test_head_loss_elements_gpu.py and
tests/test_train_default_path_gpu.py hold the head, loss, normalise, convert and rotate-blur kernels to.  No GPU.

Honest: the fp32 emulation of every reduction order stays inside every bound, on every family and shape the GPU tests
run, over three seeds.  Sharp: every entry of oracle.head_loss.MISTAKES, applied to the float64 chain and put through
the same checks, exceeds a bound 10-fold (a dropped row also breaks the exact integer sums and a hot-row probe).  The
rotation oracle: positions with a nonzero slack stay below 0.5 % in every case of the GPU test, and the float64
reference agrees with the older fp32 one everywhere inside its bound.  Last, the pitch checks of hcir_bn1d_fwd / _bwd:
refused on the host, before any launch.  Both tables are printed (pytest -s; profiles/head_loss_bounds.txt keeps a copy)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import head_loss as oh
from oracle import transform as otf

SEEDS = (0, 1, 2)
HCIR_ERR_INVALID = -1
BN_MODES = [(True, None, True), (False, 3.0, False), (True, 2.0 ** -7, False), (False, None, False)]   # relu, scale, mask
ROT_CASES = [(a, s, shape) for a, s in [(0.0, 0.3), (11.25, 0.1), (-14.9, 0.5), (7.0, 0.27), (15.0, 0.3), (-15.0, 0.2)]
             for shape in [(3, 3, 224, 224), (2, 1, 65, 40), (2, 2, 33, 47), (1, 1, 2, 2)]]
ROWS = []


@pytest.fixture(scope="module")
def table():
    yield ROWS
    print("\nhead-loss-emu: fp32 emulation of the kernels' order, worst err / bound per kernel, shape and family")
    for r in ROWS:
        print(r)


def _note(kernel, shape, family, w, limit=1.0):
    figures = "  ".join(f"{k} {v:.3f}" for k, v in w.items() if "=" not in k)                  # equalities: 0 or a failure
    ROWS.append(f"head-loss-emu {kernel:8s} {str(shape):14s} {family:14s} {figures}")
    assert all(v <= limit for v in w.values()), (kernel, shape, family, w)


def _worst(into, w):
    for k, v in w.items():
        into[k] = max(into.get(k, 0.0), v)


# ---------------------------------------------------------------------------------------------------------------
# honest
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", oh.BN_SHAPES, ids=str)
def test_bn1d_emulation_within_every_bound(shape, table):
    rows, f = shape
    for family in oh.FAMILIES:
        worst = {}
        for seed in SEEDS:
            prob = oh.make_bn1d(family, rows, f, seed=seed + rows + f)
            for relu, scale, mask in BN_MODES:
                _worst(worst, oh.check_bn1d(prob, relu, oh.emulate_bn1d(prob, relu, scale, mask), scale, mask))
        _note("bn1d", shape, family, worst)


def test_bn1d_shapes_reach_the_branches():
    fs, rs = {f for _, f in oh.BN_SHAPES}, {r for r, _ in oh.BN_SHAPES}
    assert fs == {1, 64, 65, 100, 192, 768} and rs == {1, 2, 3, 4, 5, 9, 258, 1023}
    assert len(oh.BN_SHAPES) == 12 and {m[1] for m in BN_MODES} == set(oh.BN_SCALES)
    # one column, exactly one workgroup, one live column in the last, a ragged last, three workgroups, the head's width
    assert [oh.cdiv(f, oh.BN_COLS) for f in (1, 64, 65, 100, 192, 768)] == [1, 1, 2, 2, 3, 12] and 65 % 64 == 1
    assert {r % 4 for r in rs} == {0, 1, 2, 3} and oh.bn_depth(1023) == 259 and oh.bn_depth(1) == 4


@pytest.mark.parametrize("shape", oh.TRIPLET_SHAPES, ids=str)
def test_triplet_emulation_within_every_bound(shape, table):
    b, d = shape
    for family in ("normal", "large_mean", "scaled"):
        worst = {}
        for seed in SEEDS:
            a, p, n = oh.make_triplet(family, b, d, seed=seed + b + d)
            for margin in oh.MARGINS:
                _worst(worst, oh.check_triplet(a, p, n, margin, oh.emulate_triplet(a, p, n, margin)))
        _note("triplet", shape, family, worst)


@pytest.mark.parametrize("n", oh.MSE_SIZES)
def test_mse_emulation_within_every_bound(n, table):
    assert (oh.mse_trips(n) == 17 and oh.mse_blocks(n) == 256 and n % 256) if n > 256 * 4096 else oh.mse_trips(n) <= 16
    for family in ("normal", "large_mean", "scaled"):
        worst = {}
        for seed in SEEDS:
            x, y = (t.flatten() for t in oh.make_rows(family, 1, n, seed=seed + n % 977, count=2))
            _worst(worst, oh.check_mse(x, y, oh.emulate_mse(x, y)))
        _note("mse", n, family, worst)


@pytest.mark.parametrize("shape", oh.L2_SHAPES, ids=str)
def test_l2_emulation_within_every_bound(shape, table):
    worst = {}
    for seed in SEEDS:
        x = oh.make_l2(*shape, seed=seed + shape[1])
        _worst(worst, oh.check_l2(x, oh.emulate_l2(x)))
        s = (x.double() ** 2).sum(1)
        assert float(s.max()) < 3e38 and bool((s[s > 0] > 2.0 ** -100).all())             # inside the fp32 range
        assert (x[0] != 0).any() and (shape[0] < 2 or (x[-1] == 0).all())
        assert shape[0] < 3 or 0 < float(x[-2].double().norm()) < oh.L2_EPS
    _note("l2", shape, "special rows", worst)


def test_convert_input_holds_the_special_values():
    for n in oh.CONVERT_SIZES:
        x = oh.convert_input(n)
        assert x.numel() == n and x.dtype == torch.float32
    x = oh.convert_input(1023)
    h = x.half()
    assert torch.isnan(x).any() and torch.isinf(x).any() and (torch.isinf(h) & ~torch.isinf(x)).any()
    assert ((h != 0) & (h.abs() < 2.0 ** -14)).any() and (x[:2] == 0).all() and torch.signbit(x[1])
    assert 1023 % 4 == 3 and float(x[-1]) == 65520.0 and float(h[-1]) == float("inf")      # a tie in the scalar tail
    assert float(x[-2]) == 3 * 2.0 ** -25 and float(h[-2]) == 2.0 ** -23                   # a subnormal tie, to even
    assert float(x[14]) == 1 + 2.0 ** -11 and float(h[14]) == 1.0 and float(h[15]) == 1 + 2.0 ** -9


# ---------------------------------------------------------------------------------------------------------------
# sharp
# ---------------------------------------------------------------------------------------------------------------
def _exact_ok(rows, f, mistake):
    """the exact integer sums and the hot-row probes of the GPU test, on the float64 chain"""
    base = oh.exact_bn1d(rows, f)
    for y16 in (None, base["y16"]):
        out = oh.chain_bn1d(base, False, mistake=mistake, given=(base["mean"], base["rstd"], y16))
        g = base["dy"].double() * (1 if y16 is None else (y16 > 0))
        if not (torch.equal(out["dbeta"], g.sum(0)) and torch.equal(out["dgamma"], (g * base["x"].double()).sum(0))):
            return False
    for r in oh.hot_rows(rows):
        dy = torch.zeros(rows, f)
        dy[r] = base["dy"][r]
        out = oh.chain_bn1d(dict(base, dy=dy), False, mistake=mistake, given=(base["mean"], base["rstd"], None))
        if not (torch.equal(out["dbeta"], dy[r].double()) and torch.equal(out["dgamma"], (dy[r] * base["x"][r]).double())):
            return False
    return True


def _mistake_factor(mistake):
    if mistake.startswith("bn1d"):
        rows, f = (1023, 100) if mistake in (oh.LOST, oh.LASTBLOCK) else (9, 100)
        prob = oh.make_bn1d("random_buffers", rows, f, seed=3)
        relu, scale, mask = True, 3.0, True
        ref = oh.check_bn1d(prob, relu, oh.chain_bn1d(prob, relu, scale, mask), scale, mask)
        assert max(ref.values()) <= 1.0, ref
        w = oh.check_bn1d(prob, relu, oh.chain_bn1d(prob, relu, scale, mask, mistake), scale, mask, truth=False)
    elif mistake.startswith("triplet"):
        a, p, n = oh.make_triplet("normal", 5, 65, seed=3)
        assert max(oh.check_triplet(a, p, n, oh.MARGINS[0], oh.chain_triplet(a, p, n, oh.MARGINS[0])).values()) <= 1.0
        w = oh.check_triplet(a, p, n, oh.MARGINS[0], oh.chain_triplet(a, p, n, oh.MARGINS[0], mistake=mistake))
    elif mistake.startswith("mse"):
        w = {}
        for n in oh.MSE_SIZES[1:]:
            x, y = (t.flatten() for t in oh.make_rows("normal", 1, n, seed=3, count=2))
            assert max(oh.check_mse(x, y, oh.chain_mse(x, y)).values()) <= 1.0
            w[n] = max(oh.check_mse(x, y, oh.chain_mse(x, y, mistake=mistake)).values())
        assert min(w.values()) > 1.0, w                 # seen at every size, the largest included
    else:
        x = oh.make_l2(7, 260, seed=3)
        assert max(oh.check_l2(x, oh.chain_l2(x)).values()) <= 1.0
        w = oh.check_l2(x, oh.chain_l2(x, mistake=mistake))
    return max(w.values())


def test_every_mistake_exceeds_a_bound():
    assert len(oh.MISTAKES) == 9 and len(set(oh.MISTAKES)) == 9
    print("\nhead-loss-mut: kernel mistakes applied to the float64 chain, largest err / bound")
    for mistake in oh.MISTAKES:
        factor = _mistake_factor(mistake)
        print(f"head-loss-mut  {mistake:75s} {factor:.3g}")
        assert factor >= 10.0, (mistake, factor)
    assert _exact_ok(1023, 100, None) and _exact_ok(5, 65, None)
    assert not _exact_ok(1023, 100, oh.LOST) and not _exact_ok(5, 65, oh.LOST)
    assert not _exact_ok(1023, 100, oh.LASTBLOCK)


def test_references_agree_with_torch_in_float64():
    """the chains against torch's own float64 modules and autograd"""
    prob = oh.make_bn1d("random_buffers", 9, 100, seed=4)
    for relu in (True, False):
        ref = oh.chain_bn1d(prob, relu, None, relu)
        t = oh.truth_f64(prob["x"], prob["dy"], prob["gamma"], prob["beta"], relu, (ref["y16"].half() > 0) if relu else None,
                         None)
        assert (t["y"][0] - ref["y16"]).abs().max() <= 1e-5 and (t["dx"][0] - ref["dx"]).abs().max() <= 1e-5
    rm, rv = prob["rm"].double().clone(), prob["rv"].double().clone()
    F.batch_norm(prob["x"].double(), rm, rv, None, None, True, oh.MOMENTUM, oh.EPS)
    assert (rm - ref["running_mean"]).abs().max() <= 1e-6 and (rv - ref["running_var"]).abs().max() <= 1e-6
    a, p, n = (t.double().requires_grad_(True) for t in oh.make_triplet("normal", 5, 65, seed=4))
    loss = F.triplet_margin_loss(a, p, n, margin=oh.MARGINS[0], p=2, eps=oh.TRIPLET_EPS)
    (oh.TRIPLET_GRAD * loss).backward()
    ref = oh.chain_triplet(a.detach(), p.detach(), n.detach(), oh.MARGINS[0])
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-7 and (ref["row_loss"] > 0).any() and (ref["row_loss"] == 0).any()
    for name, t in (("da", a), ("dp", p), ("dn", n)):
        assert (ref[name] - t.grad).abs().max() <= 1e-6, name
    x, y = (t.flatten().double() for t in oh.make_rows("normal", 1, 257, seed=4, count=2))
    xr = x.clone().requires_grad_(True)
    loss = F.mse_loss(xr, y)
    (oh.MSE_GRAD * loss).backward()
    ref = oh.chain_mse(x, y)
    assert abs(float(loss.detach() - ref["loss"])) <= 1e-12 and (xr.grad - ref["dx"]).abs().max() <= 1e-12
    x = oh.make_l2(7, 260, seed=4)
    assert (F.normalize(x.double(), dim=1, eps=oh.L2_EPS) - oh.chain_l2(x)["y32"]).abs().max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------
# the rotation oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle,sigma,shape", ROT_CASES, ids=str)
def test_rotation_reference_slack_share_and_agreement(angle, sigma, shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    ref, bound, share = otf.positive_transform_f64(x, angle, sigma)
    assert share <= 5e-3, share                 # not vacuous: the bound is the rounding term on 99.5 % of the positions
    assert (bound > 0).all() and oh.ratio(otf.positive_transform(x, angle, sigma), ref, bound) <= 1.0
    if angle == 0.0:
        assert share == 0.0
    xm = otf.marked_image(shape)
    refm, boundm, sharem = otf.positive_transform_f64(xm, angle, sigma)
    assert sharem <= 5e-3 and oh.ratio(otf.positive_transform(xm, angle, sigma), refm, boundm) <= 1.0


def test_rotation_reference_sees_a_replicated_border():
    """replicate instead of reflect padding on the marked image: far outside the bound"""
    shape, angle, sigma = (2, 1, 65, 40), 7.0, 0.27
    xm = otf.marked_image(shape)
    ref, bound, _ = otf.positive_transform_f64(xm, angle, sigma)
    k = torch.exp(-0.5 * (torch.linspace(-1, 1, 3) / sigma) ** 2)
    k2 = torch.outer(k / k.sum(), k / k.sum()).double().expand(1, 1, 3, 3)
    # the rotated image alone: the older reference with a delta blur (the taps of sigma = 1e-3 are 0, 1, 0)
    rot = otf.positive_transform(xm, angle, 1e-3).double()
    assert oh.ratio(F.conv2d(F.pad(rot, [1, 1, 1, 1], mode="reflect"), k2), ref, bound) <= 1.0
    assert oh.ratio(F.conv2d(F.pad(rot, [1, 1, 1, 1], mode="replicate"), k2), ref, bound) >= 10.0
    assert otf.rot_delta(256, 256) == 2.0 ** -12 and otf.rot_delta(224, 224) == 2.0 ** -12
    assert otf.rot_delta(1024, 512) == 2.0 ** -10 and otf.rot_delta(342, 2) == 2.0 ** -11


# ---------------------------------------------------------------------------------------------------------------
# hcir_bn1d_fwd / _bwd: a pitch below f is refused on the host
# ---------------------------------------------------------------------------------------------------------------
def _fwd(L, f, ldx, ld32, ld16, y32=True, y16=True):
    p = ctypes.c_void_p(16)      # never read: every call below is refused before a launch
    return L.hcir_bn1d_fwd(p, ldx, 8, f, p, p, 1e-5, 0.1, 1, None, None, p, p, p if y32 else None, ld32,
                           p if y16 else None, ld16, None)


def _bwd(L, f, lddy, ldx, ldr, lddx, relu=True):
    p = ctypes.c_void_p(16)
    return L.hcir_bn1d_bwd(p, lddy, p, ldx, 8, f, p, p, p, p if relu else None, ldr, None, p, lddx, p, p, None)


def test_bn1d_refuses_a_pitch_below_f(hcir_built):
    L = hcir_built
    f = 100
    for bad in (f - 1, 0, -f):
        assert _fwd(L, f, bad, f, f) == HCIR_ERR_INVALID
        assert _fwd(L, f, f, bad, f) == HCIR_ERR_INVALID
        assert _fwd(L, f, f, f, bad) == HCIR_ERR_INVALID
        assert _fwd(L, f, f, bad, f, y16=False) == HCIR_ERR_INVALID
        assert _fwd(L, f, f, f, bad, y32=False) == HCIR_ERR_INVALID
        assert _bwd(L, f, bad, f, f, f) == HCIR_ERR_INVALID
        assert _bwd(L, f, f, bad, f, f) == HCIR_ERR_INVALID
        assert _bwd(L, f, f, f, bad, f) == HCIR_ERR_INVALID
        assert _bwd(L, f, f, f, f, bad) == HCIR_ERR_INVALID
        assert _bwd(L, f, f, f, f, bad, relu=False) == HCIR_ERR_INVALID
    # the arguments refused before this change still are
    assert _fwd(L, 0, f, f, f) == HCIR_ERR_INVALID and _fwd(L, f, f, f, f, y32=False, y16=False) == HCIR_ERR_INVALID
    assert _bwd(L, 0, f, f, f, f) == HCIR_ERR_INVALID
