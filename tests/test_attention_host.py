"""CPU-only: the attention error bounds of oracle.attention are honest and sharp.

Honest: the plain-torch emulations of the kernels' arithmetic (one per kernel family: MFMA forward, MFMA backward,
class-token forward, class-token backward) stay inside the bounds on every input family of tests/test_attention_gpu.py
(max err / bound <= 1).  Sharp: each listed kernel mistake, applied to the float64 reference, exceeds the bound by at
least 10x on at least one family, over the elements the mistake touches.  The table of (mistake, family) factors is
printed (pytest -s).  Families that cannot show a mistake, by construction:
  uniform (K = 0)   every mistake that only moves scores (scale, swapped V rows - the mean is symmetric -, Q / K tile
                    swap leaves S = 0 only partly) and lse-without-maximum (the maximum is 0);
  flat              a dropped or duplicated key is a 1 / T effect on an output of size |v| / sqrt(T): 1 - 5 x the bound,
                    which is why the marker families exist;
  T a multiple of 32: no pad keys and no pad query rows, the pad mistakes do not exist (factor 0).
"""
import functools
import math

import pytest
import torch

from oracle import attention as oa

HD = 64
SCALE = oa.f32(HD ** -0.5)
SHAPES = [(1, 197, 2), (2, 17, 3)]       # (b, t, h): seven key tiles with a ragged last one; one tile
CLS_SHAPES = [(1, 197, 2), (3, 5, 2)]
CLS_FAMILIES = ("flat", "marker_last", "negdom", "sharp")


@functools.lru_cache(maxsize=None)
def problem(family, shape, hd=HD):
    b, t, h = shape
    scale = oa.f32(hd ** -0.5)
    qkv = oa.make_qkv(family, b, t, h, hd)
    dout = oa.make_dout(b, t, h, hd)
    ref = oa.attention_f64(qkv, b, t, h, hd, scale, dout)
    bo, bl = oa.fwd_bounds(ref)
    return qkv, dout, ref, bo, bl, oa.bwd_bounds(ref, bo, bl)


@functools.lru_cache(maxsize=None)
def cls_problem(family, shape):
    b, t, h = shape
    qkv = oa.make_qkv(family, b, t, h, HD)
    dout = oa.make_dout(b, 1, h, HD)
    ref = oa.attention_f64(qkv, b, t, h, HD, SCALE, dout, nq=1)
    bo, bl = oa.fwd_bounds(ref, "cls")
    return qkv, dout, ref, bo, bl, oa.bwd_bounds(ref, bo, bl, "cls")


# ---------------------------------------------------------------------------------------------------------------
# (a) the emulations stay inside the bounds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(1, 225, 1), (1, 1, 2)], ids=str)
@pytest.mark.parametrize("family", oa.FAMILIES)
def test_mfma_emulation_within_bounds(family, shape):
    b, t, h = shape
    qkv, dout, ref, bo, bl, (bdq, bdk, bdv) = problem(family, shape)
    out, lse = oa.emulate_fwd(qkv, b, t, h, HD, SCALE)
    dqkv = oa.emulate_bwd(qkv, out, dout, lse, b, t, h, HD, SCALE).double().permute(2, 0, 3, 1, 4)
    r = {"o": oa.ratio(oa.heads_of(out, b, t, h, HD), ref.o, bo), "lse": oa.ratio(lse, ref.lse2, bl),
         "dq": oa.ratio(dqkv[0], ref.dq, bdq), "dk": oa.ratio(dqkv[1], ref.dk, bdk),
         "dv": oa.ratio(dqkv[2], ref.dv, bdv)}
    print(f"\nattention emulation {family} {shape}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("hd,shape", [(80, (1, 50, 2)), (32, (1, 129, 1)), (128, (1, 17, 2))], ids=str)
@pytest.mark.parametrize("family", ("flat", "uniform"))
def test_generic_head_dim_emulation_within_bounds(family, hd, shape):
    b, t, h = shape
    qkv, _, ref, bo, _, _ = problem(family, shape, hd)
    for nq in (1, t):
        out, _ = oa.emulate_fwd(qkv, b, t, h, hd, oa.f32(hd ** -0.5), nq)
        r = oa.ratio(oa.heads_of(out, b, nq, h, hd), ref.o[:, :, :nq], bo[:, :, :nq])
        print(f"\nattention emulation hd {hd} {family} {shape} nq {nq}: o {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("shape", CLS_SHAPES + [(1, 1, 1), (2, 64, 1), (1, 256, 1)], ids=str)
@pytest.mark.parametrize("family", CLS_FAMILIES)
def test_cls_emulation_within_bounds(family, shape):
    b, t, h = shape
    qkv, dout, ref, bo, bl, (bdq, bdk, bdv) = cls_problem(family, shape)
    out, lse = oa.emulate_cls_fwd(qkv, b, t, h, HD, SCALE)
    dqkv = oa.emulate_cls_bwd(qkv, out, dout, lse, b, t, h, HD, SCALE).double().permute(2, 0, 3, 1, 4)
    r = {"o": oa.ratio(oa.heads_of(out, b, 1, h, HD), ref.o, bo), "lse": oa.ratio(lse[..., None], ref.lse2, bl),
         "dq": oa.ratio(dqkv[0][:, :, :1], ref.dq, bdq), "dk": oa.ratio(dqkv[1], ref.dk, bdk),
         "dv": oa.ratio(dqkv[2], ref.dv, bdv)}
    print(f"\nattention cls emulation {family} {shape}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    assert not dqkv[0][:, :, 1:].any()
    # the class-token row of the MFMA forward agrees with it within the sum of the two bounds
    full = oa.attention_f64(qkv, b, t, h, HD, SCALE)
    fo, fl = oa.fwd_bounds(full)
    mo, ml = oa.emulate_fwd(qkv, b, t, h, HD, SCALE, nq=1)
    assert oa.ratio(oa.heads_of(mo, b, 1, h, HD), oa.heads_of(out, b, 1, h, HD), bo + fo[:, :, :1]) <= 1.0
    assert oa.ratio(ml, lse[..., None].double(), bl + fl[:, :, :1]) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# (b) mistakes, applied to the float64 reference
# ---------------------------------------------------------------------------------------------------------------
def _pad(x, rows):
    return torch.cat([x, rows], 2)


def fwd_mistakes(ref, t):
    """name -> (o, lse2) of the mistaken computation; None where the mistake leaves that output alone."""
    q, k, v, sc = ref.q, ref.k, ref.v, ref.scale
    npad = 32 * ((t + 31) // 32) - t
    run = lambda q_, k_, v_, s_=sc: (lambda r: (r.o, r.lse2))(oa.core_f64(q_, k_, v_, s_))
    out = {}
    if npad:
        out["pad keys unmasked (copies of key t-1)"] = run(q, _pad(k, k[:, :, -1:].expand(-1, -1, npad, -1)),
                                                           _pad(v, v[:, :, -1:].expand(-1, -1, npad, -1)))
        zero = torch.zeros_like(k[:, :, :1]).expand(-1, -1, npad, -1)
        out["pad keys unmasked (zero rows)"] = run(q, _pad(k, zero), _pad(v, zero))
    if t > 1:
        out["last key dropped"] = run(q, k[:, :, :-1], v[:, :, :-1])
        out["first key dropped"] = run(q, k[:, :, 1:], v[:, :, 1:])
    if t >= 4:
        v2 = v.clone()
        v2[:, :, 2], v2[:, :, 3] = v[:, :, 3], v[:, :, 2]
        out["V rows 2 and 3 swapped"] = run(q, k, v2)
    n = min(32, t)
    out["Q and K rows of tile 0 swapped"] = run(torch.cat([k[:, :, :n], q[:, :, n:]], 2),
                                                torch.cat([q[:, :, :n], k[:, :, n:]], 2), v)
    out["scale off by 1 %"] = run(q, k, v, sc * 1.01)
    out["natural-log lse"] = (None, ref.lse2 * oa.LN2)
    out["lse without the row maximum"] = (None, ref.lse2 - ref.s.max(-1).values * oa.LOG2E)
    half = ((torch.arange(t) % 8) < 4).double()
    part = (ref.p * half).sum(-1)
    out["row sum over one half-wave's keys"] = (ref.o / part[..., None], ref.lse2 + torch.log2(part))
    return out


def bwd_mistakes(ref, t):
    """name -> {"dq" | "dk" | "dv": (mistaken tensor, row slice of the touched elements)}"""
    q, k, v, sc, do = ref.q, ref.k, ref.v, ref.scale, ref.do
    hd = q.shape[-1]
    every = slice(None)
    out = {}
    d4 = (do[..., :hd - 4] * ref.o[..., :hd - 4]).sum(-1)
    ds4 = ref.p * (ref.dp - d4[..., None])
    out["D missing four head dims"] = {"dq": (sc * (ds4 @ k), every), "dk": (sc * (ds4.transpose(-1, -2) @ q), every)}
    lo = 32 if t > 32 else 0
    out["dQ missing one 32-key slab"] = {"dq": (ref.dq - sc * (ref.ds[..., lo:lo + 32] @ k[:, :, lo:lo + 32]), every)}
    last = slice(t - 1, t)
    out["dK of the last live key zero"] = {"dk": (torch.zeros_like(ref.dk), last)}
    out["dV of the last live key zero"] = {"dv": (torch.zeros_like(ref.dv), last)}
    out["dK without scale"] = {"dk": (ref.dk / sc, every)}
    npad = 32 * ((t + 31) // 32) - t
    if npad:   # pad query rows behave as copies of row t-1 (its lse, its dO)
        out["dO rows past T not zeroed"] = {
            "dk": (ref.dk + npad * sc * ref.ds[:, :, -1:].transpose(-1, -2) * q[:, :, -1:], every),
            "dv": (ref.dv + npad * ref.p[:, :, -1:].transpose(-1, -2) * do[:, :, -1:], every)}
    return out


def _table(title, rows):
    print(f"\n{title}")
    for name, per in rows.items():
        print(f"  {name:42s} " + "  ".join(f"{fam} {val:.3g}" for fam, val in per.items()))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_mistakes_exceed_bounds_tenfold(shape):
    b, t, h = shape
    rows = {}
    for fam in oa.FAMILIES:
        _, _, ref, bo, bl, _ = problem(fam, shape)
        for name, (o, lse) in fwd_mistakes(ref, t).items():
            f = 0.0
            if o is not None:
                f = max(f, oa.ratio(o, ref.o, bo))
            if lse is not None:
                f = max(f, oa.ratio(lse, ref.lse2, bl))
            rows.setdefault(name, {})[fam] = f
    _table(f"forward mistakes, max err / bound, {shape}", rows)
    assert all(max(per.values()) >= 10.0 for per in rows.values()), rows
    # the forward WITHOUT lse sees the output alone: every mistake that moves o reaches 10x through o too
    rows_o = {}
    for fam in oa.FAMILIES:
        _, _, ref, bo, _, _ = problem(fam, shape)
        for name, (o, _) in fwd_mistakes(ref, t).items():
            if o is not None:
                rows_o.setdefault(name, {})[fam] = oa.ratio(o, ref.o, bo)
    _table(f"forward mistakes, o alone, {shape}", rows_o)
    assert all(max(per.values()) >= 10.0 for per in rows_o.values()), rows_o


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_mistakes_exceed_bounds_tenfold(shape):
    b, t, h = shape
    rows = {}
    for fam in oa.FAMILIES:
        _, _, ref, bo, bl, (bdq, bdk, bdv) = problem(fam, shape)
        truth = {"dq": (ref.dq, bdq), "dk": (ref.dk, bdk), "dv": (ref.dv, bdv)}
        for name, touched in bwd_mistakes(ref, t).items():
            f = 0.0
            for key, (mut, sl) in touched.items():
                f = max(f, oa.ratio(mut[:, :, sl], truth[key][0][:, :, sl], truth[key][1][:, :, sl]))
            rows.setdefault(name, {})[fam] = f
    _table(f"backward mistakes, max err / bound, {shape}", rows)
    assert all(max(per.values()) >= 10.0 for per in rows.values()), rows


@pytest.mark.parametrize("shape", CLS_SHAPES, ids=str)
def test_cls_mistakes_exceed_bounds_tenfold(shape):
    b, t, h = shape
    rows = {}
    for fam in CLS_FAMILIES:
        qkv, dout, ref, bo, bl, (bdq, bdk, bdv) = cls_problem(fam, shape)
        n_empty = 256 - t
        s_sum = 1.0 / ref.p.max(-1).values               # the row sum in units where the maximum is 1
        if n_empty:
            f = max(oa.ratio(ref.o * (s_sum / (s_sum + n_empty))[..., None], ref.o, bo),
                    oa.ratio(ref.lse2 + torch.log2((s_sum + n_empty) / s_sum), ref.lse2, bl))
            rows.setdefault("lanes without a key add exp2(0)", {})[fam] = f
        wrong = oa.core_f64(ref.q.roll(1, dims=1), ref.k, ref.v, ref.scale, ref.do)
        rows.setdefault("token 0's q from the wrong head (forward)", {})[fam] = max(
            oa.ratio(wrong.o, ref.o, bo), oa.ratio(wrong.lse2, ref.lse2, bl))
        rows.setdefault("token 0's q from the wrong head (backward)", {})[fam] = max(
            oa.ratio(wrong.dq, ref.dq, bdq), oa.ratio(wrong.dk, ref.dk, bdk), oa.ratio(wrong.dv, ref.dv, bdv))
        for name, sl in (("last key dropped", slice(0, t - 1)), ("first key dropped", slice(1, t))):
            part = oa.core_f64(ref.q, ref.k[:, :, sl], ref.v[:, :, sl], ref.scale)
            rows.setdefault(name, {})[fam] = max(oa.ratio(part.o, ref.o, bo), oa.ratio(part.lse2, ref.lse2, bl))
    _table(f"class-token mistakes, max err / bound, {shape}", rows)
    assert all(max(per.values()) >= 10.0 for per in rows.values()), rows


def test_reference_pieces_are_consistent():
    """attention_f64's closed-form gradients equal float64 autograd's; the uniform family is exact; the dS = 0 case."""
    b, t, h = 1, 37, 2
    qkv = oa.make_qkv("sharp", b, t, h, HD)
    dout = oa.make_dout(b, t, h, HD)
    ref = oa.attention_f64(qkv, b, t, h, HD, SCALE, dout)
    q, k, v = [x.clone().requires_grad_(True) for x in oa.split_qkv(qkv, b, t, h, HD)]
    o = torch.softmax(SCALE * (q @ k.transpose(-1, -2)), -1) @ v
    o.backward(oa.heads_of(dout, b, t, h, HD))
    assert (o - ref.o).abs().max() <= 1e-14
    for got, want in ((ref.dq, q.grad), (ref.dk, k.grad), (ref.dv, v.grad)):
        assert (got - want).abs().max() <= 1e-13 * max(1.0, float(want.abs().max()))
    assert torch.allclose(ref.lse2 * oa.LN2, torch.logsumexp(ref.s, -1), atol=1e-13)
    assert torch.allclose(ref.p.sum(-1), torch.ones_like(ref.lse2), atol=1e-14)
    for tt in (1, 17, 197):
        qkv = oa.make_qkv("uniform", 1, tt, 2, HD)
        assert torch.equal(qkv.float().double(), qkv.double()) and not qkv[:, :, 1].any()
        dout = torch.zeros(1, tt, 2 * HD)
        dout.view(1, tt, 2, HD)[..., :4] = torch.tensor([0.5, -0.25, 1.0, 0.125])
        r = oa.attention_f64(qkv, 1, tt, 2, HD, SCALE, dout.half())
        assert torch.equal(r.p, torch.full_like(r.p, 1.0 / tt)) and (r.o - r.v.mean(2, keepdim=True)).abs().max() < 1e-14
        assert r.ds.abs().max() <= 1e-16 and r.dq.abs().max() <= 1e-15 and r.dk.abs().max() <= 1e-15
        assert (r.dv - oa.heads_of(dout, 1, tt, 2, HD) * 1.0).abs().max() <= 1e-14   # sum_i dout_i / t = dout
    assert math.isclose(oa.f32(0.125), 0.125)
