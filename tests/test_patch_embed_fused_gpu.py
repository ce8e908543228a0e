"""GPU: hcir_patch_embed_fused (persistent 256 x 256 patch embedding with LayerNorm statistics), every element of
every token row against float64 through a per-element bound built as oracle/gemm.py::epilogue_f64 builds its fp16
bounds (err / bound <= 1), the per-slice statistics of every stored row against oracle.gemm.slice_stats_f64 and the
hcir_ln_stats_finalize result against finalize_f64.

Reference   S, A = sums of the fp16-rounded patches times the fp16 weights (oracle.gemm.acc_f64 on the im2col'ed
            operands), x = S + bias, y = x + pos_mult pos[1 + pi];   class rows: y = cls + pos_mult pos[0].
Bound       patch rows: K u A (MFMA accumulation) + u|x| (the bias add) + u|y| (the one fma that adds pos_mult pos; the
            product is not rounded) + h|y| + z (the one fp16 store), times (1 + 2^-9);
            class rows: u|y| + h|y| + z (one fma, one store).
The bound was written before the first GPU run and has not been changed since.  Worst err / bound on an MI355X
(profiles/patch_embed_bounds.txt): see that file; the fp16 store's half ulp is nearly all of the bound, so a
correctly rounded store reaches ~0.99.

Shapes (d = 768, P = 16, 224 x 224 unless stated), each a distinct edge of the tile engine:
  b1          196 rows: one ragged tile
  b3          588 rows: image boundaries inside tiles 0 and 1, ragged last tile, pos_mult = 2
  b4          784 rows: the last tile holds 16 rows - three of its four m-waves lie wholly past M
  b50-32x48   np = 6, 300 rows: 43 image boundaries per tile (the row remap)
  d1024-b2    4 n-tiles
Token buffers are prefilled with a finite sentinel between two guard rows: every token row (class rows included) must
be overwritten - a row left at the sentinel fails its bound - and the guards must come back bit-equal.
"""
import pytest
import torch

from oracle import gemm as og

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
F32, F16 = 0, 1
TILE128, BIG = 0, 1
SENT = -7.25
WORST = {}

# name -> (b, h, w, d, pos_mult)
CASES = {
    "b1": (1, 224, 224, 768, 1.0),
    "b3": (3, 224, 224, 768, 2.0),
    "b4": (4, 224, 224, 768, 1.0),
    "b50-32x48": (50, 32, 48, 768, 1.0),
    "d1024-b2": (2, 224, 224, 1024, 1.0),
}


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    yield hcir_built
    print("\npatch embed worst err / bound per case:")
    for key, val in sorted(WORST.items()):
        print(f"patch-embed-worst {key[0]:12s} {key[1]:12s} {val:.3f}")


def _problem(name):
    """Operands on the device and the float64 reference of every token row, made once per case."""
    b, h, w, d, pos_mult = CASES[name]
    c, gh, gw = 3, h // 16, w // 16
    npatch = gh * gw
    g = torch.Generator().manual_seed(17 * b + d + h)
    img = torch.randn(b, c, h, w, generator=g) + 0.5 * torch.randn(b, c, 1, 1, generator=g)
    w16 = (torch.randn(d, c * 256, generator=g) * 0.03 * (1.0 + 0.5 * torch.rand(d, 1, generator=g))).half()
    bias, cls = torch.randn(d, generator=g), torch.randn(d, generator=g)
    pos = torch.randn(npatch + 1, d, generator=g) + 2.0 * torch.randn(npatch + 1, 1, generator=g)
    dev = {k: v.cuda() for k, v in dict(img=img, w=w16, bias=bias, cls=cls, pos=pos).items()}
    # im2col of the fp16-rounded image, k = (c, ky, kx)
    a = dev["img"].half().reshape(b, c, gh, 16, gw, 16).permute(0, 2, 4, 1, 3, 5).reshape(b * npatch, c * 256).contiguous()
    acc = og.acc_f64(a, dev["w"])
    f16 = lambda v: og.H16 * v.abs() + og.Z16
    pm = float(torch.tensor(pos_mult, dtype=torch.float32))
    x = acc.s + dev["bias"].double()
    p64 = dev["pos"].double()
    y = (x.view(b, npatch, d) + pm * p64[1:]).view(b * npatch, d)
    bound = og.SECOND * (acc.k * og.U32 * acc.a + og.U32 * x.abs() + og.U32 * y.abs() + f16(y))
    yc = dev["cls"].double() + pm * p64[0]
    bc = og.SECOND * (og.U32 * yc.abs() + f16(yc))
    ref = torch.cat([yc.expand(b, 1, d), y.view(b, npatch, d)], 1).reshape(b * (npatch + 1), d)
    bnd = torch.cat([bc.expand(b, 1, d), bound.view(b, npatch, d)], 1).reshape(b * (npatch + 1), d)
    return dict(dev, b=b, c=c, h=h, wpx=w, d=d, pos_mult=pos_mult, np=npatch, t=npatch + 1, ref=ref, bound=bnd)


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _problem(name)
        return cache[name]
    return get


class Guarded:
    """rows x cols values prefilled with `fill` between two guard rows."""

    def __init__(self, rows, cols, dtype, fill):
        self.buf = torch.full((rows + 2, cols), fill, dtype=dtype, device="cuda")
        self.fill = fill
        self.body = self.buf[1:-1]

    def ptr(self):
        return self.body.data_ptr()

    def guards_untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf[0] == self.fill).all()) and bool((self.buf[-1] == self.fill).all())


def _launch(L, p, tok, part, entry="fused", **over):
    q = dict(p, **over)
    args = [q["img"].data_ptr(), q["b"], q["c"], q["h"], q["wpx"], over.get("patch", 16), q["w"].data_ptr(),
            over.get("ldw", q["w"].shape[1]), q["bias"].data_ptr(), q["cls"].data_ptr(), q["pos"].data_ptr(),
            q["pos_mult"], q["d"], tok.ptr(), over.get("dtype", F16)]
    if entry == "fused":
        return L.hcir_patch_embed_fused(*args, None if part is None else part.ptr(), _st())
    return L.hcir_patch_embed(*args, _st())


@pytest.mark.parametrize("name", list(CASES))
def test_every_token_row_and_its_statistics(L, problems, name):
    p = problems(name)
    b, d, t = p["b"], p["d"], p["t"]
    m, nsl = b * t, d // 64
    assert L.hcir_patch_embed_route(b, p["c"], p["h"], p["wpx"], 16, d, p["w"].shape[1], F16) == BIG
    tok = Guarded(m, d, torch.float16, SENT)
    part = Guarded(nsl * m, 2, torch.float32, SENT)
    stats = Guarded(m, 2, torch.float32, SENT)
    assert _launch(L, p, tok, part) == 0
    assert L.hcir_ln_stats_finalize(part.ptr(), nsl, m, d, og.LN_EPS, stats.ptr(), _st()) == 0
    assert tok.guards_untouched() and part.guards_untouched() and stats.guards_untouched()
    rows = tok.body.clone()
    is_cls = (torch.arange(m, device="cuda") % t) == 0
    r = {"patch_rows": og.ratio(rows[~is_cls], p["ref"][~is_cls], p["bound"][~is_cls]),
         "class_rows": og.ratio(rows[is_cls], p["ref"][is_cls], p["bound"][is_cls])}
    # the statistics are those of the fp16 rows the device stored, class rows included
    sl = part.body.view(nsl, m, 2)
    st = stats.body
    mean_p, m2_p, d_mean_p, d_m2_p = og.slice_stats_f64(rows)
    mean, rstd, d_mean, d_rstd = og.finalize_f64(mean_p, m2_p, og.LN_EPS, d_mean_p, d_m2_p)
    given = og.finalize_f64(sl[..., 0], sl[..., 1], og.LN_EPS)
    r.update(slice_mean=og.ratio(sl[..., 0], mean_p, d_mean_p), slice_m2=og.ratio(sl[..., 1], m2_p, d_m2_p),
             slice_mean_cls=og.ratio(sl[:, is_cls, 0], mean_p[:, is_cls], d_mean_p[:, is_cls]),
             slice_m2_cls=og.ratio(sl[:, is_cls, 1], m2_p[:, is_cls], d_m2_p[:, is_cls]),
             mean=og.ratio(st[:, 0], mean, d_mean), rstd=og.ratio(st[:, 1], rstd, d_rstd),
             fin_mean=og.ratio(st[:, 0], given[0], given[2]), fin_rstd=og.ratio(st[:, 1], given[1], given[3]))
    for k, v in r.items():
        print(f"{name} {k} err/bound = {v:.4f}")
        WORST[(name, k)] = v
    assert all(v <= 1.0 for v in r.values()), (name, r)


def test_without_statistics_same_rows(L, problems):
    """stats_part = NULL: the same token rows, bit for bit; and the old entry agrees within the two bounds."""
    p = problems("b3")
    m, d = p["b"] * p["t"], p["d"]
    with_stats, without, old = (Guarded(m, d, torch.float16, SENT) for _ in range(3))
    part = Guarded((d // 64) * m, 2, torch.float32, SENT)
    assert _launch(L, p, with_stats, part) == 0
    assert _launch(L, p, without, None) == 0
    assert _launch(L, p, old, None, entry="old") == 0
    assert without.guards_untouched() and old.guards_untouched()
    assert torch.equal(with_stats.body, without.body)
    assert og.ratio(old.body, p["ref"], p["bound"]) <= 1.0
    print(f"elements that differ from hcir_patch_embed's: {int((old.body != without.body).sum())} of {old.body.numel()}")


@pytest.mark.parametrize("what", ["patch14", "d384", "f32-tokens", "padded-ldw"])
def test_refused_shapes_leave_tok_untouched(L, problems, what):
    """Shapes off the route: HCIR_ERR_UNSUPPORTED, the route query says the old kernel, tok is not written."""
    p = problems("b3")
    over = {"patch14": dict(patch=14, ldw=640), "d384": dict(d=384), "f32-tokens": dict(dtype=F32),
            "padded-ldw": dict(ldw=832)}[what]
    q = dict(p, **over)
    assert L.hcir_patch_embed_route(q["b"], q["c"], q["h"], q["wpx"], over.get("patch", 16), q["d"],
                                    over.get("ldw", 768), over.get("dtype", F16)) == TILE128
    rows = p["b"] * (257 if what == "patch14" else p["t"])
    tok = Guarded(rows, 2 * p["d"], torch.float16, SENT)        # (room for fp32 tokens: never written)
    part = Guarded((p["d"] // 64) * rows, 2, torch.float32, SENT)
    assert _launch(L, p, tok, part, **over) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((tok.buf == SENT).all()) and bool((part.buf == SENT).all())
