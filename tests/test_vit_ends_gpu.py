"""GPU: the two ends of the ViT forward in hcir.vit_engine.

(a) The CLS-only last block (LayerNorm fold on) launches its qkv GEMM over the columns [d, 3d) only (K and V; W / c1 /
    c2 / bias advanced by d rows resp. elements, out = qkv + d, ldo = 3d).  Such a launch must leave the columns [0, d)
    alone and write the same bits into [d, 3d) as the launch over all 3d columns.  hcir_gemm_f16 at m = 600 (ragged,
    128 x 128 kernel) and at m = 1112 (ragged, 256 x 256 persistent kernel); hcir_gemm_f16_fused (LayerNorm form) at
    m = 1112 - it refuses m < 1024 (hcir_gemm_fused_supported), which is asserted at m = 600.
    Q of the class rows comes from hcir_gemm_f16_ln_rows (rows picked by their pitch, their own statistics): it must
    give those rows the bits they have in the hcir_gemm_f16_fused launch over every row, so that the embedding is the
    one the whole launch gave.
(b) Engines on randomised 1- and 2-layer models of ViT-B width: the class token of forward_tokens(cls_only_last=True)
    against cls_only_last=False (1e-6 in 1 - cosine) and against an engine run with the LayerNorm fold off (1e-5): the
    tolerances tests/test_vit_gpu.py uses for the same two comparisons.  Batch 3 (591 token rows: separate LayerNorms,
    128 x 128 kernels) and batch 6 (1182 rows: the fold, the persistent kernels and hcir_patch_embed_fused, asserted
    through the route query).  Every model runs twice with different inputs and once over a buffer full of a
    sentinel: its result may not depend on what the qkv buffer held (the attention kernel's first query tile loads Q
    rows that the CLS-only last block does not write).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import gemm as og

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
SENT = -7.25
D, HEADS, MLP = 768, 12, 3072


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    return hcir_built


# ---------------------------------------------------------------------------------------------------------------
# (a) column-range launches
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qkv_problem():
    cache = {}

    def get(m):
        if m not in cache:
            p = og.make_problem("plain", m, 3 * D, D, seed=3)
            cache[m] = {k: v.cuda() for k, v in p.items()}
        return cache[m]
    return get


def _off(t, elems):
    return t.data_ptr() + elems * t.element_size()


@pytest.mark.parametrize("m,entry", [(600, "gemm"), (1112, "gemm"), (1112, "fused")])
def test_column_range_launch_same_bits(L, qkv_problem, m, entry):
    p = qkv_problem(m)
    d = D
    assert L.hcir_gemm_fused_supported(m, 2 * d, d) == (1 if m >= 1024 else 0)
    full = torch.full((m + 2, 3 * d), SENT, dtype=torch.float16, device="cuda")
    part = torch.full((m + 2, 3 * d), SENT, dtype=torch.float16, device="cuda")

    def launch(out, c0):
        o = out[1:-1]
        if entry == "fused":
            return L.hcir_gemm_f16_fused(p["a"].data_ptr(), d, _off(p["w"], c0 * d), d, _off(p["bias"], c0), None, m,
                                         3 * d - c0, d, 0, _off(o, c0), 3 * d, p["stats"].data_ptr(),
                                         _off(p["c1"], c0), None, _st())
        return L.hcir_gemm_f16(p["a"].data_ptr(), d, _off(p["w"], c0 * d), d, _off(p["bias"], c0), None, m,
                               3 * d - c0, d, 0, _off(o, c0), 3 * d, _st())

    assert launch(full, 0) == 0
    assert launch(part, d) == 0
    torch.cuda.synchronize()
    assert bool((part[:, :d] == SENT).all()), "columns [0, d) written"
    assert bool((part[0] == SENT).all()) and bool((part[-1] == SENT).all()), "guard rows written"
    assert not bool((full[1:-1] == SENT).all(1).any())
    assert torch.equal(part[1:-1, d:], full[1:-1, d:])


@pytest.mark.parametrize("t,b", [(8, 139), (197, 5), (1112, 1)])
def test_class_row_q_has_the_bits_of_the_whole_launch(L, qkv_problem, t, b):
    """Rows 0, t, 2t, ... of a 1112-row matrix through hcir_gemm_f16_ln_rows (row pitch t * d, compact statistics,
    output pitch t * 3d) against the hcir_gemm_f16_fused launch over all rows: bit-equal Q columns, nothing else
    written.  139 rows: one ragged 192-row tile; 5 rows and 1 row: far fewer than a tile."""
    p = qkv_problem(1112)
    d, m = D, 1112
    full = torch.full((m, 3 * d), SENT, dtype=torch.float16, device="cuda")
    assert L.hcir_gemm_f16_fused(p["a"].data_ptr(), d, p["w"].data_ptr(), d, p["bias"].data_ptr(), None, m, 3 * d, d, 0,
                                 full.data_ptr(), 3 * d, p["stats"].data_ptr(), p["c1"].data_ptr(), None, _st()) == 0
    rows = torch.full((m, 3 * d), SENT, dtype=torch.float16, device="cuda")
    stats_c = p["stats"][::t][:b].contiguous()
    assert L.hcir_gemm_f16_ln_rows(p["a"].data_ptr(), t * d, p["w"].data_ptr(), d, p["bias"].data_ptr(), b, d, d,
                                   rows.data_ptr(), t * 3 * d, stats_c.data_ptr(), p["c1"].data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    picked = torch.arange(b, device="cuda") * t
    assert torch.equal(rows[picked, :d], full[picked, :d])
    rows[picked, :d] = SENT
    assert bool((rows == SENT).all()), "written outside the class rows' Q columns"
    assert L.hcir_gemm_f16_ln_rows(p["a"].data_ptr(), t * d, p["w"].data_ptr(), d, p["bias"].data_ptr(), b, d + 64, d,
                                   rows.data_ptr(), t * 3 * d, stats_c.data_ptr(), p["c1"].data_ptr(), _st()) == UNSUPPORTED


def test_fused_form_refuses_small_m(L, qkv_problem):
    p = qkv_problem(600)
    out = torch.full((600, 3 * D), SENT, dtype=torch.float16, device="cuda")
    assert L.hcir_gemm_f16_fused(p["a"].data_ptr(), D, p["w"].data_ptr(), D, p["bias"].data_ptr(), None, 600, 2 * D, D,
                                 0, out.data_ptr(), 3 * D, p["stats"].data_ptr(), p["c1"].data_ptr(), None,
                                 _st()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------------------------------------
# (b) engines
# ---------------------------------------------------------------------------------------------------------------
def _spec(layers, seed):
    from hcir.vit_engine import VitLayer, VitSpec
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    ln = lambda: (1.0 + 0.2 * rnd(D), 0.2 * rnd(D))
    ls = []
    for _ in range(layers):
        (g1, b1), (g2, b2) = ln(), ln()
        ls.append(VitLayer(ln1_w=g1, ln1_b=b1, qkv_w=rnd(3 * D, D) * D ** -0.5, qkv_b=0.2 * rnd(3 * D),
                           proj_w=rnd(D, D) * D ** -0.5, proj_b=0.2 * rnd(D), ln2_w=g2, ln2_b=b2,
                           fc1_w=rnd(MLP, D) * D ** -0.5, fc1_b=0.2 * rnd(MLP),
                           fc2_w=rnd(D, MLP) * MLP ** -0.5, fc2_b=0.2 * rnd(D)))
    return VitSpec(patch=16, dim=D, heads=HEADS, eps=1e-6, pos_mult=2.0, conv_w=rnd(D, 3, 16, 16) * 0.03,
                   conv_b=0.2 * rnd(D), cls=0.2 * rnd(1, 1, D), pos=0.2 * rnd(1, 197, D), layers=ls)


def _cos_err(a, b):
    return (1.0 - F.cosine_similarity(a.double(), b.double(), dim=1)).abs().max().item()


def _cls(engine, x, cls_only_last):
    with torch.no_grad():
        return engine.forward_tokens(x, cls_only_last=cls_only_last)[:, 0].float().cpu()


@pytest.mark.parametrize("b", [3, 6])
@pytest.mark.parametrize("layers", [1, 2])
def test_cls_only_last_block_same_class_token(L, monkeypatch, layers, b):
    from hcir import vit_engine
    dev = torch.device("cuda", 0)
    spec = _spec(layers, 100 + layers)
    x = torch.randn(b, 3, 224, 224, generator=torch.Generator().manual_seed(b)).cuda()
    monkeypatch.setattr(vit_engine, "LN_FUSE", True)
    eng = vit_engine.VitEngine(spec, dev, torch.float16)
    fold_on = b * 197 >= 1024
    assert L.hcir_gemm_fused_supported(b * 197, 3 * D, D) == (1 if fold_on else 0)
    assert L.hcir_patch_embed_route(b, 3, 224, 224, 16, D, 768, 1) == 1      # what the engine takes with the fold on
    short = _cls(eng, x, True)
    full = _cls(eng, x, False)
    assert torch.isfinite(short).all() and torch.isfinite(full).all()
    print(f"{layers} layer(s), b {b}: CLS-only vs full 1-cos = {_cos_err(short, full):.2e}")
    assert _cos_err(short, full) <= 1e-6
    # a second engine, run with the LayerNorm fold off: separate LayerNorms and the old patch embedding
    monkeypatch.setattr(vit_engine, "LN_FUSE", False)
    eng_off = vit_engine.VitEngine(spec, dev, torch.float16)
    short_off = _cls(eng_off, x, True)
    full_off = _cls(eng_off, x, False)
    print(f"{layers} layer(s), b {b}: fold on vs off 1-cos = {_cos_err(short, short_off):.2e}")
    assert _cos_err(short_off, full_off) <= 1e-6
    assert _cos_err(short, short_off) <= 1e-5
    if not fold_on:
        assert torch.equal(short, short_off)       # nothing to fold below 1024 rows: the same calls


@pytest.mark.parametrize("b", [3, 6])
@pytest.mark.parametrize("layers", [1, 2])
def test_result_does_not_depend_on_buffer_contents(L, monkeypatch, layers, b):
    from hcir import vit_engine
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(vit_engine, "LN_FUSE", True)
    spec = _spec(layers, 7)
    g = torch.Generator().manual_seed(50 + b)
    x1, x2 = (torch.randn(b, 3, 224, 224, generator=g).cuda() for _ in range(2))
    eng = vit_engine.VitEngine(spec, dev, torch.float16)
    a1 = _cls(eng, x1, True)
    a2 = _cls(eng, x2, True)
    fresh = _cls(vit_engine.VitEngine(spec, dev, torch.float16), x2, True)     # zero-initialised qkv buffer
    assert torch.equal(a2, fresh)
    eng._bufs[(b, 197, 0)]["qkv"].fill_(SENT)                                   # ... and a buffer full of something else
    assert torch.equal(_cls(eng, x1, True), a1)
    assert not torch.equal(a1, a2)
