"""GPU parity of the ViT kernels (C ABI) and of the end-to-end embedding.

Floating-point path: fp16 MFMA operands, fp32 accumulate.  Tolerances are written in
each test; the end-to-end bar is north_star's: 1 - cos(embedding, oracle) <= 1e-3.
Per-kernel references are plain torch fp32 of the same op on the same (fp16-rounded)
operands; the end-to-end reference is oracle.vit (fp32, un-rounded weights).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit as ovit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hcir_built):
    assert torch.cuda.is_available()
    return hcir_built


def _st():
    return torch.cuda.current_stream().cuda_stream


# m >= 1024 with n % 256 == 0 and k % 64 == 0 takes the persistent 256 x 256 kernel (full and edge tiles,
# one tile per workgroup and several), everything else the 128 x 128 kernel
@pytest.mark.parametrize("m,n,k", [(128, 128, 64), (197 * 3, 768, 768), (1000, 2304, 768),
                                   (333, 3072, 768), (260, 768, 3072), (5, 8, 8), (130, 136, 72),
                                   (1024, 256, 64), (1300, 768, 768), (197 * 11, 2304, 768),
                                   (1537, 3072, 768), (1100, 768, 3072), (256 * 70 + 3, 1024, 128)])
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 6])
def test_gemm_epilogues(L, m, n, k, epi):
    from hcir import _lib
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k + epi)
    a = (torch.randn(m, k, generator=g) * 0.5).half()
    w = (torch.randn(n, k, generator=g) * (k ** -0.5)).half()
    bias = torch.randn(n, generator=g)
    scale = torch.rand(n, generator=g) + 0.5
    ref = a.float() @ w.float().t() + bias
    ad, wd, bd, sd_ = a.cuda(), w.cuda(), bias.cuda(), scale.cuda()
    if epi in (0, 1):
        out = torch.empty(m, n, dtype=torch.float16, device="cuda")
        if epi == 1:
            ref = F.gelu(ref)
        sp = None
    elif epi == 2:
        resid = torch.randn(m, n, generator=g)
        out = resid.cuda()
        ref = resid + scale * ref
        sp = sd_.data_ptr()
    elif epi == 6:      # fp16 residual stream: read-modify-write in fp16 storage, add in fp32
        resid = torch.randn(m, n, generator=g).half()
        out = resid.cuda()
        ref = resid.float() + scale * ref
        sp = sd_.data_ptr()
    else:
        out = torch.empty(m, n, dtype=torch.float32, device="cuda")
        sp = None
    st = L.hcir_gemm_f16(ad.data_ptr(), k, wd.data_ptr(), k, bd.data_ptr(), sp, m, n, k, epi,
                         out.data_ptr(), n, _st())
    assert st == 0
    got = out.float().cpu()
    # fp32 accumulate of exact fp16 products: error is fp32 summation + (for fp16 outputs) one rounding
    tol = 2e-3 if epi in (0, 1, 6) else 1e-4
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=tol * max(1.0, ref.abs().max().item()), rtol=0)


@pytest.mark.parametrize("epi", [0, 6])
def test_gemm_row_pitch(L, epi):
    """A and W as strided views (row pitch > k): the persistent kernel carries separate pitches; the small
    kernel refuses them."""
    g = torch.Generator().manual_seed(91 + epi)
    m, n, k, lda, ldw, ldo = 1500, 512, 192, 256, 320, 640
    abuf = (torch.randn(m, lda, generator=g) * 0.5).half()
    wbuf = (torch.randn(n, ldw, generator=g) * k ** -0.5).half()
    bias = torch.randn(n, generator=g)
    obuf = torch.randn(m, ldo, generator=g).half()
    ref = abuf[:, :k].float() @ wbuf[:, :k].float().t() + bias
    if epi == 6:
        ref = obuf[:, :n].float() + ref
    ad, wd, bd, od = abuf.cuda(), wbuf.cuda(), bias.cuda(), obuf.cuda()
    assert L.hcir_gemm_f16(ad.data_ptr(), lda, wd.data_ptr(), ldw, bd.data_ptr(), None, m, n, k, epi,
                           od.data_ptr(), ldo, _st()) == 0
    got = od.float().cpu()
    np.testing.assert_allclose(got[:, :n].numpy(), ref.numpy(), atol=2e-3 * ref.abs().max().item(), rtol=0)
    np.testing.assert_array_equal(got[:, n:].numpy(), obuf[:, n:].float().numpy())   # padding untouched
    # small kernel (m < 1024): pitches other than k are refused, not mis-read
    assert L.hcir_gemm_f16(ad.data_ptr(), lda, wd.data_ptr(), ldw, bd.data_ptr(), None, 512, n, k, epi,
                           od.data_ptr(), ldo, _st()) == -2
    assert L.hcir_gemm_f16(ad.data_ptr(), k - 8, wd.data_ptr(), ldw, bd.data_ptr(), None, m, n, k, epi,
                           od.data_ptr(), ldo, _st()) == -1


@pytest.mark.parametrize("m,n,k", [(1500, 512, 192), (300, 256, 128), (197 * 8, 768, 3072)])
@pytest.mark.parametrize("epi", [2, 6])
def test_gemm_residual_out_of_place(L, m, n, k, epi):
    """hcir_gemm_f16_resid: out = resid + (acc + bias) with resid a separate buffer that stays untouched; bit-identical
    to the in-place form on a copy (both the persistent and the small kernel); other epilogues refuse a resid."""
    g = torch.Generator().manual_seed(m + n + k + epi)
    dt = torch.float32 if epi == 2 else torch.float16
    a = (torch.randn(m, k, generator=g) * 0.5).half().cuda()
    w = (torch.randn(n, k, generator=g) * k ** -0.5).half().cuda()
    bias = torch.randn(n, generator=g).cuda()
    resid = torch.randn(m, n, generator=g).to(dt).cuda()
    keep = resid.clone()
    out = torch.full((m, n), 9.0, dtype=dt, device="cuda")
    assert L.hcir_gemm_f16_resid(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), None, m, n, k, epi,
                                 resid.data_ptr(), out.data_ptr(), n, _st()) == 0
    inplace = keep.clone()
    assert L.hcir_gemm_f16(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), None, m, n, k, epi, inplace.data_ptr(), n,
                           _st()) == 0
    assert torch.equal(out, inplace) and torch.equal(resid, keep)
    assert L.hcir_gemm_f16_resid(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), None, m, n, k, 0, resid.data_ptr(),
                                 out.data_ptr(), n, _st()) == -1


@pytest.mark.parametrize("m,n,k", [(1500, 512, 192), (197 * 8, 3072, 768), (1025, 256, 64), (197 * 64, 3072, 768),
                                   (256 * 64, 1024, 256)])
def test_gemm_gelu_dual_output(L, m, n, k):
    """hcir_gemm_f16_gelu_dual: out_pre bit-equal to the BIAS_F16 epilogue, out_act bit-equal to the BIAS_GELU_F16
    epilogue (same fp32 value, rounded once each), whichever kernel the single-output launches select (the 256 x 256
    kernel for whole rounds of tiles, the 128 x 192 kernel for small launches and the rows behind the last whole
    round: both apply the bias in fp32 before the one rounding), and within fp16 rounding of torch's exact GELU;
    small M refused."""
    g = torch.Generator().manual_seed(m + n + k)
    a = (torch.randn(m, k, generator=g) * 0.5).half().cuda()
    w = (torch.randn(n, k, generator=g) * k ** -0.5).half().cuda()
    bias = torch.randn(n, generator=g).cuda()
    pre, act = (torch.full((m, n), 3.0, dtype=torch.float16, device="cuda") for _ in range(2))
    assert L.hcir_gemm_f16_gelu_dual(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), m, n, k, pre.data_ptr(),
                                     act.data_ptr(), n, _st()) == 0
    r0, r1 = (torch.empty((m, n), dtype=torch.float16, device="cuda") for _ in range(2))
    assert L.hcir_gemm_f16(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), None, m, n, k, 0, r0.data_ptr(), n, _st()) == 0
    assert L.hcir_gemm_f16(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), None, m, n, k, 1, r1.data_ptr(), n, _st()) == 0
    assert torch.equal(pre, r0) and torch.equal(act, r1)
    ref = F.gelu(a.float().cpu() @ w.float().cpu().t() + bias.cpu())
    assert (act.float().cpu() - ref).abs().max() <= 2e-3 * max(1.0, ref.abs().max().item())
    assert L.hcir_gemm_f16_gelu_dual(a.data_ptr(), k, w.data_ptr(), k, bias.data_ptr(), 512, n, k, pre.data_ptr(),
                                     act.data_ptr(), n, _st()) == -2


@pytest.mark.parametrize("m,n,k", [(64 * 197, 768, 3072), (64 * 197, 3072, 768), (64 * 197, 768, 768),
                                   (40 * 197, 768, 3072), (100 * 197, 1024, 4096)])
@pytest.mark.parametrize("epi", [0, 6])
def test_gemm_small_m_persistent(L, m, n, k, epi):
    """Small M on the persistent 256 x 256 kernel (64 images: 150 tiles for proj / fc2, 600 for fc1 - tile counts that
    fill the last round of the 256 CUs badly).  Reference values and run-to-run bit-identity.  (A stream-K schedule
    for these shapes was built and measured in round 3 - correct, deterministic, 48 % slower on fc2: 256 KB fp32
    partial tiles per workgroup; DESIGN.md "GEMM round 3".)"""
    g = torch.Generator().manual_seed(m + n + k + epi)
    a = (torch.randn(m, k, generator=g) * 0.5).half()
    w = (torch.randn(n, k, generator=g) * (k ** -0.5)).half()
    bias = torch.randn(n, generator=g)
    ad, wd, bd = a.cuda(), w.cuda(), bias.cuda()
    ref = (ad.float() @ wd.float().t() + bd).cpu()           # fp32 reference (torch on the device, fp32 accumulate)
    outs = []
    for rep in range(3):
        if epi == 6:
            resid = torch.randn(m, n, generator=torch.Generator().manual_seed(9)).half()
            out = resid.cuda()
            want = resid.float() + ref
        else:
            out = torch.full((m, n), float("nan"), dtype=torch.float16, device="cuda")
            want = ref
        assert L.hcir_gemm_f16(ad.data_ptr(), k, wd.data_ptr(), k, bd.data_ptr(), None, m, n, k, epi, out.data_ptr(), n,
                               _st()) == 0
        outs.append(out.clone())
    got = outs[0].float().cpu()
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=2e-3 * max(1.0, want.abs().max().item()), rtol=0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("m,n,k", [(197 * 300 + 5, 2304, 768), (197 * 220, 3072, 768), (70001, 512, 128)])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_many_tiles_per_workgroup(L, m, n, k, ln, epi):
    """Several 256 x 256 tiles per workgroup (23-32 at the benchmark's batch), ragged last row of tiles, plain and
    LayerNorm-folded fp16 epilogues.  (1) fp32 reference; (2) a row range of the same problem small enough for the
    128 x 192 kernel (same k order, same epilogue arithmetic) must give the SAME BITS; (3) run-to-run bit-identity.
    Also the gate for any change of the tile boundary (such as finishing tile t inside the first k-step of tile t+1):
    it has to pass this test unchanged."""
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    a = (torch.randn(m, k, device="cuda", generator=g) * 0.5 + torch.randn(m, 1, device="cuda", generator=g)).half()
    w = (torch.randn(n, k, device="cuda", generator=g) * k ** -0.5).half()
    bias = torch.randn(n, device="cuda", generator=g)
    x = a.float()
    stats = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()], 1).contiguous()
    c1 = w.float().sum(1)

    def run(rows0, nrows, out):
        ap = a.data_ptr() + rows0 * k * 2
        if ln:
            return L.hcir_gemm_f16_fused(ap, k, w.data_ptr(), k, bias.data_ptr(), None, nrows, n, k, epi, out.data_ptr(),
                                         n, stats.data_ptr() + rows0 * 8, c1.data_ptr(), None, _st())
        return L.hcir_gemm_f16(ap, k, w.data_ptr(), k, bias.data_ptr(), None, nrows, n, k, epi, out.data_ptr(), n, _st())

    outs = []
    for rep in range(2):
        out = torch.full((m, n), float("nan"), dtype=torch.float16, device="cuda")
        assert run(0, m, out) == 0
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    got = outs[0]
    assert torch.isfinite(got).all()
    for r0 in range(0, m, 8192):                       # reference in row blocks (memory)
        r1 = min(m, r0 + 8192)
        xa = a[r0:r1].float()
        if ln:
            xa = (xa - stats[r0:r1, :1]) * stats[r0:r1, 1:]
        want = xa @ w.float().t() + bias
        if epi == 1:
            want = F.gelu(want)
        err = (got[r0:r1].float() - want).abs().max().item()
        assert err <= 3e-3 * max(1.0, want.abs().max().item()), (r0, err)
    # the same rows through the 128 x 192 kernel (a launch of < 0.7 rounds of 256 x 256 tiles takes it)
    tn = n // 256
    nrows = max(1024, (150 // tn) * 256)
    for rows0 in (0, ((m // 2) // 256) * 256 + 256, m - nrows):
        part = torch.full((nrows, n), float("nan"), dtype=torch.float16, device="cuda")
        assert run(rows0, nrows, part) == 0
        torch.cuda.synchronize()
        assert torch.equal(part, got[rows0:rows0 + nrows]), rows0


@pytest.fixture(scope="module")
def same_bits_problem():
    """Operands of test_gemm_big_and_mid_kernels_same_bits, made once: 4 x 45 tiles of 256 x 256 (180 x 10 >= 256 x 7:
    the 256 x 256 kernel; 180 <= 256: no tail split; ragged last row of tiles), k = 64."""
    m, n, k = 11517, 1024, 64
    g = torch.Generator(device="cuda").manual_seed(m + n + k)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    a = (rnd(m, k) * 0.5).half()
    w = (rnd(n, k) * k ** -0.5).half()
    x = a.float()
    return dict(m=m, n=n, k=k, a=a, w=w, bias=rnd(n), scale=torch.rand(n, device="cuda", generator=g) + 0.5,
                resid=rnd(m, n), acc=x @ w.float().t(), c1=w.float().sum(1),
                stats=torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()], 1).contiguous())


@pytest.mark.parametrize("case", ["bias_f16", "gelu_f16", "resid_f32_scale", "bias_f32", "resid_f16_scale", "resid_f16",
                                  "affine_relu_f16", "affine_f32", "ln_bias_f16", "ln_gelu_f16", "resid_f16_stats"])
def test_gemm_big_and_mid_kernels_same_bits(L, same_bits_problem, case):
    """The 256 x 256 and the 128 x 192 kernel share one epilogue and one k order: for EVERY epilogue, a row range of a
    problem that is small enough for the 128 x 192 kernel (1530 rows = 8 x 8 tiles, under 0.7 of a round of 256 x 256
    tiles; the last 48-row half ragged) gives the bits that the 256 x 256 kernel gave for those rows of the whole
    problem - the per-row statistics slices included.  One fp32 reference comparison per epilogue (tolerances of
    test_gemm_epilogues), so that "same bits" is not "same wrong bits"."""
    p = same_bits_problem
    m, n, k, a, w, bias, scale, acc = (p[x] for x in ("m", "n", "k", "a", "w", "bias", "scale", "acc"))
    epi, fused, sc, f32 = {"bias_f16": (0, None, None, False), "gelu_f16": (1, None, None, False),
                           "resid_f32_scale": (2, None, scale, True), "bias_f32": (3, None, None, True),
                           "resid_f16_scale": (6, None, scale, False), "resid_f16": (6, None, None, False),
                           "affine_relu_f16": (4, None, scale, False), "affine_f32": (5, None, scale, True),
                           "ln_bias_f16": (0, "ln", None, False), "ln_gelu_f16": (1, "ln", None, False),
                           "resid_f16_stats": (6, "stats", None, False)}[case]
    dt = torch.float32 if f32 else torch.float16
    resid = p["resid"].to(dt) if epi in (2, 6) else None
    if fused == "ln":
        ref = (a.float() - p["stats"][:, :1]) * p["stats"][:, 1:] @ w.float().t() + bias
    elif epi in (4, 5):
        ref = acc * scale + bias
    else:
        ref = acc + bias
    if epi == 1:
        ref = F.gelu(ref)
    if epi == 4:
        ref = F.relu(ref)
    if resid is not None:
        ref = resid.float() + (ref * sc if sc is not None else ref)
    nsl = n // 64

    def run(rows0, nrows):
        out = resid[rows0:rows0 + nrows].clone() if resid is not None else \
            torch.full((nrows, n), float("nan"), dtype=dt, device="cuda")
        part = torch.full((nsl, nrows, 2), float("nan"), device="cuda") if fused == "stats" else None
        ap, scp = a.data_ptr() + rows0 * k * 2, sc.data_ptr() if sc is not None else None
        if fused:
            st = L.hcir_gemm_f16_fused(ap, k, w.data_ptr(), k, bias.data_ptr(), scp, nrows, n, k, epi, out.data_ptr(), n,
                                       p["stats"].data_ptr() + rows0 * 8 if fused == "ln" else None,
                                       p["c1"].data_ptr() if fused == "ln" else None,
                                       part.data_ptr() if part is not None else None, _st())
        else:
            st = L.hcir_gemm_f16(ap, k, w.data_ptr(), k, bias.data_ptr(), scp, nrows, n, k, epi, out.data_ptr(), n, _st())
        assert st == 0
        torch.cuda.synchronize()
        return out, part

    full, full_part = run(0, m)
    tol = 1e-4 if f32 else 2e-3
    err = (full.float() - ref).abs().max().item()
    print(f"{case}: max abs error {err:.3e}, bound {tol * max(1.0, ref.abs().max().item()):.3e}")
    assert err <= tol * max(1.0, ref.abs().max().item())
    nrows = 1530
    for rows0 in (0, m - nrows):
        part_out, part_stats = run(rows0, nrows)
        assert torch.equal(part_out, full[rows0:rows0 + nrows]), rows0
        if fused == "stats":      # the whole problem's slices have pitch m, the row range's pitch nrows
            assert torch.isfinite(full_part).all()
            assert torch.equal(part_stats, full_part[:, rows0:rows0 + nrows]), rows0


@pytest.mark.parametrize("m,d,mlp", [(1500, 256, 512), (197 * 6, 768, 3072), (197 * 64, 768, 3072)])
def test_gemm_fused_layernorm(L, m, d, mlp):
    """hcir_gemm_f16_fused: (1) the fp16-residual epilogue also emits per-row (mean, M2) slices ->
    hcir_ln_stats_finalize -> (mean, rstd) of the STORED rows; (2) the consumer GEMM reads the raw rows and
    applies LayerNorm algebraically.  Checked against torch LayerNorm + Linear (+ GELU) in fp32."""
    g = torch.Generator().manual_seed(m + d)
    eps = 1e-6
    a = (torch.randn(m, mlp, generator=g) * 0.5).half()
    w2 = (torch.randn(d, mlp, generator=g) * mlp ** -0.5).half()
    b2 = torch.randn(d, generator=g)
    # residual rows with a per-row offset (mean != 0) and a few large channels
    resid = torch.randn(m, d, generator=g) + torch.randn(m, 1, generator=g) * 2.0
    resid[: m // 4] += 60.0          # rows with |mean| / std ~ 50: the variance must survive (Chan combination)
    resid[:, 5] *= 20.0
    resid = resid.half()
    new_rows = (resid.float() + a.float() @ w2.float().t() + b2).half()          # what the epilogue stores
    ad, wd, bd, od = a.cuda(), w2.cuda(), b2.cuda(), resid.cuda()
    nsl = L.hcir_gemm_stats_slices(d)
    assert nsl == d // 64 and L.hcir_gemm_fused_supported(m, d, mlp) == 1
    part = torch.full((nsl, m, 2), float("nan"), device="cuda")
    stats = torch.empty((m, 2), device="cuda")
    assert L.hcir_gemm_f16_fused(ad.data_ptr(), mlp, wd.data_ptr(), mlp, bd.data_ptr(), None, m, d, mlp, 6,
                                 od.data_ptr(), d, None, None, part.data_ptr(), _st()) == 0
    assert L.hcir_ln_stats_finalize(part.data_ptr(), nsl, m, d, eps, stats.data_ptr(), _st()) == 0
    got_rows = od.cpu()
    np.testing.assert_allclose(got_rows.float().numpy(), new_rows.float().numpy(),
                               atol=2e-3 * new_rows.float().abs().max().item(), rtol=0)
    x = got_rows.double()                                   # statistics are those of the rows AS STORED
    mean, var = x.mean(1), x.var(1, unbiased=False)
    st_cpu = stats.cpu().double()
    np.testing.assert_allclose(st_cpu[:, 0].numpy(), mean.numpy(), atol=1e-5 * x.abs().max().item(), rtol=0)
    np.testing.assert_allclose(st_cpu[:, 1].numpy(), (var + eps).rsqrt().numpy(), rtol=2e-5)

    # consumer: LayerNorm(x) @ W1^T + b1 (+ GELU) from the raw rows
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.2 * torch.randn(d, generator=g)
    w1 = torch.randn(mlp, d, generator=g) * d ** -0.5
    b1 = torch.randn(mlp, generator=g)
    wg = (w1.double() * gamma.double()[None, :]).half()
    c1 = wg.double().sum(1).float()
    c2 = (w1.double() @ beta.double() + b1.double()).float()
    ref = F.layer_norm(got_rows.float(), (d,), gamma, beta, eps) @ w1.t() + b1
    for epi, fn in ((0, lambda z: z), (1, F.gelu)):
        out = torch.empty((m, mlp), dtype=torch.float16, device="cuda")
        assert L.hcir_gemm_f16_fused(od.data_ptr(), d, wg.cuda().data_ptr(), d, c2.cuda().data_ptr(), None, m, mlp,
                                     d, epi, out.data_ptr(), mlp, stats.data_ptr(), c1.cuda().data_ptr(), None,
                                     _st()) == 0
        torch.cuda.synchronize()
        want = fn(ref)
        np.testing.assert_allclose(out.float().cpu().numpy(), want.numpy(),
                                   atol=3e-3 * max(1.0, want.abs().max().item()), rtol=0)
    # argument checks: nothing fused / both / unsupported shapes and epilogues
    assert L.hcir_gemm_f16_fused(od.data_ptr(), d, wd.data_ptr(), d, bd.data_ptr(), None, m, d, d, 0,
                                 od.data_ptr(), d, None, None, None, _st()) == -1
    assert L.hcir_gemm_f16_fused(ad.data_ptr(), mlp, wd.data_ptr(), mlp, bd.data_ptr(), None, 512, d, mlp, 6,
                                 od.data_ptr(), d, None, None, part.data_ptr(), _st()) == -2
    assert L.hcir_gemm_f16_fused(ad.data_ptr(), mlp, wd.data_ptr(), mlp, bd.data_ptr(), None, m, d, mlp, 0,
                                 od.data_ptr(), d, None, None, part.data_ptr(), _st()) == -2


def test_gemm_affine_epilogues(L):
    g = torch.Generator().manual_seed(5)
    m, n, k = 70, 512, 768
    a = torch.randn(m, k, generator=g).half()
    w = (torch.randn(n, k, generator=g) * k ** -0.5).half()
    s, b = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    ref = (a.float() @ w.float().t()) * s + b
    o16 = torch.empty(m, n, dtype=torch.float16, device="cuda")
    o32 = torch.empty(m, n, dtype=torch.float32, device="cuda")
    args = (a.cuda(), w.cuda(), b.cuda(), s.cuda())
    assert L.hcir_gemm_f16(args[0].data_ptr(), k, args[1].data_ptr(), k, args[2].data_ptr(), args[3].data_ptr(),
                           m, n, k, 4, o16.data_ptr(), n, _st()) == 0
    assert L.hcir_gemm_f16(args[0].data_ptr(), k, args[1].data_ptr(), k, args[2].data_ptr(), args[3].data_ptr(),
                           m, n, k, 5, o32.data_ptr(), n, _st()) == 0
    np.testing.assert_allclose(o32.cpu().numpy(), ref.numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(o16.float().cpu().numpy(), F.relu(ref).numpy(), atol=4e-3, rtol=0)


@pytest.mark.parametrize("xdt", [torch.float32, torch.float16])
@pytest.mark.parametrize("rows,d", [(197 * 2, 768), (7, 1024), (33, 2048), (5, 64)])
def test_layernorm(L, rows, d, xdt):
    g = torch.Generator().manual_seed(rows + d)
    x = (torch.randn(rows, d, generator=g) * 3 + 0.7).to(xdt)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    ref = F.layer_norm(x.float(), (d,), w, b, 1e-6)
    y = torch.empty(rows, d, dtype=torch.float16, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    assert L.hcir_layernorm_f16(xd.data_ptr(), 0 if xdt == torch.float32 else 1, rows, d, d, wd.data_ptr(),
                                bd.data_ptr(), 1e-6, y.data_ptr(), d, _st()) == 0
    # fp16 output rounding: 2^-11 relative
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), atol=2e-3 * ref.abs().max().item(), rtol=0)
    from oracle import rowops as ro
    from oracle.attention import f32
    assert ro.ratio(y.cpu(), *ro.layernorm_f64(x, w, b, f32(1e-6))) <= 1.0       # every element, the derived bound


@pytest.mark.parametrize("b,t,h", [(2, 197, 12), (1, 17, 2), (3, 64, 4), (2, 257, 16), (1, 33, 1), (1, 288, 2)])
def test_attention(L, b, t, h):
    g = torch.Generator().manual_seed(b * 100 + t + h)
    hd = 64
    qkv = (torch.randn(b, t, 3, h, hd, generator=g) * 1.5).half()
    q, k, v = [qkv[:, :, i].float().permute(0, 2, 1, 3) for i in range(3)]  # [b,h,t,hd]
    scale = hd ** -0.5
    ref = torch.softmax((q * scale) @ k.transpose(-2, -1), -1) @ v
    ref = ref.permute(0, 2, 1, 3).reshape(b, t, h * hd)
    out = torch.empty(b, t, h * hd, dtype=torch.float16, device="cuda")
    qd = qkv.cuda()
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, scale, t, out.data_ptr(), _st()) == 0
    # P is rounded to fp16 before PV (2^-11 relative per term), output rounded to fp16
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), atol=6e-3, rtol=0)


def test_attention_persistent_kernel_matches_per_item_kernel(L):
    """>= 512 (b, head) items at 193..224 tokens take the persistent double-buffered kernel (seven waves, the next
    item's K / V images in flight under the current item's compute); fewer items take the workgroup-per-item kernel.
    Same arithmetic: the outputs of one 48-image call equal those of two 24-image calls bit for bit, run after run."""
    b, t, h = 48, 197, 12
    g = torch.Generator().manual_seed(77)
    qkv = (torch.randn(b, t, 3 * h * 64, generator=g) * 0.7).half().cuda()
    scale = 64 ** -0.5
    whole = torch.empty(b, t, h * 64, dtype=torch.float16, device="cuda")
    halves = torch.empty_like(whole)
    for lo in (0, b // 2):
        assert L.hcir_attn_fwd(qkv[lo:lo + b // 2].data_ptr(), b // 2, t, h, 64, scale, t, halves[lo:lo + b // 2].data_ptr(),
                               _st()) == 0
    for rep in range(5):
        whole.fill_(float("nan"))
        assert L.hcir_attn_fwd(qkv.data_ptr(), b, t, h, 64, scale, t, whole.data_ptr(), _st()) == 0
        assert torch.equal(whole, halves), rep
    q, k, v = qkv.float().reshape(b, t, 3, h, 64).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax((q * scale) @ k.transpose(-2, -1), dim=-1) @ v).transpose(1, 2).reshape(b, t, h * 64)
    assert (whole.float() - ref).abs().max().item() <= 4e-3


@pytest.mark.parametrize("b,t,h,hd", [(2, 257, 16, 80), (1, 197, 3, 128), (3, 33, 2, 32), (1, 288, 2, 96), (2, 50, 4, 48)])
def test_attention_other_head_dims(L, b, t, h, hd):
    """head_dim != 64 (vit_huge_patch14: 1280 / 16 = 80, HP/src/models_vit.py:266-270): the generic kernel."""
    g = torch.Generator().manual_seed(b * 100 + t + h + hd)
    qkv = (torch.randn(b, t, 3, h, hd, generator=g) * 1.2).half()
    q, k, v = [qkv[:, :, i].float().permute(0, 2, 1, 3) for i in range(3)]
    scale = hd ** -0.5
    ref = (torch.softmax((q * scale) @ k.transpose(-2, -1), -1) @ v).permute(0, 2, 1, 3).reshape(b, t, h * hd)
    out = torch.full((b, t, h * hd), float("nan"), dtype=torch.float16, device="cuda")
    qd = qkv.cuda()
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, scale, t, out.data_ptr(), _st()) == 0
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), atol=6e-3, rtol=0)
    part = torch.empty(b, 1, h * hd, dtype=torch.float16, device="cuda")
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, scale, 1, part.data_ptr(), _st()) == 0
    assert torch.equal(part, out[:, :1])
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, 72, scale, t, out.data_ptr(), _st()) == -2   # unsupported


def test_attention_query_row_limit(L):
    """nq < T: only the first nq query rows are computed, written compactly [B][nq][H*hd]."""
    b, t, h, hd = 3, 197, 12, 64
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(b, t, 3, h, hd, generator=g).half()
    qd = qkv.cuda()
    full = torch.empty(b, t, h * hd, dtype=torch.float16, device="cuda")
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, hd ** -0.5, t, full.data_ptr(), _st()) == 0
    for nq in (1, 40):
        part = torch.empty(b, nq, h * hd, dtype=torch.float16, device="cuda")
        assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, hd ** -0.5, nq, part.data_ptr(), _st()) == 0
        assert torch.equal(part, full[:, :nq])
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, hd ** -0.5, t + 1, full.data_ptr(), _st()) == -1


def test_attention_spiked_row(L):
    """One key dominates one query (softmax near one-hot) and large negative scores elsewhere."""
    b, t, h, hd = 1, 197, 1, 64
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(b, t, 3, h, hd, generator=g).half()
    qkv[0, 5, 0] = qkv[0, 150, 1] * 6.0     # q5 aligned with k150
    q, k, v = [qkv[:, :, i].float().permute(0, 2, 1, 3) for i in range(3)]
    ref = (torch.softmax((q * hd ** -0.5) @ k.transpose(-2, -1), -1) @ v).permute(0, 2, 1, 3).reshape(b, t, hd)
    out = torch.empty(b, t, hd, dtype=torch.float16, device="cuda")
    qd = qkv.cuda()
    assert L.hcir_attn_fwd(qd.data_ptr(), b, t, h, hd, hd ** -0.5, t, out.data_ptr(), _st()) == 0
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), atol=6e-3, rtol=0)


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16])
@pytest.mark.parametrize("b,pos_mult", [(3, 2.0), (1, 1.0)])
def test_patch_embed(L, b, pos_mult, tdt):
    g = torch.Generator().manual_seed(b)
    d = 768
    img = torch.randn(b, 3, 224, 224, generator=g)
    w = (torch.randn(d, 3, 16, 16, generator=g) * 0.03)
    bias, cls, pos = torch.randn(d, generator=g), torch.randn(d, generator=g), torch.randn(197, d, generator=g)
    w16 = w.half()
    ref = F.conv2d(img.half().float(), w16.float(), bias, stride=16).flatten(2).transpose(1, 2)
    ref = torch.cat([cls.expand(b, 1, d), ref], 1) + pos_mult * pos
    tok = torch.empty(b, 197, d, device="cuda", dtype=tdt)
    args = [t_.cuda() for t_ in (img, w16.reshape(d, -1).contiguous(), bias, cls, pos)]
    assert L.hcir_patch_embed(args[0].data_ptr(), b, 3, 224, 224, 16, args[1].data_ptr(), 768, args[2].data_ptr(),
                              args[3].data_ptr(), args[4].data_ptr(), pos_mult, d, tok.data_ptr(),
                              0 if tdt == torch.float32 else 1, _st()) == 0
    tol = 2e-4 if tdt == torch.float32 else 1e-3   # fp16 storage: one rounding, 2^-11 relative
    np.testing.assert_allclose(tok.float().cpu().numpy(), ref.numpy(), atol=tol * ref.abs().max().item(), rtol=0)


def test_patch_embed_patch14(L):
    """Generic patch size (ViT-L/14: P = 14, K = 588 zero-padded to 640, 257 tokens)."""
    g = torch.Generator().manual_seed(14)
    b, d, P = 2, 1024, 14
    img = torch.randn(b, 3, 224, 224, generator=g)
    w16 = (torch.randn(d, 3, P, P, generator=g) * 0.04).half()
    bias, cls, pos = torch.randn(d, generator=g), torch.randn(d, generator=g), torch.randn(257, d, generator=g)
    ref = F.conv2d(img.half().float(), w16.float(), bias, stride=P).flatten(2).transpose(1, 2)
    ref = torch.cat([cls.expand(b, 1, d), ref], 1) + pos
    wp = torch.zeros(d, 640, dtype=torch.float16)
    wp[:, :588] = w16.reshape(d, -1)
    tok = torch.empty(b, 257, d, device="cuda")
    args = [t_.cuda() for t_ in (img, wp, bias, cls, pos)]
    assert L.hcir_patch_embed(args[0].data_ptr(), b, 3, 224, 224, P, args[1].data_ptr(), 640, args[2].data_ptr(),
                              args[3].data_ptr(), args[4].data_ptr(), 1.0, d, tok.data_ptr(), 0, _st()) == 0
    np.testing.assert_allclose(tok.cpu().numpy(), ref.numpy(), atol=2e-4 * ref.abs().max().item(), rtol=0)
    assert L.hcir_patch_embed(args[0].data_ptr(), b, 3, 224, 224, P, args[1].data_ptr(), 588, args[2].data_ptr(),
                              args[3].data_ptr(), args[4].data_ptr(), 1.0, d, tok.data_ptr(), 0, _st()) == -1


def _randomize(model, seed):
    """Perturb every parameter / buffer so that no bias, LN weight or BN statistic is trivial."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in list(model.named_parameters()) + list(model.named_buffers()):
            if not p.dtype.is_floating_point:
                continue
            if "running_var" in name:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif name.endswith("ln_1.weight") or name.endswith("ln_2.weight") or name.endswith("ln.weight") \
                    or "norm" in name and name.endswith("weight") or ".1.weight" in name or ".4.weight" in name:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() <= 1 or "cls_token" in name or "pos_emb" in name or "pos_embed" in name:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))


def _cos_err(a, b):
    return (1.0 - F.cosine_similarity(a.double(), b.double(), dim=1)).abs().max().item()


@pytest.mark.parametrize("resid", [torch.float32, torch.float16])
def test_vit_b16_embedding_vs_oracle(L, resid, monkeypatch):
    """SHAM2('vit_b_16').extract_features + F.normalize vs the fp32 oracle: <= 1e-3 cosine, with the
    residual stream stored in fp32 and in fp16."""
    from hcir import vit_engine
    from hcir.main_backbone import SHAM2
    monkeypatch.setattr(vit_engine, "DEFAULT_RESID_DTYPE", resid)
    torch.manual_seed(42)
    model = SHAM2("vit_b_16").eval()
    _randomize(model, 1)
    # the two aliases of pos_embedding / must stay tied after perturbation
    assert model.backbone.pos_embedding.data_ptr() == model.backbone.encoder.pos_embedding.data_ptr()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(7))
    ref = ovit.sham2_extract_features(sd, x, "vit_b_16")
    model = model.cuda()
    with torch.no_grad():
        got = model.extract_features(x.cuda()).cpu()
        cls, pooled = model.backbone(x.cuda())
        z = model(x.cuda()).cpu()
        zm = model.forward_momentum(x.cuda()).cpu()
    assert model.backbone.engine(torch.device("cuda", 0)).resid_dtype == resid
    print(f"resid {resid}: embedding 1-cos = {_cos_err(got, ref):.2e}")
    assert _cos_err(got, ref) <= (1e-4 if resid == torch.float16 else 1e-5)   # bar 1e-3; measured far below
    ref_cls, ref_pool = ovit.vitwrapper_forward(sd, x, "backbone.")
    # extract_features runs the CLS-only last block, backbone(x) the full one: same class token
    assert _cos_err(got, cls.cpu()) <= 1e-6
    assert _cos_err(cls.cpu(), ref_cls) <= 1e-3
    assert _cos_err(pooled.cpu(), ref_pool) <= 1e-3
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=3e-2 * ref.abs().max().item(), rtol=0)
    # projection heads (eval-mode BN folded into the GEMM epilogue)
    ref_z = ovit.projection_head_forward(sd, ref_cls, "projection_head.")
    assert _cos_err(z, ref_z) <= 1e-3
    ref_m = ovit.projection_head_forward(sd, ovit.vitwrapper_forward(sd, x, "backbone_momentum.")[0],
                                         "projection_head_momentum.")
    assert _cos_err(zm, ref_m) <= 1e-3


def test_vit_b16_batch_on_persistent_gemm(L):
    """Batch 8 (M = 1576 token rows) runs the encoder GEMMs on the persistent 256 x 256 kernel, the path
    bench.py measures; same 1e-3 cosine bar against the fp32 oracle, per-image results independent of batch."""
    from hcir.main_backbone import SHAM2
    torch.manual_seed(43)
    model = SHAM2("vit_b_16").eval()
    _randomize(model, 2)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    ref = ovit.sham2_extract_features(sd, x, "vit_b_16")
    model = model.cuda()
    with torch.no_grad():
        got = model.extract_features(x.cuda()).cpu()
        small = model.extract_features(x[:3].cuda()).cpu()      # 128 x 128 kernel
    print(f"batch 8: embedding 1-cos = {_cos_err(got, ref):.2e}")
    assert _cos_err(got, ref) <= 1e-4
    assert _cos_err(got[:3], small) <= 1e-6


def test_vit_b16_layernorm_fold_vs_separate(L, monkeypatch):
    """fp16 residual stream, batch 8: LayerNorm folded into the GEMMs (default) and the separate
    hcir_layernorm_f16 launches give the same embedding within fp16 noise, both within the oracle bar."""
    from hcir import vit_engine
    from hcir.main_backbone import SHAM2
    monkeypatch.setattr(vit_engine, "DEFAULT_RESID_DTYPE", torch.float16)
    torch.manual_seed(44)
    model = SHAM2("vit_b_16").eval()
    _randomize(model, 3)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(12))
    ref = ovit.sham2_extract_features(sd, x, "vit_b_16")
    model = model.cuda()
    outs = {}
    for fuse in (True, False):
        monkeypatch.setattr(vit_engine, "LN_FUSE", fuse)
        with torch.no_grad():
            outs[fuse] = model.extract_features(x.cuda()).cpu()
            full = model.backbone(x.cuda())[0].cpu()          # full last block (no CLS-only shortcut)
        assert _cos_err(outs[fuse], full) <= 1e-6
        print(f"LN fold {fuse}: embedding 1-cos vs oracle = {_cos_err(outs[fuse], ref):.2e}")
        assert _cos_err(outs[fuse], ref) <= 1e-4
    assert _cos_err(outs[True], outs[False]) <= 1e-5


def test_vit_requires_no_grad_and_device(L):
    from hcir import HcirError
    from hcir.main_backbone import SHAM2
    model = SHAM2("vit_b_16").eval()
    x = torch.randn(1, 3, 224, 224)
    with torch.no_grad(), pytest.raises(HcirError):
        model.extract_features(x)  # CPU tensor: no fallback
    model = model.cuda()
    f = model.extract_features(x.cuda())  # autograd on: the differentiable forward (hcir.vit_train)
    assert f.requires_grad and f.shape == (1, 768)
    with torch.no_grad():
        assert _cos_err(f.detach().cpu(), model.extract_features(x.cuda()).cpu()) <= 1e-5   # same embedding
    with pytest.raises(NotImplementedError):
        model.backbone(x.cuda())  # class token + pooled patches: inference-only
    with pytest.raises(ValueError):
        SHAM2("vgg16")


@pytest.mark.parametrize("mean_over_std,outlier", [(0.0, 0.0), (5.0, 0.0), (50.0, 0.0), (1.0, 300.0)])
def test_layernorm_fold_precision_under_offsets(L, mean_over_std, outlier):
    """The folded form computes rstd * (x . W'^T) - rstd * mean * c1: with a large row mean the two terms cancel.
    Rows with mean/std up to 50 and a 300-sigma outlier channel (the "massive activation" pattern of trained
    ViTs): the folded GEMM must stay as close to the fp32 LayerNorm + Linear as the separate
    hcir_layernorm_f16 + hcir_gemm_f16 path does (both are limited by one fp16 rounding of an operand)."""
    g = torch.Generator().manual_seed(int(mean_over_std * 10 + outlier))
    m, d, n, eps = 1280, 768, 768, 1e-6
    x = torch.randn(m, d, generator=g) + mean_over_std * (1.0 + 0.1 * torch.randn(m, 1, generator=g))
    if outlier:
        x[:, 7] += outlier
    x16 = x.half()
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.2 * torch.randn(d, generator=g)
    w = torch.randn(n, d, generator=g) * d ** -0.5
    b = torch.randn(n, generator=g)
    ref = (F.layer_norm(x16.double(), (d,), gamma.double(), beta.double(), eps) @ w.double().t() + b.double()).float()
    xd = x16.cuda()
    # separate path
    ln = torch.empty((m, d), dtype=torch.float16, device="cuda")
    out_sep = torch.empty((m, n), dtype=torch.float16, device="cuda")
    assert L.hcir_layernorm_f16(xd.data_ptr(), 1, m, d, d, gamma.cuda().data_ptr(), beta.cuda().data_ptr(), eps,
                                ln.data_ptr(), d, _st()) == 0
    w16 = w.half().cuda()
    assert L.hcir_gemm_f16(ln.data_ptr(), d, w16.data_ptr(), d, b.cuda().data_ptr(), None, m, n, d, 0,
                           out_sep.data_ptr(), n, _st()) == 0
    # folded path: statistics of the stored rows, W' = fp16(gamma o W)
    xs = x16.double()
    stats = torch.stack([xs.mean(1), (xs.var(1, unbiased=False) + eps).rsqrt()], 1).float().cuda()
    wg = (w.double() * gamma.double()[None, :]).half()
    c1 = wg.double().sum(1).float().cuda()
    c2 = (w.double() @ beta.double() + b.double()).float().cuda()
    out_fold = torch.empty((m, n), dtype=torch.float16, device="cuda")
    assert L.hcir_gemm_f16_fused(xd.data_ptr(), d, wg.cuda().data_ptr(), d, c2.data_ptr(), None, m, n, d, 0,
                                 out_fold.data_ptr(), n, stats.data_ptr(), c1.data_ptr(), None, _st()) == 0
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    e_sep = (out_sep.float().cpu() - ref).abs().max().item() / scale
    e_fold = (out_fold.float().cpu() - ref).abs().max().item() / scale
    print(f"mean/std {mean_over_std}, outlier {outlier}: max err / max|ref|  separate {e_sep:.2e}  folded {e_fold:.2e}")
    assert e_sep <= 4e-3
    assert e_fold <= max(4e-3, 3.0 * e_sep)
