"""The four kernels of csrc/mim.hip on an MI355X against float64 / exact references, with the bounds derived in
tests/_mim_ref.py (read there how each follows from the kernel's arithmetic).  Every case prints its worst
error / bound (`mim-err ...` lines, collected in profiles/mim_errors.txt).  No case feeds a kernel an index outside
its range: the in-kernel guard is a safety net, not a feature with a test that provokes it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mim_ref as mref

pytestmark = pytest.mark.gpu

SHAPES = [(3, 17, 256, torch.float16), (2, 5, 64, torch.float32), (2, 197, 768, torch.float16)]
_ids = lambda s: f"{s[0]}x{s[1]}x{s[2]}-{'f16' if s[3] == torch.float16 else 'f32'}"


def _mask(kind, b, t, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(b, t, dtype=torch.uint8)
    if kind == "patches":
        m[:, 1:] = 1
    elif kind == "all":
        m[:] = 1
    elif kind == "random":
        _, idx = mref.random_token_mask(torch.rand(b, t, generator=g), 0.75)
        m.scatter_(1, idx, 1)
    elif kind == "first_share":          # masked rows in the first rows of image 0 only
        m[0, 1:min(t, 41)] = 1
    else:
        assert kind == "none"
    return m


@pytest.mark.parametrize("pos_mult", [1.0, 2.0])
@pytest.mark.parametrize("kind", ["none", "patches", "all", "random"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_mask_tokens(hcir_built, shape, kind, pos_mult):
    from hcir import train_ops as ops
    b, t, d, dt = shape
    g = torch.Generator().manual_seed(b * t + d)
    tok = torch.randn(b * t + 3, d, generator=g).to(dt)          # three rows behind the tokens: never touched
    mt, pos = 0.02 * torch.randn(d, generator=g), 0.02 * torch.randn(t, d, generator=g)
    mask = _mask(kind, b, t)
    out = tok.cuda()
    ops.mim_mask_tokens(out, b, t, mask.cuda(), mt.cuda(), pos.cuda(), pos_mult)
    out = out.cpu()
    mk = torch.cat([mask.reshape(-1).bool(), torch.zeros(3, dtype=torch.bool)])
    assert torch.equal(out[~mk].view(torch.int16 if dt == torch.float16 else torch.int32),
                       tok[~mk].view(torch.int16 if dt == torch.float16 else torch.int32))
    if kind == "none":
        return
    exact = (mt.double() + pos_mult * pos.double()).expand(b, t, d).reshape(b * t, d)[mask.reshape(-1).bool()].numpy()
    err = np.abs(out[mk].double().numpy() - exact)
    ratio = float(np.max(err / mref.mask_token_bound(exact, dt == torch.float16)))
    print(f"mim-err mask_tokens {_ids(shape)} {kind} pos_mult={pos_mult:g}: {ratio:.3f}")
    assert ratio <= 1.0


# "first_share": (2, 197, 768) runs in seven workgroup shares of 57 rows; only the first holds masked rows
@pytest.mark.parametrize("shape,kind", [(s, k) for s in SHAPES for k in ("none", "patches", "all", "random")]
                         + [(SHAPES[2], "first_share")], ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_mask_bwd(hcir_built, shape, kind):
    from hcir import train_ops as ops
    b, t, d, _ = shape
    m, npat = b * t, b * (t - 1)
    if kind == "first_share":
        assert mref.bwd_plan(m) == (7, 57)
    g = torch.Generator().manual_seed(m + d)
    dtok = 3e-3 * torch.randn(m + 13, d, generator=g)              # rows behind b t: never read
    mask = _mask(kind, b, t, 1)
    pad = 5
    outs = []
    for _ in range(2):
        dpatch = torch.full((npat + pad, d), 7.0, dtype=torch.float16).cuda()
        gmt = torch.full((d,), float("nan")).cuda()
        ops.mim_mask_bwd(dtok.cuda(), b, t, mask.cuda(), gmt, dpatch)
        outs.append((gmt.cpu(), dpatch.cpu()))
    (gmt, dpatch), (gmt2, dpatch2) = outs
    assert torch.equal(gmt.view(torch.int32), gmt2.view(torch.int32)) and torch.equal(dpatch.view(torch.int16),
                                                                                      dpatch2.view(torch.int16))
    rows = dtok[:m].view(b, t, d)
    mk = mask.bool()
    want = torch.where(mk[:, 1:, None], torch.zeros(()), rows[:, 1:]).to(torch.float16).reshape(npat, d)
    assert torch.equal(dpatch[:npat].view(torch.int16), want.view(torch.int16))       # +0 rows by their bits
    assert (dpatch[npat:] == 7.0).all()
    terms = rows[mk].double().numpy()
    exact, scale = terms.sum(0), np.abs(terms).sum(0)
    err = np.abs(gmt.double().numpy() - exact)
    if kind == "none":
        assert not gmt.any()
        return
    bound = mref.gamma(mref.g_mask_token_k(m)) * scale
    ratio = float(np.max(err / bound))
    emu = mref.emulate_mask_bwd(dtok[:m].numpy(), mask.reshape(-1).numpy())
    print(f"mim-err mask_bwd {_ids(shape)} {kind}: {ratio:.3f}   (bit-equal to the fp32 emulation: "
          f"{bool(np.array_equal(emu, gmt.numpy()))})")
    assert ratio <= 1.0


def _image_for(n, ps, b, g, f16_channel0=False):
    """Images [b, 3, gh ps, gw ps] with gh != gw and at least n patches, and n distinct patch tokens per image in
    shuffled order (lightly's idx_mask: 1 + patch)."""
    gw = max(2, int(np.ceil(np.sqrt(n))) + 1)
    gh = max(1, -(-n // gw))
    img = torch.randn(b, 3, gh * ps, gw * ps, generator=g)
    if f16_channel0:
        img[:, 0] = img[:, 0].half().float()
    idx = torch.stack([torch.randperm(gh * gw, generator=g)[:n] + 1 for _ in range(b)])
    return img, idx


@pytest.mark.parametrize("size", [(64, 64), (32, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ps", [8, 16])
def test_patch_targets(hcir_built, ps, size):
    from hcir import train_ops as ops
    g = torch.Generator().manual_seed(ps + size[1])
    b = 3
    img = torch.randn(b, 3, *size, generator=g)
    seq = (size[0] // ps) * (size[1] // ps) + 1
    _, idx = mref.random_token_mask(torch.rand(b, seq, generator=g), 0.75)
    out = ops.mim_patch_targets(img.cuda(), idx.cuda(), ps).cpu()
    want = mref.get_at_index(mref.patchify(img, ps), idx - 1).reshape(-1, 3 * ps * ps)
    assert out.shape == want.shape and torch.equal(out.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("p", [192, 768])
@pytest.mark.parametrize("rows", [(1, 1), (3, 13), (1, 151), (11, 100)], ids=lambda r: f"rows={r[0] * r[1]}")
def test_l1_fwd(hcir_built, rows, p):
    from hcir import train_ops as ops
    b, n = rows
    ps = {192: 8, 768: 16}[p]
    if b * n > mref.L1_BLOCKS:
        assert mref.l1_plan(b * n)[1] == 2                 # above one row per workgroup: shares of two rows
    g = torch.Generator().manual_seed(b * n + p)
    img, idx = _image_for(n, ps, b, g, f16_channel0=True)
    target = mref.get_at_index(mref.patchify(img, ps), idx - 1).reshape(b * n, p)
    pred = (target + 0.5 * torch.randn(target.shape, generator=g)).half()
    # planted on channel-0 elements (fp16-representable targets): equal, one fp16 ulp above, one below
    flat, tflat = pred.view(-1), target.reshape(-1)
    cand = torch.arange(0, flat.numel(), 3)
    pick = cand[torch.randperm(cand.numel(), generator=g)[: min(cand.numel(), 60)]]
    eq, up, dn = pick[0::3], pick[1::3], pick[2::3]
    t16 = tflat.half()
    assert torch.equal(t16[pick].float(), tflat[pick])
    flat[eq] = t16[eq]
    flat[up] = torch.from_numpy(np.nextafter(t16[up].numpy(), np.float16(np.inf)))
    flat[dn] = torch.from_numpy(np.nextafter(t16[dn].numpy(), np.float16(-np.inf)))
    outs = []
    for _ in range(2):
        loss, sgn = ops.mim_l1_fwd(pred.cuda(), img.cuda(), idx.cuda(), ps)
        outs.append((loss.cpu(), sgn.cpu()))
    (loss, sgn), (loss2, sgn2) = outs
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(sgn.view(torch.int16),
                                                                                        sgn2.view(torch.int16))
    diff = pred.double() - target.double()
    want = torch.sign(diff).to(torch.float16)
    assert sgn.shape[0] == (b * n + 63) // 64 * 64 and not sgn[b * n:].any()
    assert torch.equal(sgn[: b * n].view(torch.int16), want.view(torch.int16))
    sf = sgn[: b * n].reshape(-1)
    assert (sf[eq] == 0).all() and (sf[up] == 1).all() and (sf[dn] == -1).all()
    exact = diff.abs().mean().item()
    bound = mref.gamma(mref.l1_k(b * n, p)) * exact
    ratio = abs(loss.double().item() - exact) / bound
    emu = mref.emulate_l1(pred.numpy(), target.numpy())
    print(f"mim-err l1_fwd rows={b * n} P={p}: {ratio:.3f}   (bit-equal to the fp32 emulation: "
          f"{bool(emu == loss.numpy())})")
    assert ratio <= 1.0


def test_l1_fwd_refuses_p_588(hcir_built):
    """P = 3 * 14 * 14 is no multiple of 8: no slow path, HCIR_ERR_UNSUPPORTED before anything is launched."""
    from hcir import _lib
    L = _lib.lib()
    img = torch.randn(1, 3, 28, 28).cuda()
    idx = torch.tensor([[1, 3]]).cuda()
    pred = torch.zeros(2, 588, dtype=torch.float16).cuda()
    loss, sgn, ws = torch.full((), 5.0).cuda(), torch.full((2, 588), 5.0, dtype=torch.float16).cuda(), \
        torch.zeros(64).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rc = L.hcir_mim_l1_fwd(pred.data_ptr(), img.data_ptr(), 1, 3, 28, 28, 14, idx.data_ptr(), 2, loss.data_ptr(),
                           sgn.data_ptr(), ws.data_ptr(), 256, st)
    assert rc == _lib.ERR_UNSUPPORTED
    out = torch.empty(2, 588).cuda()
    assert L.hcir_mim_patch_targets(img.data_ptr(), 1, 3, 28, 28, 14, idx.data_ptr(), 2, out.data_ptr(),
                                    st) == _lib.ERR_UNSUPPORTED
    tok = torch.zeros(4, 12).cuda()
    assert L.hcir_mim_mask_tokens(tok.data_ptr(), _lib.F32, 2, 2, 12, idx.data_ptr(), tok.data_ptr(), tok.data_ptr(),
                                  1.0, st) == _lib.ERR_UNSUPPORTED
    assert L.hcir_mim_mask_bwd_workspace_bytes(2, 2, 12) == 0
    torch.cuda.synchronize()
    assert float(loss) == 5.0 and (sgn == 5.0).all()
