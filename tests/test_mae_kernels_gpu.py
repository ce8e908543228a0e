"""The kernels of csrc/mae.hip on an MI355X against exact / float64 references, with the bounds derived in
tests/_mae_ref.py (read there how each follows from the kernel's arithmetic).  The token kernels must be EXACT: the
gather and the scatter are copies, the decoder input is asked bit for bit against the same two roundings in torch on
the CPU (and against its derived bound), the decoder-input backward's fp16 rows bit for bit and its mask-token sum
within gamma_k sum|terms|.  The MSE kernel: every difference element and the loss within their bounds.  Every case
prints its worst error / bound (`mae-err ...` lines, collected in profiles/mae_errors.txt).  No case feeds a kernel an
index outside its range: the in-kernel guard is a safety net, not a feature with a test that provokes it.

Index tables: "random" is lightly's pair at ratio 0.75 in shuffled (non-sorted) order; "cls_only" keeps the class token
alone (k = 1, everything else masked); "all_kept" masks nothing (k = t) - the gather and the scatter then see the
identity permuted, the decoder input has no mask-token row and g_mask_token is +0."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mae_ref as aref

pytestmark = pytest.mark.gpu

SHAPES = [(3, 17, 256), (2, 197, 512), (5, 33, 256)]     # (b, t, d): 33 tokens = one row past a 32-row workgroup
KINDS = ["random", "cls_only", "all_kept"]
_ids = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else s
_i16 = lambda x: x.view(torch.int16)
_i32 = lambda x: x.view(torch.int32)


def _pad64(m):
    return (m + 63) // 64 * 64


def _idx_keep(kind, b, t, seed=0):
    g = torch.Generator().manual_seed(seed + t)
    if kind == "cls_only":
        return torch.zeros(b, 1, dtype=torch.int64)
    if kind == "all_kept":
        return torch.stack([torch.randperm(t, generator=g) for _ in range(b)])
    keep, _ = aref.random_token_mask(torch.rand(b, t, generator=g), 0.75)
    return torch.stack([row[torch.randperm(row.numel(), generator=g)] for row in keep]).contiguous()


def _index(idx, d):
    return idx.unsqueeze(-1).expand(-1, -1, d)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gather_rows(hcir_built, shape, kind):
    from hcir import train_ops as ops
    b, t, d = shape
    idx = _idx_keep(kind, b, t)
    k = idx.shape[1]
    tok = torch.randn(_pad64(b * t), d, generator=torch.Generator().manual_seed(b * t + d)).half()
    out = torch.full((_pad64(b * k), d), float("nan"), dtype=torch.float16).cuda()
    ops.mae_gather_rows(tok.cuda(), b, t, idx.cuda(), out)
    out = out.cpu()
    want = torch.gather(tok[: b * t].view(b, t, d), 1, _index(idx, d)).reshape(b * k, d)
    assert torch.equal(_i16(out[: b * k]), _i16(want))
    assert torch.equal(_i16(out[b * k:]), torch.zeros_like(_i16(out[b * k:])))      # pad rows: +0, written by the kernel


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_scatter_rows(hcir_built, shape, kind):
    from hcir import train_ops as ops
    b, t, d = shape
    idx = _idx_keep(kind, b, t, 1)
    k = idx.shape[1]
    comp = torch.randn(_pad64(b * k), d, generator=torch.Generator().manual_seed(k + d))
    dtok = torch.full((b * t + 3, d), float("nan")).cuda()                          # three rows behind: never touched
    ops.mae_scatter_rows(comp.cuda(), b, t, idx.cuda(), dtok)
    dtok = dtok.cpu()
    want = torch.zeros(b, t, d).scatter_(1, _index(idx, d), comp[: b * k].view(b, k, d)).view(b * t, d)
    assert torch.equal(_i32(dtok[: b * t]), _i32(want))                             # every row written, zeros as +0
    assert bool(torch.isnan(dtok[b * t:]).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_decoder_input(hcir_built, shape, kind):
    from hcir import train_ops as ops
    b, t, d = shape
    idx = _idx_keep(kind, b, t, 2)
    k = idx.shape[1]
    g = torch.Generator().manual_seed(b + t + d)
    embed = (0.7 * torch.randn(_pad64(b * k), d, generator=g)).half()
    mt, pos = 0.02 * torch.randn(d, generator=g), torch.rand(t, d, generator=g) * 2 - 1
    x = torch.full((b * t + 3, d), float("nan"), dtype=torch.float16).cuda()
    ops.mae_decoder_input(embed.cuda(), b, t, idx.cuda(), mt.cuda(), pos.cuda(), x)
    x = x.cpu()
    rows32 = mt.view(1, 1, d).repeat(b, t, 1).scatter_(1, _index(idx, d), embed[: b * k].float().view(b, k, d))
    want = (rows32 + pos).half().view(b * t, d)                                     # one fp32 add, one rounding to fp16
    assert torch.equal(_i16(x[: b * t]), _i16(want))
    assert bool(torch.isnan(x[b * t:]).all())
    rows64 = mt.double().view(1, 1, d).repeat(b, t, 1).scatter_(1, _index(idx, d),
                                                                 embed[: b * k].double().view(b, k, d))
    exact = (rows64 + pos.double()).view(b * t, d).numpy()
    ratio = float(np.max(np.abs(x[: b * t].double().numpy() - exact) / aref.f16_of_f32_sum_bound(exact)))
    print(f"mae-err decoder_input {_ids(shape)} {kind}: {ratio:.3f}")
    assert ratio <= 1.0


# (300, 5, 64): 256 shares of two images, the last 106 of them empty
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES + [(300, 5, 64)], ids=_ids)
def test_decoder_input_bwd(hcir_built, shape, kind):
    from hcir import train_ops as ops
    b, t, d = shape
    idx = _idx_keep(kind, b, t, 3)
    k = idx.shape[1]
    dres = 3e-3 * torch.randn(b * t + 13, d, generator=torch.Generator().manual_seed(b * t + d))   # rows behind: never read
    outs = []
    for _ in range(2):
        demb = torch.full((_pad64(b * k) + 5, d), 7.0, dtype=torch.float16).cuda()
        gmt = torch.full((d,), float("nan")).cuda()
        ops.mae_decoder_input_bwd(dres.cuda(), b, t, idx.cuda(), demb, gmt)
        outs.append((gmt.cpu(), demb.cpu()))
    (gmt, demb), (gmt2, demb2) = outs
    assert torch.equal(_i32(gmt), _i32(gmt2)) and torch.equal(_i16(demb), _i16(demb2))
    rows = dres[: b * t].view(b, t, d)
    want = torch.gather(rows, 1, _index(idx, d)).half().reshape(b * k, d)
    assert torch.equal(_i16(demb[: b * k]), _i16(want))
    assert bool((demb[b * k:] == 7.0).all())                                        # rows past b k: not touched
    kept = torch.zeros(b, t, dtype=torch.bool).scatter_(1, idx, True)
    if kind == "all_kept":
        assert torch.equal(_i32(gmt), torch.zeros(d, dtype=torch.int32))
        return
    terms = rows[~kept].double().numpy()
    exact, scale = terms.sum(0), np.abs(terms).sum(0)
    bound = aref.gamma(aref.g_mask_token_k(b, t)) * scale
    ratio = float(np.max(np.abs(gmt.double().numpy() - exact) / bound))
    emu = aref.emulate_decoder_input_bwd(dres[: b * t].numpy(), kept.reshape(-1).numpy(), b, t)
    print(f"mae-err decoder_input_bwd g_mask_token {_ids(shape)} {kind}: {ratio:.3f}   (bit-equal to the fp32 "
          f"emulation: {bool(np.array_equal(emu, gmt.numpy()))})")
    assert ratio <= 1.0


def _image_for(n, ps, b, g):
    """Images [b, 3, gh ps, gw ps] with gh != gw and at least n patches, and n distinct patch tokens per image in
    shuffled order (lightly's idx_mask: 1 + patch)."""
    gw = max(2, int(np.ceil(np.sqrt(n))) + 1)
    gh = max(1, -(-n // gw))
    img = torch.randn(b, 3, gh * ps, gw * ps, generator=g)
    idx = torch.stack([torch.randperm(gh * gw, generator=g)[:n] + 1 for _ in range(b)])
    return img, idx


# rows = b n: 39 and 151 are no multiples of 64; 1100 rows run two rows per workgroup; ps 8: P = 192 < one pass of 2048
@pytest.mark.parametrize("b,n,ps", [(3, 13, 16), (1, 1, 16), (1, 151, 8), (2, 64, 16), (2, 550, 8)])
def test_mse_fwd(hcir_built, b, n, ps):
    from hcir import train_ops as ops
    g = torch.Generator().manual_seed(b * n + ps)
    img, idx = _image_for(n, ps, b, g)
    p, rows = 3 * ps * ps, b * n
    target = aref.get_at_index(aref.patchify(img, ps), idx - 1).reshape(rows, p)
    pred = (target + 0.5 * torch.randn(rows, p, generator=g)).half()
    pred[0, :8] = target[0, :8].half()                                              # some differences tiny or zero
    pad = torch.full((_pad64(rows) - rows + 3, p), 5.0, dtype=torch.float16)          # rows behind pred: never read
    outs = []
    for _ in range(2):
        loss, diff = ops.mae_mse_fwd(torch.cat([pred, pad]).cuda(), img.cuda(), idx.cuda(), ps)
        outs.append((loss.cpu(), diff.cpu()))
    (loss, diff), (loss2, diff2) = outs
    assert torch.equal(_i32(loss.reshape(1)), _i32(loss2.reshape(1))) and torch.equal(_i16(diff), _i16(diff2))
    assert tuple(diff.shape) == (_pad64(rows), p) and loss.dim() == 0 and loss.dtype == torch.float32
    assert torch.equal(_i16(diff[rows:]), torch.zeros_like(_i16(diff[rows:])))
    want16 = (pred.float() - target).half()                                         # the same two roundings on the CPU
    assert torch.equal(_i16(diff[:rows]), _i16(want16))
    exact = pred.double().numpy() - target.double().numpy()
    dratio = float(np.max(np.abs(diff[:rows].double().numpy() - exact) / aref.f16_of_f32_sum_bound(exact)))
    terms = exact ** 2
    bound = aref.gamma(aref.mse_k(rows, p)) * terms.mean()
    lratio = abs(float(loss) - terms.mean()) / bound
    emu = aref.emulate_mse(pred.numpy(), target.numpy()) if rows * p <= 120000 else None
    print(f"mae-err mse_fwd rows {rows} P {p}: diff {dratio:.3f} loss {lratio:.3f}   (bit-equal to the fp32 emulation: "
          f"{None if emu is None else bool(emu == loss.numpy())})")
    assert dratio <= 1.0 and lratio <= 1.0
