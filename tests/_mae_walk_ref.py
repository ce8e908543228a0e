"""The op surface of the MAE walk (hcir.vit_train.MaeTrainer) as float64 stand-ins on the CPU: everything of
tests/_mim_walk_ref.py, the full-row attention pair restated for ANY head dim (the stand-ins of tests/_vit_walk_ref.py
fix 64; the MAE decoder has 32 - the head dim comes from the packed buffer's width, as in hcir.train_ops), and the ops
of csrc/mae.hip on the same buffer layouts: compact buffers [pad64(b k), d] whose pad rows the gather WRITES as zero
(the walk hands it uninitialised memory) and which the decoder-input backward must not touch, a token stream
[pad64(b t), d] of which the first b t rows are live.  Test infrastructure (test_mae_host.py)."""
import torch

from _mim_walk_ref import *  # noqa: F401,F403  (the stand-in surface is the module's namespace)
from _mim_walk_ref import ACC, ACT, DEVICE_TYPE  # noqa: F401
from _vit_walk_ref import _LOG2E


def _qkv(qkv, b, t, heads):
    hd = qkv.shape[1] // (3 * heads)
    return qkv[: b * t].view(b, t, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)


def attn_fwd_lse(qkv, b, t, heads, scale, out, lse):
    q, k, v = _qkv(qkv, b, t, heads)
    s = scale * q @ k.transpose(-1, -2)
    lse.view(b, heads, t).copy_(torch.logsumexp(s, -1) * _LOG2E)
    out[: b * t] = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b * t, -1)


def attn_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv):
    q, k, v = _qkv(qkv, b, t, heads)
    hd = q.shape[-1]
    o, do = (x[: b * t].view(b, t, heads, hd).transpose(1, 2) for x in (out, d_out))
    p = torch.exp2(scale * _LOG2E * q @ k.transpose(-1, -2) - lse.view(b, heads, t, 1))
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    d3 = torch.stack((scale * ds @ k, scale * ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do))
    d_qkv[: b * t] = d3.permute(1, 3, 0, 2, 4).reshape(b * t, 3 * heads * hd)


def _index(idx, d):
    return idx.unsqueeze(-1).expand(-1, -1, d)


def mae_gather_rows(tok, b, t, idx, out):
    k, d = idx.shape[1], tok.shape[1]
    out[: b * k] = torch.gather(tok[: b * t].view(b, t, d), 1, _index(idx, d)).reshape(b * k, d)
    out[b * k:] = 0


def mae_scatter_rows(comp, b, t, idx, dtok):
    k, d = idx.shape[1], comp.shape[1]
    rows = torch.zeros(b, t, d, dtype=dtok.dtype)
    rows.scatter_(1, _index(idx, d), comp[: b * k].view(b, k, d))
    dtok[: b * t] = rows.view(b * t, d)


def mae_decoder_input(embed, b, t, idx_keep, mask_token, pos, x):
    k, d = idx_keep.shape[1], mask_token.numel()
    rows = mask_token.view(1, 1, d).repeat(b, t, 1)
    rows.scatter_(1, _index(idx_keep, d), embed[: b * k].view(b, k, d))
    x[: b * t] = (rows + pos.view(1, t, d)).view(b * t, d)


def mae_decoder_input_bwd(dres, b, t, idx_keep, d_embed, g_mask_token):
    k, d = idx_keep.shape[1], g_mask_token.numel()
    g = dres[: b * t].view(b, t, d)
    d_embed[: b * k] = torch.gather(g, 1, _index(idx_keep, d)).reshape(b * k, d)
    kept = torch.zeros(b, t, dtype=torch.bool)
    kept.scatter_(1, idx_keep, True)
    g_mask_token.copy_(g[~kept].sum(0))


def mae_mse_fwd(pred, img, idx, ps):
    b, n = idx.shape
    c, hh, ww = img.shape[1:]
    patches = img.reshape(b, c, hh // ps, ps, ww // ps, ps).permute(0, 2, 4, 3, 5, 1).reshape(b, -1, ps * ps * c)
    target = torch.gather(patches, 1, _index(idx - 1, patches.shape[-1])).reshape(b * n, -1)
    diff = torch.zeros_like(pred)
    diff[: b * n] = pred[: b * n] - target
    return (diff[: b * n] ** 2).mean(), diff
