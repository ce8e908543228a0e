"""float64 stand-ins on the CPU for the op surface hcir.vit_train.VitTrainer walks (hcir.train_ops): the same names and
signatures, plain torch on the same buffer layouts - row-padded matrices of which only the first `rows` rows are read
or written, qkv as [B][T][3][H][64], lse in the log2 domain as include/hcir.h defines it.  gemm_tn contracts over ALL
stored rows, as the kernel does: a pad row that is not zero is seen.  Test infrastructure (test_vit_walk_host.py)."""
import math

import torch
import torch.nn.functional as F

DEVICE_TYPE, ACT, ACC = "cpu", torch.float64, torch.float64
_LOG2E = math.log2(math.e)


def _rows(t, rows, d, pitch):
    """[rows, d] view of a buffer whose rows lie `pitch` elements apart."""
    return torch.as_strided(t, (rows, d), (pitch, 1))


def patch_embed(x, ps, w16, bias, cls, pos, pos_mult, tok):
    b, c, hh, ww = x.shape
    gh, gw, d = hh // ps, ww // ps, w16.shape[0]
    patches = x.reshape(b, c, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(b, gh * gw, -1)
    out = tok[: b * (gh * gw + 1)].view(b, gh * gw + 1, d)
    out[:, 0] = cls + pos_mult * pos[0]
    out[:, 1:] = patches @ w16.t() + bias + pos_mult * pos[1:]


def layernorm(x, rows, gamma, beta, eps, y):
    y[:rows] = F.layer_norm(x[:rows], (gamma.numel(),), gamma, beta, eps)


def gemm(a, w, bias, rows, out, resid=None):
    acc = a[:rows] @ w.t()
    if bias is not None:
        acc = acc + bias
    out[:rows] = acc if resid is None else acc + resid[:rows]


def gelu_fwd(u, rows=None, out=None):
    out = torch.empty_like(u) if out is None else out
    rows = u.shape[0] if rows is None else rows
    out[:rows] = F.gelu(u[:rows])
    return out


def fc1_gelu(x, w, bias, rows, u, h):
    gemm(x, w, bias, rows, u)
    gelu_fwd(u, rows, h)


def cls_head(tok, b, t, gamma, beta, eps, out):
    d = gamma.numel()
    out.copy_(F.layer_norm(_rows(tok, b, d, t * d), (d,), gamma, beta, eps))


def add_to_f16(a, b=None, out=None, rows=None):
    rows = a.shape[0] if rows is None else rows
    out[:rows] = a[:rows] if b is None else a[:rows] + b[:rows]
    return out


def _put(dst, val, accumulate):
    dst.copy_(dst + val if accumulate else val)


def layernorm_bwd(x, dy16, gamma, eps, dres_in, dres_out, dgamma, dbeta, accumulate=True, rows=None, ldx=None, ldr=None,
                  dres16=None, dres_colsum=None):
    d = gamma.numel()
    rows = dy16.shape[0] if rows is None else rows
    xr, dy = _rows(x, rows, d, d if ldx is None else ldx), dy16[:rows]
    mean, var = xr.mean(1, keepdim=True), xr.var(1, unbiased=False, keepdim=True)
    xhat = (xr - mean) * torch.rsqrt(var + eps)
    g = dy * gamma
    dx = torch.rsqrt(var + eps) * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    ldr = d if ldr is None else ldr
    out = dx if dres_in is None else _rows(dres_in, rows, d, ldr) + dx
    _rows(dres_out, rows, d, ldr).copy_(out)
    _put(dgamma, (dy * xhat).sum(0), accumulate)
    _put(dbeta, dy.sum(0), accumulate)
    if dres16 is not None:
        dres16[:rows] = out
        if dres_colsum is not None:
            dres_colsum.copy_(out.sum(0))


def gelu_bwd_colsum(u, dh, du, colsum_out, rows=None, accumulate=False):
    rows = u.shape[0] if rows is None else rows
    ur = u[:rows]
    dgelu = 0.5 * (1 + torch.erf(ur / math.sqrt(2))) + ur * torch.exp(-0.5 * ur * ur) / math.sqrt(2 * math.pi)
    du[:rows] = dh[:rows] * dgelu
    _put(colsum_out, du[:rows].sum(0), accumulate)


def colsum(x16, out, accumulate=True, rows=None):
    _put(out, x16[: x16.shape[0] if rows is None else rows].sum(0), accumulate)


def gemm_tn(a16, b16, dw, accumulate=True):
    _put(dw, a16.t() @ b16, accumulate)


def _qkv(qkv, b, t, heads):
    """q, k, v as [b, heads, t, 64] views of the packed [b][t][3][heads][64] buffer."""
    return qkv[: b * t].view(b, t, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)


def _attn_fwd(qkv, b, t, heads, scale, out, lse, nq):
    q, k, v = _qkv(qkv, b, t, heads)
    s = scale * q[:, :, :nq] @ k.transpose(-1, -2)
    lse.view(b, heads, nq).copy_(torch.logsumexp(s, -1) * _LOG2E)
    out[: b * nq] = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(b * nq, heads * 64)


def _attn_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv, nq):
    q, k, v = _qkv(qkv, b, t, heads)
    q = q[:, :, :nq]
    o, do = (x[: b * nq].view(b, nq, heads, 64).transpose(1, 2) for x in (out, d_out))
    p = torch.exp2(scale * _LOG2E * q @ k.transpose(-1, -2) - lse.view(b, heads, nq, 1))
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    dq = torch.zeros(b, heads, t, 64, dtype=qkv.dtype)
    dq[:, :, :nq] = scale * ds @ k
    d3 = torch.stack((dq, scale * ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do))        # [3, b, heads, t, 64]
    d_qkv[: b * t] = d3.permute(1, 3, 0, 2, 4).reshape(b * t, 3 * heads * 64)


def attn_fwd_lse(qkv, b, t, heads, scale, out, lse):
    _attn_fwd(qkv, b, t, heads, scale, out, lse, t)


def attn_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv):
    _attn_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv, t)


def attn_cls_fwd_lse(qkv, b, t, heads, scale, out, lse):
    _attn_fwd(qkv, b, t, heads, scale, out, lse, 1)


def attn_cls_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv):
    _attn_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv, 1)
