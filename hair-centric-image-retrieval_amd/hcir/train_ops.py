"""hcir.train_ops — torch-tensor wrappers over the training half of the C ABI (include/hcir.h, "Training side").

The op surface of the ViT's training walk (hcir.vit_train: every launch of its forward and backward is one of these
functions, so a test can run the walk over stand-ins) and the two small losses of the HSimCLR step
(HP/src/pretrain_engine.py:681-751).  Every wrapper takes HIP-device tensors and raises otherwise: no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import HcirError, check
from .ops import _dev, _ptr, _stream, _ws

_XDT = {torch.float32: _lib.F32, torch.float16: _lib.F16}
# what a walk over these ops (hcir.vit_train) allocates: where, GEMM-operand dtype, accumulator / gradient dtype
DEVICE_TYPE, ACT, ACC = "cuda", torch.float16, torch.float32


def patch_embed(x: torch.Tensor, ps: int, w16: torch.Tensor, bias, cls, pos, pos_mult: float, tok) -> None:
    """tok[b][0] = cls + pos_mult pos[0];  tok[b][1 + p] = w16 . patch(b, p) + bias + pos_mult pos[1 + p]."""
    _dev(x, "x")
    b, c, hh, ww = x.shape
    check(_lib.lib().hcir_patch_embed(x.data_ptr(), b, c, hh, ww, ps, w16.data_ptr(), w16.shape[1], bias.data_ptr(),
                                      cls.data_ptr(), pos.data_ptr(), float(pos_mult), w16.shape[0], tok.data_ptr(),
                                      _XDT[tok.dtype], _stream(x)), "hcir_patch_embed")


def layernorm(x: torch.Tensor, rows: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, y: torch.Tensor) -> None:
    """y[:rows] = fp16(LayerNorm(x[:rows])) over contiguous rows of gamma.numel() elements."""
    _dev(x, "x")
    d = gamma.numel()
    check(_lib.lib().hcir_layernorm_f16(x.data_ptr(), _XDT[x.dtype], rows, d, d, gamma.data_ptr(), beta.data_ptr(),
                                        float(eps), y.data_ptr(), d, _stream(x)), "hcir_layernorm_f16")


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], rows: int, out: torch.Tensor,
         resid: Optional[torch.Tensor] = None) -> None:
    """out[:rows] = fp16(a[:rows] @ w^T + bias (+ resid[:rows]));  w fp16 [N, K] as stored, contiguous rows."""
    _dev(a, "a")
    n, k = w.shape
    epi = _lib.EPI_BIAS_F16 if resid is None else _lib.EPI_BIAS_RESID_F16
    check(_lib.lib().hcir_gemm_f16_resid(a.data_ptr(), k, w.data_ptr(), k, _ptr(bias), None, rows, n, k, epi,
                                         _ptr(resid), out.data_ptr(), n, _stream(a)), f"hcir_gemm_f16_resid({n}x{k})")


def fc1_gelu(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, rows: int, u: torch.Tensor, h: torch.Tensor) -> None:
    """u = fp16(x @ w^T + bias) (kept for the GELU backward) and h = fp16(gelu(.)): from one pass over the accumulators
    where the persistent kernel takes the shape, else a GEMM and a GELU pass over u."""
    n, k = w.shape
    L = _lib.lib()
    if L.hcir_gemm_fused_supported(rows, n, k):
        _dev(x, "x")
        check(L.hcir_gemm_f16_gelu_dual(x.data_ptr(), k, w.data_ptr(), k, _ptr(bias), rows, n, k, u.data_ptr(),
                                        h.data_ptr(), n, _stream(x)), "hcir_gemm_f16_gelu_dual")
    else:
        gemm(x, w, bias, rows, u)
        gelu_fwd(u, rows, h)


def cls_head(tok: torch.Tensor, b: int, t: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
             out: torch.Tensor) -> None:
    """out[b] = LayerNorm(tok[b][0]) for tok [b][t][d] (fp32 out)."""
    _dev(tok, "tok")
    check(_lib.lib().hcir_cls_head(tok.data_ptr(), _XDT[tok.dtype], b, t, gamma.numel(), gamma.data_ptr(),
                                   beta.data_ptr(), float(eps), 0, out.data_ptr(), None, _stream(tok)), "hcir_cls_head")


def gelu_fwd(u: torch.Tensor, rows: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gelu(u), or of the first `rows` rows of the matrix u, into `out` (allocated when None)."""
    _dev(u, "u")
    if u.dtype != torch.float16 or u.numel() % 8:
        raise HcirError("gelu_fwd expects a contiguous fp16 tensor with numel % 8 == 0")
    h = torch.empty_like(u) if out is None else out
    n = u.numel() if rows is None else rows * u.shape[1]
    check(_lib.lib().hcir_gelu_fwd_f16(u.data_ptr(), n, h.data_ptr(), _stream(u)), "hcir_gelu_fwd_f16")
    return h


def gelu_bwd(u: torch.Tensor, dh: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(u, "u")
    _dev(dh, "dh")
    if u.dtype != torch.float16 or dh.dtype != torch.float16 or u.shape != dh.shape or u.numel() % 8:
        raise HcirError("gelu_bwd expects two contiguous fp16 tensors of equal shape, numel % 8 == 0")
    du = torch.empty_like(u) if out is None else out
    check(_lib.lib().hcir_gelu_bwd_f16(u.data_ptr(), dh.data_ptr(), u.numel(), du.data_ptr(), _stream(u)),
          "hcir_gelu_bwd_f16")
    return du


def add_to_f16(a: torch.Tensor, b: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               rows: Optional[int] = None) -> torch.Tensor:
    """fp16(a + b) of fp32 tensors (b optional), or of the first `rows` rows of the matrices."""
    _dev(a, "a")
    if a.dtype != torch.float32 or a.numel() % 4:
        raise HcirError("add_to_f16 expects contiguous fp32, numel % 4 == 0")
    y = torch.empty(a.shape, dtype=torch.float16, device=a.device) if out is None else out
    n = a.numel() if rows is None else rows * a.shape[1]
    check(_lib.lib().hcir_add_f32_f16(a.data_ptr(), _ptr(b), n, y.data_ptr(), _stream(a)), "hcir_add_f32_f16")
    return y


def layernorm_bwd(x: torch.Tensor, dy16: torch.Tensor, gamma: torch.Tensor, eps: float,
                  dres_in: Optional[torch.Tensor], dres_out: torch.Tensor, dgamma: torch.Tensor, dbeta: torch.Tensor,
                  accumulate: bool = True, rows: Optional[int] = None, ldx: Optional[int] = None,
                  ldr: Optional[int] = None, dres16: Optional[torch.Tensor] = None,
                  dres_colsum: Optional[torch.Tensor] = None) -> None:
    """dres_out = dres_in + LayerNorm'(x)[dy16];  dgamma / dbeta (+)= the column reductions.
    x [rows, d] (fp32 or fp16, row pitch ldx), dy16 fp16 [rows, d], dres_* fp32 (row pitch ldr).
    dres16 (fp16 [rows, d]): also receives fp16(dres_out); dres_colsum (fp32 [d]): the column sums of that copy."""
    for t, n in ((x, "x"), (dy16, "dy"), (gamma, "gamma"), (dres_out, "dres_out"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _dev(t, n)
    d = gamma.numel()
    rows = dy16.shape[0] if rows is None else rows
    ldx = d if ldx is None else ldx
    ldr = d if ldr is None else ldr
    L = _lib.lib()
    nb = L.hcir_layernorm_bwd_blocks(rows)
    ws = _ws.get(x.device, nb * d * 12)
    if dres16 is not None:
        _dev(dres16, "dres16")
        if dres16.dtype != torch.float16 or dres16.stride(0) != d:
            raise HcirError("dres16: fp16 [rows, d], contiguous rows")
    check(L.hcir_layernorm_bwd_fused(x.data_ptr(), _XDT[x.dtype], rows, d, ldx, dy16.data_ptr(), d, gamma.data_ptr(),
                                     float(eps), _ptr(dres_in), dres_out.data_ptr(), ldr, dgamma.data_ptr(),
                                     dbeta.data_ptr(), int(accumulate), _ptr(dres16), d, _ptr(dres_colsum),
                                     ws.data_ptr(), ws.numel(), _stream(x)), "hcir_layernorm_bwd_fused")


def gelu_bwd_colsum(u: torch.Tensor, dh: torch.Tensor, du: torch.Tensor, colsum_out: torch.Tensor,
                    rows: Optional[int] = None, accumulate: bool = False) -> None:
    """du = dh * gelu'(u) over the first `rows` rows of [m, n] fp16 matrices, and colsum_out[n] (+)= sum_rows du."""
    for t, nm in ((u, "u"), (dh, "dh"), (du, "du"), (colsum_out, "colsum")):
        _dev(t, nm)
    if u.dtype != torch.float16 or dh.dtype != torch.float16 or du.dtype != torch.float16 or u.shape != dh.shape:
        raise HcirError("gelu_bwd_colsum expects fp16 matrices of equal shape")
    m = u.shape[0] if rows is None else rows
    n = u.shape[1]
    L = _lib.lib()
    ws = _ws.get(u.device, L.hcir_colsum_chunks(m) * n * 4)
    check(L.hcir_gelu_bwd_colsum_f16(u.data_ptr(), dh.data_ptr(), m, n, u.stride(0), du.data_ptr(),
                                     colsum_out.data_ptr(), int(accumulate), ws.data_ptr(), ws.numel(), _stream(u)),
          "hcir_gelu_bwd_colsum_f16")


def colsum(x16: torch.Tensor, out: torch.Tensor, accumulate: bool = True, rows: Optional[int] = None) -> None:
    """out[n] (+)= sum over rows of the fp16 matrix x16 [m, n]."""
    _dev(x16, "x")
    _dev(out, "out")
    m = x16.shape[0] if rows is None else rows
    n = x16.shape[1]
    L = _lib.lib()
    ws = _ws.get(x16.device, L.hcir_colsum_chunks(m) * n * 4)
    check(L.hcir_colsum_f16(x16.data_ptr(), m, n, x16.stride(0), out.data_ptr(), int(accumulate), ws.data_ptr(),
                            ws.numel(), _stream(x16)), "hcir_colsum_f16")


def gemm_tn(a16: torch.Tensor, b16: torch.Tensor, dw: torch.Tensor, accumulate: bool = True) -> None:
    """dw[N, K] (+)= a16[M, N]^T @ b16[M, K]   (fp16 operands, fp32 result).  M % 64 == 0 (the caller pads with zero
    rows), N % 256 == 0, K % 256 == 0."""
    for t, n in ((a16, "a"), (b16, "b"), (dw, "dw")):
        _dev(t, n)
    if a16.dtype != torch.float16 or b16.dtype != torch.float16 or dw.dtype != torch.float32:
        raise HcirError("gemm_tn: fp16 operands, fp32 output")
    m, n = a16.shape
    k = b16.shape[1]
    if b16.shape[0] != m or tuple(dw.shape) != (n, k):
        raise HcirError(f"gemm_tn shape mismatch: a {tuple(a16.shape)} b {tuple(b16.shape)} dw {tuple(dw.shape)}")
    L = _lib.lib()
    wsb = L.hcir_gemm_f16_tn_workspace_bytes(m, n, k)
    if wsb == 0:
        raise HcirError(f"gemm_tn unsupported shape M={m} N={n} K={k} (M % 64, N % 256, K % 256)")
    ws = _ws.get(a16.device, wsb)
    check(L.hcir_gemm_f16_tn(a16.data_ptr(), a16.stride(0), b16.data_ptr(), b16.stride(0), m, n, k, dw.data_ptr(),
                             dw.stride(0), int(accumulate), ws.data_ptr(), ws.numel(), _stream(a16)),
          "hcir_gemm_f16_tn")


def _head_dim(qkv: torch.Tensor, heads: int) -> int:
    """Head dim of a packed [rows, 3 * heads * hd] (or [b, t, 3 * heads * hd]) qkv buffer: its last axis; the C entry
    points decide which they support (64 and, for the full-row pair, 32)."""
    return qkv.shape[-1] // (3 * heads)


def attn_fwd_lse(qkv: torch.Tensor, b: int, t: int, heads: int, scale: float, out: torch.Tensor,
                 lse: torch.Tensor) -> None:
    check(_lib.lib().hcir_attn_fwd_lse(qkv.data_ptr(), b, t, heads, _head_dim(qkv, heads), float(scale),
                                       out.data_ptr(), lse.data_ptr(), _stream(qkv)), "hcir_attn_fwd_lse")


def attn_bwd(qkv: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, lse: torch.Tensor, b: int, t: int, heads: int,
             scale: float, d_qkv: torch.Tensor) -> None:
    check(_lib.lib().hcir_attn_bwd(qkv.data_ptr(), out.data_ptr(), d_out.data_ptr(), lse.data_ptr(), b, t, heads,
                                   _head_dim(qkv, heads), float(scale), d_qkv.data_ptr(), _stream(qkv)),
          "hcir_attn_bwd")


def attn_cls_fwd_lse(qkv: torch.Tensor, b: int, t: int, heads: int, scale: float, out: torch.Tensor,
                     lse: torch.Tensor) -> None:
    """attn_fwd_lse for the class-token query of every image: out [b, heads*64], lse [b, heads]."""
    check(_lib.lib().hcir_attn_cls_fwd_lse(qkv.data_ptr(), b, t, heads, _head_dim(qkv, heads), float(scale),
                                           out.data_ptr(), lse.data_ptr(), _stream(qkv)), "hcir_attn_cls_fwd_lse")


def attn_cls_bwd(qkv: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, lse: torch.Tensor, b: int, t: int,
                 heads: int, scale: float, d_qkv: torch.Tensor) -> None:
    """Its backward: d_qkv gets dK, dV of every token, dQ of token 0 and zero for the other tokens' dQ."""
    check(_lib.lib().hcir_attn_cls_bwd(qkv.data_ptr(), out.data_ptr(), d_out.data_ptr(), lse.data_ptr(), b, t, heads,
                                       _head_dim(qkv, heads), float(scale), d_qkv.data_ptr(), _stream(qkv)),
          "hcir_attn_cls_bwd")


# ---------------------------------------------------------------------------------------------------------------
# SimMIM (csrc/mim.hip): the two ops of the masked walk, the patch targets and the masked-patch L1 loss
# ---------------------------------------------------------------------------------------------------------------
def mim_mask_tokens(tok: torch.Tensor, b: int, t: int, mask: torch.Tensor, mask_token: torch.Tensor,
                    pos: torch.Tensor, pos_mult: float) -> None:
    """tok[b][k] = mask_token + pos_mult pos[k] where mask[b][k] != 0 (uint8 [b, t]); other rows untouched."""
    _dev(tok, "tok")
    _dev(mask, "mask")
    if mask.dtype != torch.uint8 or mask.numel() != b * t:
        raise HcirError("mim_mask_tokens: mask is a uint8 table [b, t]")
    d = mask_token.numel()
    check(_lib.lib().hcir_mim_mask_tokens(tok.data_ptr(), _XDT[tok.dtype], b, t, d, mask.data_ptr(),
                                          mask_token.data_ptr(), pos.data_ptr(), float(pos_mult), _stream(tok)),
          "hcir_mim_mask_tokens")


def mim_mask_bwd(dtok: torch.Tensor, b: int, t: int, mask: torch.Tensor, g_mask_token: torch.Tensor,
                 dpatch: torch.Tensor) -> None:
    """g_mask_token[d] = sum of the masked rows of dtok (fp32 [b t, d]); dpatch[b (t-1), d] = fp16 of the patch rows of
    dtok, +0 where masked."""
    for x, nm in ((dtok, "dtok"), (mask, "mask"), (g_mask_token, "g_mask_token"), (dpatch, "dpatch")):
        _dev(x, nm)
    if dtok.dtype != torch.float32 or dpatch.dtype != torch.float16 or mask.dtype != torch.uint8:
        raise HcirError("mim_mask_bwd: dtok fp32, dpatch fp16, mask uint8")
    d = g_mask_token.numel()
    if dpatch.shape[0] < b * (t - 1) or dtok.shape[0] < b * t or mask.numel() != b * t:
        raise HcirError("mim_mask_bwd: buffers shorter than the shape")
    L = _lib.lib()
    ws = _ws.get(dtok.device, L.hcir_mim_mask_bwd_workspace_bytes(b, t, d))
    check(L.hcir_mim_mask_bwd(dtok.data_ptr(), b, t, d, mask.data_ptr(), g_mask_token.data_ptr(), dpatch.data_ptr(),
                              ws.data_ptr(), ws.numel(), _stream(dtok)), "hcir_mim_mask_bwd")


def _mim_image_args(img: torch.Tensor, idx: torch.Tensor):
    _dev(img, "images")
    _dev(idx, "idx_mask")
    if img.dtype != torch.float32 or img.dim() != 4 or idx.dtype != torch.int64 or idx.dim() != 2 \
            or idx.shape[0] != img.shape[0]:
        raise HcirError("images fp32 [b, C, H, W] and idx_mask int64 [b, n]")
    return tuple(img.shape), idx.shape[1]


def mim_patch_targets(img: torch.Tensor, idx: torch.Tensor, ps: int) -> torch.Tensor:
    """patchify(img)[idx - 1] as fp32 [b n, C ps ps], lightly's element order (py, px, c)."""
    (b, c, h, w), n = _mim_image_args(img, idx)
    out = torch.empty((b * n, c * ps * ps), dtype=torch.float32, device=img.device)
    check(_lib.lib().hcir_mim_patch_targets(img.data_ptr(), b, c, h, w, ps, idx.data_ptr(), n, out.data_ptr(),
                                            _stream(img)), "hcir_mim_patch_targets")
    return out


def mim_l1_fwd(pred: torch.Tensor, img: torch.Tensor, idx: torch.Tensor, ps: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean |pred - patchify(img)[idx - 1]| as a 0-d fp32 tensor, sign(pred - target) as fp16 [pad64(b n), P] with
    zero pad rows: the operand the backward walk's weight-gradient GEMM takes); pred fp16, at least b n rows of P."""
    (b, c, h, w), n = _mim_image_args(img, idx)
    _dev(pred, "pred")
    p = c * ps * ps
    if pred.dtype != torch.float16 or pred.dim() != 2 or pred.shape[1] != p or pred.shape[0] < b * n:
        raise HcirError(f"mim_l1_fwd: pred fp16 [>= {b * n}, {p}], got {tuple(pred.shape)} {pred.dtype}")
    loss = torch.empty((), dtype=torch.float32, device=img.device)
    sgn = torch.empty(((b * n + 63) // 64 * 64, p), dtype=torch.float16, device=img.device)
    sgn[b * n:].zero_()
    L = _lib.lib()
    ws = _ws.get(img.device, L.hcir_mim_l1_workspace_bytes(b * n))
    check(L.hcir_mim_l1_fwd(pred.data_ptr(), img.data_ptr(), b, c, h, w, ps, idx.data_ptr(), n, loss.data_ptr(),
                            sgn.data_ptr(), ws.data_ptr(), ws.numel(), _stream(img)), "hcir_mim_l1_fwd")
    return loss, sgn


# ---------------------------------------------------------------------------------------------------------------
# MAE (csrc/mae.hip): the token kernels of the masked-encoder / decoder walk and the masked-patch MSE loss
# ---------------------------------------------------------------------------------------------------------------
def _mae_idx(idx: torch.Tensor, b: int, name: str) -> int:
    _dev(idx, name)
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != b or not idx.is_contiguous():
        raise HcirError(f"{name}: contiguous int64 [b, k]")
    return idx.shape[1]


def mae_gather_rows(tok: torch.Tensor, b: int, t: int, idx: torch.Tensor, out: torch.Tensor) -> None:
    """out[i k + j] = tok[i t + idx[i][j]] for fp16 tok [>= b t, d] -> fp16 out [pad64(b k), d], pad rows zero."""
    _dev(tok, "tok")
    _dev(out, "out")
    k, d = _mae_idx(idx, b, "idx"), tok.shape[1]
    if tok.dtype != torch.float16 or out.dtype != torch.float16 or tok.shape[0] < b * t \
            or tuple(out.shape) != ((b * k + 63) // 64 * 64, d):
        raise HcirError("mae_gather_rows: fp16 tok [>= b t, d] and fp16 out [pad64(b k), d]")
    check(_lib.lib().hcir_mae_gather_rows(tok.data_ptr(), b, t, d, idx.data_ptr(), k, out.data_ptr(), _stream(tok)),
          "hcir_mae_gather_rows")


def mae_scatter_rows(comp: torch.Tensor, b: int, t: int, idx: torch.Tensor, dtok: torch.Tensor) -> None:
    """dtok[i t + idx[i][j]] = comp[i k + j], every other row of the first b t of dtok zero (fp32, both)."""
    _dev(comp, "comp")
    _dev(dtok, "dtok")
    k, d = _mae_idx(idx, b, "idx"), comp.shape[1]
    if comp.dtype != torch.float32 or dtok.dtype != torch.float32 or comp.shape[0] < b * k or dtok.shape[0] < b * t \
            or dtok.shape[1] != d:
        raise HcirError("mae_scatter_rows: fp32 comp [>= b k, d] and fp32 dtok [>= b t, d]")
    check(_lib.lib().hcir_mae_scatter_rows(comp.data_ptr(), b, t, d, idx.data_ptr(), k, dtok.data_ptr(),
                                           _stream(comp)), "hcir_mae_scatter_rows")


def mae_decoder_input(embed: torch.Tensor, b: int, t: int, idx_keep: torch.Tensor, mask_token: torch.Tensor,
                      pos: torch.Tensor, x: torch.Tensor) -> None:
    """x[i t + tok] = fp16((tok kept at j ? embed[i k + j] : mask_token) + pos[tok]) for every token of every image."""
    for v, nm in ((embed, "embed"), (mask_token, "mask_token"), (pos, "pos"), (x, "x")):
        _dev(v, nm)
    k, d = _mae_idx(idx_keep, b, "idx_keep"), mask_token.numel()
    if embed.dtype != torch.float16 or x.dtype != torch.float16 or mask_token.dtype != torch.float32 \
            or pos.dtype != torch.float32 or embed.shape[0] < b * k or x.shape[0] < b * t or pos.numel() != t * d \
            or embed.shape[1] != d or x.shape[1] != d:
        raise HcirError("mae_decoder_input: fp16 embed [>= b k, d], fp32 mask_token [d] and pos [t, d], fp16 x [>= b t, d]")
    check(_lib.lib().hcir_mae_decoder_input(embed.data_ptr(), b, t, d, idx_keep.data_ptr(), k, mask_token.data_ptr(),
                                            pos.data_ptr(), x.data_ptr(), _stream(x)), "hcir_mae_decoder_input")


def mae_decoder_input_bwd(dres: torch.Tensor, b: int, t: int, idx_keep: torch.Tensor, d_embed: torch.Tensor,
                          g_mask_token: torch.Tensor) -> None:
    """d_embed[i k + j] = fp16(dres[i t + idx_keep[i][j]]) (rows past b k untouched); g_mask_token[d] = the sum of the
    rows of dres (fp32 [>= b t, d]) whose token is not kept."""
    for v, nm in ((dres, "dres"), (d_embed, "d_embed"), (g_mask_token, "g_mask_token")):
        _dev(v, nm)
    k, d = _mae_idx(idx_keep, b, "idx_keep"), g_mask_token.numel()
    if dres.dtype != torch.float32 or d_embed.dtype != torch.float16 or g_mask_token.dtype != torch.float32 \
            or dres.shape[0] < b * t or d_embed.shape[0] < b * k or dres.shape[1] != d or d_embed.shape[1] != d:
        raise HcirError("mae_decoder_input_bwd: fp32 dres [>= b t, d], fp16 d_embed [>= b k, d], fp32 g_mask_token [d]")
    L = _lib.lib()
    ws = _ws.get(dres.device, L.hcir_mae_decoder_input_bwd_workspace_bytes(b, d))
    check(L.hcir_mae_decoder_input_bwd(dres.data_ptr(), b, t, d, idx_keep.data_ptr(), k, d_embed.data_ptr(),
                                       g_mask_token.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dres)),
          "hcir_mae_decoder_input_bwd")


def mae_mse_fwd(pred: torch.Tensor, img: torch.Tensor, idx: torch.Tensor, ps: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean (pred - patchify(img)[idx - 1])^2 as a 0-d fp32 tensor, fp16(pred - target) as [pad64(b n), P] with zero
    pad rows: the operand the backward walk takes); pred fp16, at least b n rows of P."""
    (b, c, h, w), n = _mim_image_args(img, idx)
    _dev(pred, "pred")
    p = c * ps * ps
    if pred.dtype != torch.float16 or pred.dim() != 2 or pred.shape[1] != p or pred.shape[0] < b * n:
        raise HcirError(f"mae_mse_fwd: pred fp16 [>= {b * n}, {p}], got {tuple(pred.shape)} {pred.dtype}")
    loss = torch.empty((), dtype=torch.float32, device=img.device)
    diff = torch.empty(((b * n + 63) // 64 * 64, p), dtype=torch.float16, device=img.device)
    diff[b * n:].zero_()
    L = _lib.lib()
    ws = _ws.get(img.device, L.hcir_mae_mse_workspace_bytes(b * n))
    check(L.hcir_mae_mse_fwd(pred.data_ptr(), img.data_ptr(), b, c, h, w, ps, idx.data_ptr(), n, loss.data_ptr(),
                             diff.data_ptr(), ws.data_ptr(), ws.numel(), _stream(img)), "hcir_mae_mse_fwd")
    return loss, diff


# ---------------------------------------------------------------------------------------------------------------
# losses (torch.autograd Functions over the HIP kernels)
# ---------------------------------------------------------------------------------------------------------------
class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, p, n, margin, eps):
        a, p, n = (t.detach().float().contiguous() for t in (a, p, n))
        for t, nm in ((a, "anchor"), (p, "positive"), (n, "negative")):
            _dev(t, nm)
        b, d = a.shape
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        row = torch.empty(b, dtype=torch.float32, device=a.device)
        dist = torch.empty((2, b), dtype=torch.float32, device=a.device)
        check(_lib.lib().hcir_triplet_margin_fwd(a.data_ptr(), p.data_ptr(), n.data_ptr(), b, d, float(margin),
                                                 float(eps), loss.data_ptr(), row.data_ptr(), dist.data_ptr(),
                                                 _stream(a)), "hcir_triplet_margin_fwd")
        ctx.save_for_backward(a, p, n, row, dist)
        ctx.eps = float(eps)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, p, n, row, dist = ctx.saved_tensors
        b, d = a.shape
        g = g.detach().float().contiguous().reshape(1)
        da, dp, dn = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
        check(_lib.lib().hcir_triplet_margin_bwd(a.data_ptr(), p.data_ptr(), n.data_ptr(), b, d, ctx.eps,
                                                 row.data_ptr(), dist.data_ptr(), g.data_ptr(), da.data_ptr(),
                                                 dp.data_ptr(), dn.data_ptr(), _stream(a)), "hcir_triplet_margin_bwd")
        return da, dp, dn, None, None


class TripletMarginLoss(torch.nn.Module):
    """nn.TripletMarginLoss(margin, p=2, eps, swap=False, reduction='mean') on the HIP path
    (HP/src/pretrain_engine.py:96-97)."""

    def __init__(self, margin: float = 1.0, p: float = 2.0, eps: float = 1e-6, swap: bool = False,
                 reduction: str = "mean"):
        super().__init__()
        if p != 2 or swap or reduction != "mean":
            raise NotImplementedError("hcir TripletMarginLoss implements p=2, swap=False, reduction='mean'")
        self.margin, self.p, self.eps = margin, p, eps

    def forward(self, anchor, positive, negative):
        return _TripletFn.apply(anchor, positive, negative, self.margin, self.eps)


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x, y = x.detach().float().contiguous(), y.detach().float().contiguous()
        _dev(x, "input")
        _dev(y, "target")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = torch.empty(256, dtype=torch.float32, device=x.device)
        check(_lib.lib().hcir_mse_fwd(x.data_ptr(), y.data_ptr(), x.numel(), loss.data_ptr(), ws.data_ptr(),
                                      _stream(x)), "hcir_mse_fwd")
        ctx.save_for_backward(x, y)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = g.detach().float().contiguous().reshape(1)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if dx is None and dy is None:
            return None, None
        check(_lib.lib().hcir_mse_bwd(x.data_ptr(), y.data_ptr(), x.numel(), g.data_ptr(), _ptr(dx), _ptr(dy),
                                      _stream(x)), "hcir_mse_bwd")
        return dx, dy


def mse_loss(input: torch.Tensor, target: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """F.mse_loss(input, target, reduction='mean') on the HIP path (HP/src/pretrain_engine.py:730)."""
    if reduction != "mean":
        raise NotImplementedError("hcir mse_loss implements reduction='mean'")
    if input.shape != target.shape:
        raise ValueError("mse_loss: shapes differ")
    return _MseFn.apply(input, target)
