"""hcir.ops — thin torch-tensor wrappers over the C ABI (include/hcir.h).

Every wrapper takes HIP-device tensors, passes raw device pointers and the current
stream, and raises if the tensor lives anywhere else: no CPU fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import BF16, F16, F32, HcirError, check

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}


def _dev(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise HcirError(f"hcir op got `{name}` on {t.device}; the hot path runs on a HIP device "
                        "only (no CPU fallback)")
    if not t.is_contiguous():
        raise HcirError(f"`{name}` must be contiguous")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def row_invnorm(x: torch.Tensor, eps: float) -> torch.Tensor:
    """1 / max(||x_i||, eps) per row (fp32)."""
    _dev(x, "x")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.lib().hcir_row_invnorm(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0),
                                      _DT[x.dtype], eps, out.data_ptr(), _stream(x)), "hcir_row_invnorm")
    return out


def l2_normalize(x: torch.Tensor, eps: float = 1e-12, want_f16: bool = False):
    """F.normalize(x, dim=1) for fp32 rows; optionally also an fp16 copy."""
    _dev(x, "x")
    if x.dtype != torch.float32:
        raise HcirError("l2_normalize expects fp32")
    y = torch.empty_like(x)
    y16 = torch.empty(x.shape, dtype=torch.float16, device=x.device) if want_f16 else None
    check(_lib.lib().hcir_l2_normalize(x.data_ptr(), x.shape[0], x.shape[1], eps, y.data_ptr(),
                                       _ptr(y16), _stream(x)), "hcir_l2_normalize")
    return (y, y16) if want_f16 else y


def convert(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 -> fp16/bf16 copy (gallery upload)."""
    _dev(x, "x")
    if x.dtype != torch.float32:
        raise HcirError("convert expects fp32 input")
    if dtype == torch.float32:
        return x
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(_lib.lib().hcir_convert_f32(x.data_ptr(), x.numel(), _DT[dtype], y.data_ptr(), _stream(x)),
          "hcir_convert_f32")
    return y


class _WorkspaceCache:
    """Scratch buffers for the C ABI (which allocates nothing itself), one per (device, stream): two streams
    never share a buffer, so concurrent calls cannot race on it.  A buffer grows on demand and is dropped only after
    SHRINK_AFTER consecutive requests that would fit an eighth of it (a one-off k = 642 sweep does not pin its
    gigabytes for the process lifetime, while a training backward that alternates 66 MB weight-gradient workspaces
    with KB-sized reductions keeps ONE buffer instead of re-allocating it several hundred times per step)."""

    SHRINK_AFTER = 64

    def __init__(self):
        self._buf = {}
        self._small = {}

    def get(self, device: torch.device, nbytes: int) -> torch.Tensor:
        key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
        b = self._buf.get(key)
        if b is not None and b.numel() >= nbytes:
            if b.numel() > max(8 * nbytes, 64 << 20):
                self._small[key] = self._small.get(key, 0) + 1
                if self._small[key] < self.SHRINK_AFTER:
                    return b
            else:
                self._small[key] = 0
                return b
        b = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        self._buf[key] = b
        self._small[key] = 0
        return b


_ws = _WorkspaceCache()
WORKSPACE_LIMIT_BYTES = 1 << 30   # sim_topk splits its queries into chunks whose workspace stays below this


def sim_topk(q: torch.Tensor, g: torch.Tensor, k: int, q_inv_norm: Optional[torch.Tensor] = None,
             g_inv_norm: Optional[torch.Tensor] = None, idx_base: int = 0
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k of (<q_i, g_j> * g_inv_norm[j]) * q_inv_norm[i]; (values fp32, indices int64).

    Ties: score descending, then index ascending.  Raises ValueError when k > len(g),
    as sklearn's kneighbors does (HP/src/classification_engine.py:71 sweeps k up to 642).
    """
    _dev(q, "q")
    _dev(g, "g")
    if q.dtype != g.dtype or q.dtype not in _DT:
        raise HcirError(f"q/g dtypes must match and be fp32/fp16/bf16, got {q.dtype}/{g.dtype}")
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise HcirError(f"shape mismatch: q {tuple(q.shape)} g {tuple(g.shape)}")
    nq, d = q.shape
    ng = g.shape[0]
    if k > ng:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, "
                         f"n_samples_fit = {ng}, n_samples = {nq}")
    if k < 1:
        raise ValueError(f"Expected n_neighbors > 0. Got {k}")
    for t, n in ((q_inv_norm, "q_inv_norm"), (g_inv_norm, "g_inv_norm")):
        if t is not None:
            _dev(t, n)
            if t.dtype != torch.float32:
                raise HcirError(f"{n} must be fp32")
    L = _lib.lib()
    val = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    # bounded workspace: the partial lists are 2 * 512 * nq * {16,32,64} * 4 B (270 KB per query at k > 32), so a
    # large query set is scanned in chunks (queries are independent; each chunk re-streams the gallery)
    chunk = nq
    while chunk > 128 and L.hcir_sim_topk_workspace_bytes(chunk, ng, d, k, _DT[q.dtype]) > WORKSPACE_LIMIT_BYTES:
        chunk = (chunk + 1) // 2
    if chunk < nq:
        chunk = (chunk + 127) // 128 * 128
    for s0 in range(0, nq, chunk):
        n = min(chunk, nq - s0)
        wsb = L.hcir_sim_topk_workspace_bytes(n, ng, d, k, _DT[q.dtype])
        ws = _ws.get(q.device, wsb)
        qn = None if q_inv_norm is None else q_inv_norm[s0:s0 + n]
        check(L.hcir_sim_topk(q[s0:s0 + n].data_ptr(), n, g.data_ptr(), ng, d, k, _DT[q.dtype], _ptr(qn),
                              _ptr(g_inv_norm), idx_base, val[s0:s0 + n].data_ptr(), idx[s0:s0 + n].data_ptr(),
                              ws.data_ptr(), ws.numel(), _stream(q)), "hcir_sim_topk")
    return val, idx


def topk_merge(vals: torch.Tensor, idx: torch.Tensor, k_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge [nlists, nq, k_in] sorted lists into [nq, k_out]."""
    _dev(vals, "vals")
    _dev(idx, "idx")
    if vals.dtype != torch.float32 or idx.dtype != torch.int64 or vals.shape != idx.shape:
        raise HcirError("topk_merge expects fp32 values and int64 indices of equal shape")
    nl, nq, kin = vals.shape
    ov = torch.empty((nq, k_out), dtype=torch.float32, device=vals.device)
    oi = torch.empty((nq, k_out), dtype=torch.int64, device=vals.device)
    check(_lib.lib().hcir_topk_merge(vals.data_ptr(), idx.data_ptr(), nl, nq, kin, k_out,
                                     ov.data_ptr(), oi.data_ptr(), _stream(vals)), "hcir_topk_merge")
    return ov, oi


# ------------------------------------------------------------------ ResNet trunk (csrc/conv.hip)
def conv_out_size(n: int, r: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - r) // stride + 1


def stem_out_size(n: int) -> int:
    """Side of the pooled stem map: conv 7 / 2 / pad 3, then maxpool 3 / 2 / pad 1."""
    return ((n - 1) // 2 + 1 - 1) // 2 + 1


def conv2d_f16(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, stride: int, pad: int,
               resid: Optional[torch.Tensor] = None, relu: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu?(conv(x, w) * scale + bias (+ resid)): x fp16 [B,H,W,Cin], w fp16 [Cout,R,S,Cin], scale / bias fp32 [Cout],
    resid fp16 of the output's shape -> fp16 [B,Ho,Wo,Cout] (written into `out` when given)."""
    for t, n in ((x, "x"), (w, "w"), (scale, "scale"), (bias, "bias")):
        _dev(t, n)
    if x.dtype != torch.float16 or w.dtype != torch.float16 or x.dim() != 4 or w.dim() != 4:
        raise HcirError("conv2d_f16 expects fp16 NHWC activations and fp16 [Cout,R,S,Cin] weights")
    if scale.dtype != torch.float32 or bias.dtype != torch.float32:
        raise HcirError("conv2d_f16 expects fp32 scale and bias")
    b, h, wd, cin = x.shape
    cout, r, s, cin_w = w.shape
    if cin_w != cin or scale.numel() != cout or bias.numel() != cout:
        raise HcirError(f"shape mismatch: x {tuple(x.shape)} w {tuple(w.shape)} scale {tuple(scale.shape)}")
    shape = (b, conv_out_size(h, r, stride, pad), conv_out_size(wd, s, stride, pad), cout)
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=x.device)
    for t, n in ((out, "out"), (resid, "resid")):
        if t is not None:
            _dev(t, n)
            if t.dtype != torch.float16 or tuple(t.shape) != shape:
                raise HcirError(f"`{n}` must be fp16 {shape}, got {t.dtype} {tuple(t.shape)}")
    check(_lib.lib().hcir_conv2d_f16(x.data_ptr(), b, h, wd, cin, w.data_ptr(), cout, r, s, stride, pad,
                                     scale.data_ptr(), bias.data_ptr(), _ptr(resid), int(relu), out.data_ptr(),
                                     _stream(x)), "hcir_conv2d_f16")
    return out


def resnet_stem(img: torch.Tensor, w_packed: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """maxpool(relu(bn(conv7x7/2(img)))): img fp32 NCHW [B,3,H,W], w_packed from resnet_engine.pack_stem_weight ->
    fp16 NHWC [B,Hp,Wp,64]."""
    for t, n in ((img, "img"), (w_packed, "w_packed"), (scale, "scale"), (bias, "bias")):
        _dev(t, n)
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3:
        raise HcirError(f"resnet_stem expects an fp32 [B,3,H,W] image, got {img.dtype} {tuple(img.shape)}")
    if w_packed.dtype != torch.float16 or w_packed.numel() != 10 * 2 * 64 * 8:
        raise HcirError("resnet_stem expects the packed fp16 stem weight (pack_stem_weight)")
    if scale.dtype != torch.float32 or bias.dtype != torch.float32 or scale.numel() != 64 or bias.numel() != 64:
        raise HcirError("resnet_stem expects fp32 scale and bias of 64 channels")
    b, _, h, wd = img.shape
    shape = (b, stem_out_size(h), stem_out_size(wd), 64)
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=img.device)
    _dev(out, "out")
    if out.dtype != torch.float16 or tuple(out.shape) != shape:
        raise HcirError(f"`out` must be fp16 {shape}")
    check(_lib.lib().hcir_resnet_stem(img.data_ptr(), b, h, wd, w_packed.data_ptr(), scale.data_ptr(),
                                      bias.data_ptr(), out.data_ptr(), _stream(img)), "hcir_resnet_stem")
    return out


def avgpool_nhwc(x: torch.Tensor, l2_normalize: bool = False, eps: float = 1e-12,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mean over H, W of fp16 [B,H,W,C] -> fp32 [B,C]; optionally F.normalize of each row."""
    _dev(x, "x")
    if x.dtype != torch.float16 or x.dim() != 4:
        raise HcirError("avgpool_nhwc expects fp16 [B,H,W,C]")
    b, h, wd, c = x.shape
    if out is None:
        out = torch.empty((b, c), dtype=torch.float32, device=x.device)
    _dev(out, "out")
    if out.dtype != torch.float32 or tuple(out.shape) != (b, c):
        raise HcirError(f"`out` must be fp32 {(b, c)}")
    check(_lib.lib().hcir_avgpool_nhwc_f16(x.data_ptr(), b, h, wd, c, int(l2_normalize), eps, out.data_ptr(),
                                           _stream(x)), "hcir_avgpool_nhwc_f16")
    return out


# ------------------------------------------------------------------ ResNet body backward (csrc/conv_bwd.hip)
def _wgrad_shape(x: torch.Tensor, dy: torch.Tensor, r: int, stride: int, pad: int):
    if x.dtype != torch.float16 or dy.dtype != torch.float16 or x.dim() != 4 or dy.dim() != 4:
        raise HcirError("conv2d_wgrad expects fp16 NHWC x [B,H,W,Cin] and dy [B,Ho,Wo,Cout]")
    b, h, wd, cin = x.shape
    cout = dy.shape[3]
    want = (b, conv_out_size(h, r, stride, pad), conv_out_size(wd, r, stride, pad), cout)
    if tuple(dy.shape) != want:
        raise HcirError(f"shape mismatch: x {tuple(x.shape)} with a {r}x{r} / {stride} / pad {pad} conv gives dy "
                        f"{want}, got {tuple(dy.shape)}")
    return b, h, wd, cin, cout


def conv2d_wgrad_splits(b: int, h: int, w: int, cin: int, cout: int, r: int, stride: int, pad: int) -> int:
    """Number of M splits hcir_conv2d_wgrad_f16 runs the shape with; raises for a shape without a kernel."""
    n = _lib.lib().hcir_conv2d_wgrad_splits(b, h, w, cin, cout, r, r, stride, pad)
    if n < 0:
        check(n, "hcir_conv2d_wgrad_splits")
    return n


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, r: int, stride: int, pad: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient of conv2d_f16's convolution: x fp16 [B,H,W,Cin], dy fp16 [B,Ho,Wo,Cout] -> fp32
    [Cout,R,S,Cin] (the layout of resnet_engine.pack_conv_weight), deterministic."""
    _dev(x, "x")
    _dev(dy, "dy")
    b, h, wd, cin, cout = _wgrad_shape(x, dy, r, stride, pad)
    shape = (cout, r, r, cin)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _dev(out, "out")
    if out.dtype != torch.float32 or tuple(out.shape) != shape:
        raise HcirError(f"`out` must be fp32 {shape}, got {out.dtype} {tuple(out.shape)}")
    L = _lib.lib()
    wsb = L.hcir_conv2d_wgrad_workspace_bytes(b, h, wd, cin, cout, r, r, stride, pad)
    ws = _ws.get(x.device, wsb) if wsb else None
    check(L.hcir_conv2d_wgrad_f16(x.data_ptr(), dy.data_ptr(), b, h, wd, cin, cout, r, r, stride, pad, out.data_ptr(),
                                  _ptr(ws), wsb, _stream(x)), "hcir_conv2d_wgrad_f16")
    return out


def spread2_nhwc(src: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, 2i, 2j] = src[b, i, j], zero elsewhere: src fp16 [B,hs,ws,C] -> fp16 [B,h,w,C], every element written."""
    _dev(src, "src")
    if src.dtype != torch.float16 or src.dim() != 4:
        raise HcirError("spread2_nhwc expects fp16 [B,hs,ws,C]")
    b, hs, ws, c = src.shape
    shape = (b, h, w, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=src.device)
    _dev(out, "out")
    if out.dtype != torch.float16 or tuple(out.shape) != shape:
        raise HcirError(f"`out` must be fp16 {shape}, got {out.dtype} {tuple(out.shape)}")
    check(_lib.lib().hcir_spread2_nhwc_f16(src.data_ptr(), b, hs, ws, c, h, w, out.data_ptr(), _stream(src)),
          "hcir_spread2_nhwc_f16")
    return out


# ------------------------------------------------------------------ ResNet body BatchNorm2d, training (csrc/bn2d.hip)
def _bn2d_map(t: torch.Tensor, name: str, like: Optional[torch.Tensor] = None) -> None:
    _dev(t, name)
    if t.dtype != torch.float16 or t.dim() != 4:
        raise HcirError(f"`{name}` must be an fp16 NHWC [B,H,W,C] tensor, got {t.dtype} {tuple(t.shape)}")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise HcirError(f"`{name}` {tuple(t.shape)} on {t.device} does not match {tuple(like.shape)} on {like.device}")


def _bn2d_vec(t: torch.Tensor, name: str, x: torch.Tensor) -> None:
    _dev(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != (x.shape[3],) or t.device != x.device:
        raise HcirError(f"`{name}` must be fp32 [{x.shape[3]}] on {x.device}, got {t.dtype} {tuple(t.shape)} on "
                        f"{t.device}")


def bn2d_chunks(m: int, c: int) -> int:
    """Number of row chunks the BatchNorm2d reductions run an [m, c] map with; raises for a shape without a kernel."""
    n = _lib.lib().hcir_bn2d_chunks(m, c)
    if n < 0:
        check(n, "hcir_bn2d_chunks")
    return n


def bn2d_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, momentum: float,
             resid: Optional[torch.Tensor] = None, relu: bool = False, running_mean: Optional[torch.Tensor] = None,
             running_var: Optional[torch.Tensor] = None):
    """Batch-statistics BatchNorm2d (+ resid) (+ ReLU) of x fp16 NHWC [B,H,W,C] -> (y fp16 like x, save_mean fp32 [C],
    save_rstd fp32 [C]); running_mean / running_var fp32 [C], where given, are updated in place with `momentum`
    (the unbiased variance for running_var), as F.batch_norm(training=True) does."""
    _bn2d_map(x, "x")
    _bn2d_vec(gamma, "gamma", x)
    _bn2d_vec(beta, "beta", x)
    if resid is not None:
        _bn2d_map(resid, "resid", x)
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _bn2d_vec(t, name, x)
    c = x.shape[3]
    m = x.numel() // c
    y = torch.empty_like(x)
    save_mean = torch.empty(c, dtype=torch.float32, device=x.device)
    save_rstd = torch.empty(c, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    wsb = L.hcir_bn2d_workspace_bytes(m, c)
    ws = _ws.get(x.device, wsb)
    check(L.hcir_bn2d_fwd_nhwc_f16(x.data_ptr(), m, c, gamma.data_ptr(), beta.data_ptr(), eps, momentum, _ptr(resid),
                                   int(bool(relu)), _ptr(running_mean), _ptr(running_var), save_mean.data_ptr(),
                                   save_rstd.data_ptr(), y.data_ptr(), ws.data_ptr(), wsb, _stream(x)),
          "hcir_bn2d_fwd_nhwc_f16")
    return y, save_mean, save_rstd


def bn2d_bwd(dy: torch.Tensor, x: torch.Tensor, y_relu: Optional[torch.Tensor], gamma: torch.Tensor,
             save_mean: torch.Tensor, save_rstd: torch.Tensor, want_dresid: bool = False):
    """Backward of bn2d_fwd: -> (dx fp16 like x, dresid fp16 like x or None, dgamma fp32 [C], dbeta fp32 [C]).
    y_relu: the forward's output when it applied ReLU (its sign is the mask), else None."""
    _bn2d_map(x, "x")
    _bn2d_map(dy, "dy", x)
    if y_relu is not None:
        _bn2d_map(y_relu, "y_relu", x)
    _bn2d_vec(gamma, "gamma", x)
    _bn2d_vec(save_mean, "save_mean", x)
    _bn2d_vec(save_rstd, "save_rstd", x)
    c = x.shape[3]
    m = x.numel() // c
    dx = torch.empty_like(x)
    dresid = torch.empty_like(x) if want_dresid else None
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    wsb = L.hcir_bn2d_workspace_bytes(m, c)
    ws = _ws.get(x.device, wsb)
    check(L.hcir_bn2d_bwd_nhwc_f16(dy.data_ptr(), x.data_ptr(), _ptr(y_relu), m, c, gamma.data_ptr(),
                                   save_mean.data_ptr(), save_rstd.data_ptr(), dx.data_ptr(), _ptr(dresid),
                                   dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), wsb, _stream(x)),
          "hcir_bn2d_bwd_nhwc_f16")
    return dx, dresid, dgamma, dbeta


def bn2d_stats(x: torch.Tensor, eps: float, momentum: float, running_mean: Optional[torch.Tensor] = None,
               running_var: Optional[torch.Tensor] = None):
    """The statistics half of bn2d_fwd alone (its kernels, its bits): x fp16 NHWC [B,H,W,C] -> (save_mean, save_rstd)
    fp32 [C]; running_mean / running_var, where given, are updated in place."""
    _bn2d_map(x, "x")
    for t, name in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _bn2d_vec(t, name, x)
    c = x.shape[3]
    m = x.numel() // c
    save_mean = torch.empty(c, dtype=torch.float32, device=x.device)
    save_rstd = torch.empty(c, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    wsb = L.hcir_bn2d_workspace_bytes(m, c)
    ws = _ws.get(x.device, wsb)
    check(L.hcir_bn2d_stats_nhwc_f16(x.data_ptr(), m, c, eps, momentum, _ptr(running_mean), _ptr(running_var),
                                     save_mean.data_ptr(), save_rstd.data_ptr(), ws.data_ptr(), wsb, _stream(x)),
          "hcir_bn2d_stats_nhwc_f16")
    return save_mean, save_rstd


# ------------------------------------------------------------------ ResNet stem, training (csrc/stem_train.hip)
def stem_conv_size(n: int) -> int:
    """Side of the stem's conv map: conv 7 / 2 / pad 3."""
    return (n - 1) // 2 + 1


def _stem_img(img: torch.Tensor, what: str):
    _dev(img, "img")
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3:
        raise HcirError(f"{what} expects an fp32 [B,3,H,W] image, got {img.dtype} {tuple(img.shape)}")
    return img.shape[0], img.shape[2], img.shape[3]


def _stem_out(out: Optional[torch.Tensor], shape, dtype, like: torch.Tensor) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    _dev(out, "out")
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != like.device:
        raise HcirError(f"`out` must be {dtype} {tuple(shape)} on {like.device}, got {out.dtype} {tuple(out.shape)}")
    return out


def _stem_map(c: torch.Tensor, name: str) -> None:
    _bn2d_map(c, name)
    if c.shape[3] != 64:
        raise HcirError(f"`{name}` must be an fp16 NHWC [B,H,W,64] stem map, got {tuple(c.shape)}")


def stem_conv(img: torch.Tensor, w_packed: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16(conv7x7/2/pad3(fp16(img), w)) with no epilogue: img fp32 NCHW [B,3,H,W], w_packed from
    resnet_engine.pack_stem_weight -> the pre-norm map, fp16 NHWC [B,Hc,Wc,64]."""
    b, h, wd = _stem_img(img, "stem_conv")
    _dev(w_packed, "w_packed")
    if w_packed.dtype != torch.float16 or w_packed.numel() != 10 * 2 * 64 * 8:
        raise HcirError("stem_conv expects the packed fp16 stem weight (pack_stem_weight)")
    out = _stem_out(out, (b, stem_conv_size(h), stem_conv_size(wd), 64), torch.float16, img)
    check(_lib.lib().hcir_stem_conv_f16(img.data_ptr(), b, h, wd, w_packed.data_ptr(), out.data_ptr(), _stream(img)),
          "hcir_stem_conv_f16")
    return out


def stem_bn_relu_pool(c: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, save_mean: torch.Tensor,
                      save_rstd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """maxpool3x3/2/pad1(relu((c - mean) * rstd * gamma + beta)): c fp16 NHWC [B,Hc,Wc,64] -> fp16 [B,Hp,Wp,64]."""
    _stem_map(c, "c")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (save_mean, "save_mean"), (save_rstd, "save_rstd")):
        _bn2d_vec(t, name, c)
    b, hc, wc, _ = c.shape
    out = _stem_out(out, (b, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, 64), torch.float16, c)
    check(_lib.lib().hcir_stem_bn_relu_pool_f16(c.data_ptr(), b, hc, wc, gamma.data_ptr(), beta.data_ptr(),
                                                save_mean.data_ptr(), save_rstd.data_ptr(), out.data_ptr(),
                                                _stream(c)), "hcir_stem_bn_relu_pool_f16")
    return out


def stem_pool_relu_bwd(dp: torch.Tensor, c: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                       save_mean: torch.Tensor, save_rstd: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of stem_bn_relu_pool down to the conv map: dp fp16 [B,Hp,Wp,64], c fp16 [B,Hc,Wc,64] -> the gradient
    with respect to the normalised map, fp16 like c, every element written."""
    _stem_map(c, "c")
    _stem_map(dp, "dp")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (save_mean, "save_mean"), (save_rstd, "save_rstd")):
        _bn2d_vec(t, name, c)
    b, hc, wc, _ = c.shape
    want = (b, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, 64)
    if tuple(dp.shape) != want or dp.device != c.device:
        raise HcirError(f"shape mismatch: c {tuple(c.shape)} pools to {want}, got dp {tuple(dp.shape)}")
    out = _stem_out(out, tuple(c.shape), torch.float16, c)
    check(_lib.lib().hcir_stem_pool_relu_bwd_f16(dp.data_ptr(), c.data_ptr(), b, hc, wc, gamma.data_ptr(),
                                                 beta.data_ptr(), save_mean.data_ptr(), save_rstd.data_ptr(),
                                                 out.data_ptr(), _stream(c)), "hcir_stem_pool_relu_bwd_f16")
    return out


def stem_wgrad_parts(b: int, h: int, w: int) -> int:
    """Number of persistent parts hcir_stem_wgrad_f16 runs the shape with; raises for a shape without a kernel."""
    n = _lib.lib().hcir_stem_wgrad_parts(b, h, w)
    if n < 0:
        check(n, "hcir_stem_wgrad_parts")
    return n


def stem_wgrad(img: torch.Tensor, dc: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient of stem_conv: img fp32 [B,3,H,W], dc fp16 NHWC [B,Hc,Wc,64] -> fp32 [64,3,7,7] (torch's
    layout), deterministic."""
    b, h, wd = _stem_img(img, "stem_wgrad")
    _stem_map(dc, "dc")
    want = (b, stem_conv_size(h), stem_conv_size(wd), 64)
    if tuple(dc.shape) != want or dc.device != img.device:
        raise HcirError(f"shape mismatch: img {tuple(img.shape)} gives a conv map {want}, got dc {tuple(dc.shape)}")
    out = _stem_out(out, (64, 3, 7, 7), torch.float32, img)
    L = _lib.lib()
    wsb = L.hcir_stem_wgrad_workspace_bytes(b, h, wd)
    ws = _ws.get(img.device, wsb) if wsb else None
    check(L.hcir_stem_wgrad_f16(img.data_ptr(), dc.data_ptr(), b, h, wd, out.data_ptr(), _ptr(ws), wsb,
                                _stream(img)), "hcir_stem_wgrad_f16")
    return out
