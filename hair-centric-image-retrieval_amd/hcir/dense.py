"""hcir.dense — DenseCL's dense correspondence on the HIP path.

    select_most_similar(x, y, y_values)      lightly.models.utils.select_most_similar as the DenseCL step calls it
                                             (HairPretraining/src/pretrain_engine.py:300): for every query position the
                                             value row of the most similar key position of the same image
    dense_match(x, y, y_values=None)         the kernel call itself (hcir_dense_match_f16): indices and gathered rows

x [B, N, C] and y [B, M, C] are a trunk's last maps read as position rows - the fp16 NHWC map of
hcir.conv_train.train_trunk_map as it stands, without a permute.  HIP device only: there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import HcirError, check
from .ops import _DT, _stream, _ws

MAX_POSITIONS = 256    # hcir_dense_match_f16: N, M <= 256


def _check(x, y, y_values) -> None:
    for name, t in (("x", x), ("y", y)) + ((("y_values", y_values),) if y_values is not None else ()):
        if not torch.is_tensor(t) or t.dim() != 3:
            raise HcirError(f"select_most_similar expects `{name}` as a [B, positions, channels] tensor")
        if not t.is_cuda:
            raise HcirError(f"select_most_similar got `{name}` on {t.device}; the match runs on a HIP device only "
                            "(no CPU fallback)")
    if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
        raise HcirError(f"select_most_similar: x {tuple(x.shape)} and y {tuple(y.shape)} must agree in batch and channels")
    if x.shape[1] < 1 or y.shape[1] < 1 or x.shape[0] < 1:
        raise HcirError("select_most_similar needs at least one image, one query and one key position")
    if x.shape[1] > MAX_POSITIONS or y.shape[1] > MAX_POSITIONS:
        raise HcirError(f"select_most_similar serves at most {MAX_POSITIONS} positions per image, got "
                        f"{x.shape[1]} / {y.shape[1]}")
    if x.shape[2] % 8:
        raise HcirError(f"select_most_similar needs a channel count that is a multiple of 8, got {x.shape[2]}")
    for name, t in (("x", x), ("y", y)):
        if t.dtype not in (torch.float16, torch.float32):
            raise HcirError(f"select_most_similar takes fp16 or fp32 `{name}`, got {t.dtype}")
    if y_values is not None:
        if y_values.shape[:2] != y.shape[:2]:
            raise HcirError(f"select_most_similar: y_values {tuple(y_values.shape)} must have y's [B, M] "
                            f"{tuple(y.shape[:2])}")
        if y_values.shape[2] % 8:
            raise HcirError(f"select_most_similar needs a value width that is a multiple of 8, got {y_values.shape[2]}")
        if y_values.dtype not in (torch.float16, torch.float32):
            raise HcirError(f"select_most_similar takes fp16 or fp32 `y_values`, got {y_values.dtype}")


def dense_match(x: torch.Tensor, y: torch.Tensor, y_values: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(idx int32 [B, N], out [B, N, Dv] or None): idx[b, n] = argmax_m x_bn . y_bm / max(||y_bm||, 1e-12), the lowest
    m on an exact tie of the fp32 scores; out[b, n] = y_values[b, idx[b, n]], bit for bit.  fp32 x / y are rounded to
    fp16 once.  Nothing here is differentiable."""
    _check(x, y, y_values)
    x16, y16 = x.detach().half().contiguous(), y.detach().half().contiguous()
    b, n, c = x16.shape
    m = y16.shape[1]
    L = _lib.lib()
    idx = torch.empty((b, n), dtype=torch.int32, device=x.device)
    vals = out = None
    dv = 0
    if y_values is not None:
        vals = y_values.detach().contiguous()
        dv = vals.shape[2]
        out = torch.empty((b, n, dv), dtype=vals.dtype, device=x.device)
    ws = _ws.get(x.device, L.hcir_dense_match_workspace_bytes(b, m))
    check(L.hcir_dense_match_f16(x16.data_ptr(), y16.data_ptr(), None if vals is None else vals.data_ptr(),
                                 _DT[vals.dtype] if vals is not None else _DT[torch.float16], b, n, m, c, dv,
                                 idx.data_ptr(), None if out is None else out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream(x16)), "hcir_dense_match_f16")
    return idx, out


def select_most_similar(x: torch.Tensor, y: torch.Tensor, y_values: torch.Tensor) -> torch.Tensor:
    """lightly.models.utils.select_most_similar: for every image b and query position n the row of y_values [B, M, Dv]
    at the key position whose y [B, M, C] row has the largest cosine with x [B, N, C]'s -> [B, N, Dv] in y_values'
    dtype.  The match itself (hcir_dense_match_f16) carries no gradient, as an arg-max does not; fp32 x and y are
    rounded to fp16 ONCE before it, so a near-tie may resolve differently from an fp32 torch run.  Where y_values
    requires a gradient the kernel's indices are gathered with torch, which keeps the gather differentiable;
    otherwise the kernel gathers."""
    if y_values is None:
        raise HcirError("select_most_similar needs y_values (dense_match returns the indices alone)")
    if torch.is_grad_enabled() and y_values.requires_grad:
        _check(x, y, y_values)
        idx, _ = dense_match(x, y, None)
        index = idx.long().unsqueeze(-1).expand(-1, -1, y_values.shape[2])
        return torch.gather(y_values, 1, index)
    return dense_match(x, y, y_values)[1]
