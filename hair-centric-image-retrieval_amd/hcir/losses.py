"""hcir.losses — NTXentLoss with lightly's constructor/forward signature
(lightly.loss.NTXentLoss; call sites HP/src/pretrain_engine.py:93,725), computed by
hcir_ntxent_fwd (fused normalise + 2B x 2B MFMA cosine + masked log-sum-exp) and, when the inputs
require grad, differentiated by hcir_ntxent_bwd through a torch.autograd.Function — a drop-in
`criterion(out0, out1)` for a training loop whose backbone runs on PyTorch-ROCm.

With a memory bank (memory_bank_size=(K, D), the DenseCL criteria) the loss is hcir_ntxent_bank_fwd / _bwd and the
module keeps lightly's queue.

SupConLoss with the constructor/forward signature of the reference's class (HairPretraining/utils/losses.py:8-101; call
sites HairPretraining/src/pretrain_engine.py:76,390), computed by hcir_supcon_fwd / hcir_supcon_bwd the same way.

MSNLoss with lightly's constructor/forward signature (lightly.loss.MSNLoss; the criterion of the MSN step,
HairPretraining/src/pretrain_engine.py:91,262), computed by hcir_msn_targets / hcir_msn_fwd / hcir_msn_bwd.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import HcirError, check
from .ops import _DT, _dev, _stream, _ws


def ntxent_forward(out0: torch.Tensor, out1: torch.Tensor, temperature: float, want_lse: bool = False):
    _dev(out0, "out0")
    _dev(out1, "out1")
    if out0.shape != out1.shape or out0.dim() != 2 or out0.dtype != out1.dtype:
        raise HcirError(f"NTXentLoss expects two [B, D] tensors of one dtype, got {tuple(out0.shape)} "
                        f"{out0.dtype} / {tuple(out1.shape)} {out1.dtype}")
    if out0.dtype not in _DT:
        raise HcirError(f"unsupported dtype {out0.dtype}")
    b, d = out0.shape
    L = _lib.lib()
    dt = _DT[out0.dtype]
    ws = _ws.get(out0.device, L.hcir_ntxent_workspace_bytes(b, d, dt))
    loss = torch.empty((), dtype=torch.float32, device=out0.device)
    lse = torch.empty(2 * b, dtype=torch.float32, device=out0.device) if want_lse else None
    check(L.hcir_ntxent_fwd(out0.data_ptr(), out1.data_ptr(), b, d, dt, 1.0 / temperature,
                            loss.data_ptr(), None if lse is None else lse.data_ptr(), ws.data_ptr(),
                            ws.numel(), _stream(out0)), "hcir_ntxent_fwd")
    return (loss, lse) if want_lse else loss


def ntxent_backward(out0, out1, temperature, lse, grad_out: float):
    b, d = out0.shape
    L = _lib.lib()
    dt = _DT[out0.dtype]
    ws = _ws.get(out0.device, L.hcir_ntxent_bwd_workspace_bytes(b, d, dt))
    g0, g1 = torch.empty_like(out0), torch.empty_like(out1)
    check(L.hcir_ntxent_bwd(out0.data_ptr(), out1.data_ptr(), b, d, dt, 1.0 / temperature, lse.data_ptr(),
                            float(grad_out), g0.data_ptr(), g1.data_ptr(), ws.data_ptr(), ws.numel(),
                            _stream(out0)), "hcir_ntxent_bwd")
    return g0, g1


def _supcon_labels(features: torch.Tensor, labels):
    """labels as a contiguous int64 [B] tensor on the features' device (None stays None); no value is read here."""
    if labels is None:
        return None
    if not isinstance(labels, torch.Tensor):
        labels = torch.as_tensor(labels)
    if labels.is_floating_point() or labels.is_complex():
        raise HcirError(f"SupConLoss compares labels as 64-bit integers, got {labels.dtype}")
    return labels.reshape(-1).to(device=features.device, dtype=torch.int64).contiguous()


def supcon_forward(features: torch.Tensor, labels, temperature: float, base_temperature: float,
                   normalize: bool = False, want_saved: bool = False):
    """hcir_supcon_fwd on contiguous [B, V, D] features; labels None or int64 [B] on the same device.  Returns the
    loss, or (loss, row_lse, row_npos) with want_saved."""
    _dev(features, "features")
    if features.dim() != 3 or not features.is_contiguous():
        raise HcirError(f"supcon_forward expects contiguous [B, V, D] features, got {tuple(features.shape)}")
    if features.dtype not in _DT:
        raise HcirError(f"unsupported dtype {features.dtype}")
    b, v, d = features.shape
    L = _lib.lib()
    dt = _DT[features.dtype]
    ws = _ws.get(features.device, L.hcir_supcon_workspace_bytes(b, v, d, dt, 0))
    loss = torch.empty((), dtype=torch.float32, device=features.device)
    lse = torch.empty(b * v, dtype=torch.float32, device=features.device) if want_saved else None
    npos = torch.empty(b * v, dtype=torch.int32, device=features.device) if want_saved else None
    check(L.hcir_supcon_fwd(features.data_ptr(), None if labels is None else labels.data_ptr(), b, v, d, dt,
                            1.0 / temperature, temperature / base_temperature, int(bool(normalize)),
                            loss.data_ptr(), None if lse is None else lse.data_ptr(),
                            None if npos is None else npos.data_ptr(), ws.data_ptr(), ws.numel(),
                            _stream(features)), "hcir_supcon_fwd")
    return (loss, lse, npos) if want_saved else loss


def supcon_backward(features, labels, temperature, base_temperature, normalize, lse, npos, grad_out: float):
    b, v, d = features.shape
    if (b * v) % 8:
        raise HcirError("hcir_supcon_bwd needs batch size x n_views to be a multiple of 8")
    L = _lib.lib()
    dt = _DT[features.dtype]
    ws = _ws.get(features.device, L.hcir_supcon_workspace_bytes(b, v, d, dt, 1))
    grad = torch.empty_like(features)
    check(L.hcir_supcon_bwd(features.data_ptr(), None if labels is None else labels.data_ptr(), b, v, d, dt,
                            1.0 / temperature, 1.0 / base_temperature, int(bool(normalize)), lse.data_ptr(),
                            npos.data_ptr(), float(grad_out), grad.data_ptr(), ws.data_ptr(), ws.numel(),
                            _stream(features)), "hcir_supcon_bwd")
    return grad


class _SupConFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, labels, temperature, base_temperature, normalize):
        features = features.contiguous()
        loss, lse, npos = supcon_forward(features, labels, temperature, base_temperature, normalize, want_saved=True)
        ctx.save_for_backward(features, lse, npos)
        ctx.labels = labels
        ctx.cfg = (temperature, base_temperature, normalize)
        return loss

    @staticmethod
    def backward(ctx, grad):
        features, lse, npos = ctx.saved_tensors
        g = supcon_backward(features, ctx.labels, *ctx.cfg, lse, npos, float(grad))  # one host read of dL
        return g, None, None, None, None


class SupConLoss(nn.Module):
    """SupConLoss(temperature=0.07, contrast_mode='all', base_temperature=0.07) of HairPretraining/utils/losses.py:8-101
    (the criterion of the simclr_supcon step, HairPretraining/src/pretrain_engine.py:76,390), computed by
    hcir_supcon_fwd / hcir_supcon_bwd.  `normalize=False` is the drop-in for the class; `normalize=True` fuses the
    F.normalize the reference's model applies to its output (HairPretraining/src/backbone.py:414-417), and its
    backward, into the loss, as NTXentLoss does."""

    def __init__(self, temperature: float = 0.07, contrast_mode: str = "all", base_temperature: float = 0.07,
                 normalize: bool = False):
        super().__init__()
        if contrast_mode == "one":
            raise NotImplementedError("contrast_mode='one' is never used by the reference (every SupConLoss there is "
                                      "built with the default 'all', HairPretraining/src/pretrain_engine.py:76)")
        if contrast_mode != "all":
            raise ValueError("Unknown mode: {}".format(contrast_mode))
        if abs(temperature) < 1e-8 or abs(base_temperature) < 1e-8:
            raise ValueError(f"Illegal temperature: abs({temperature}) or abs({base_temperature}) < 1e-8")
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature
        self.normalize = bool(normalize)

    def forward(self, features: torch.Tensor, labels=None, mask=None) -> torch.Tensor:
        if len(features.shape) < 3:
            raise ValueError("`features` needs to be [bsz, n_views, ...], at least 3 dimensions are required")
        if labels is not None and mask is not None:
            raise ValueError("Cannot define both `labels` and `mask`")
        if mask is not None:
            raise NotImplementedError("an explicit `mask` is never passed by the reference (its one call site, "
                                      "HairPretraining/src/pretrain_engine.py:390, passes labels); use labels")
        if len(features.shape) > 3:
            features = features.reshape(features.shape[0], features.shape[1], -1)
        if labels is not None:
            labels = _supcon_labels(features, labels)
            if labels.shape[0] != features.shape[0]:
                raise ValueError("Num of labels does not match num of features")
        if not features.is_cuda:
            raise HcirError(f"SupConLoss got `features` on {features.device}; the loss runs on a HIP device only "
                            "(no CPU fallback)")
        if torch.is_grad_enabled() and features.requires_grad:
            if (features.shape[0] * features.shape[1]) % 8:
                raise HcirError("hcir_supcon_bwd needs batch size x n_views to be a multiple of 8")
            return _SupConFn.apply(features, labels, self.temperature, self.base_temperature, self.normalize)
        return supcon_forward(features.contiguous(), labels, self.temperature, self.base_temperature, self.normalize)


class _NTXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out0, out1, temperature):
        out0, out1 = out0.contiguous(), out1.contiguous()
        loss, lse = ntxent_forward(out0, out1, temperature, want_lse=True)
        ctx.save_for_backward(out0, out1, lse)
        ctx.temperature = temperature
        return loss

    @staticmethod
    def backward(ctx, grad):
        out0, out1, lse = ctx.saved_tensors
        g0, g1 = ntxent_backward(out0, out1, ctx.temperature, lse, float(grad))  # one host read of dL
        return g0, g1, None


def ntxent_bank_forward(out0: torch.Tensor, out1: torch.Tensor, bank: torch.Tensor, temperature: float,
                        want_saved: bool = False):
    """hcir_ntxent_bank_fwd on contiguous [N, D] rows of one dtype and an fp32 [K, D] bank.  Returns (loss, k_unit), or
    (loss, k_unit, row_lse, row_pos) with want_saved; k_unit fp32 [N, D] are the normalised rows of out1."""
    _dev(out0, "out0")
    _dev(out1, "out1")
    _dev(bank, "bank")
    if out0.shape != out1.shape or out0.dim() != 2 or out0.dtype != out1.dtype:
        raise HcirError(f"NTXentLoss expects two [N, D] tensors of one dtype, got {tuple(out0.shape)} "
                        f"{out0.dtype} / {tuple(out1.shape)} {out1.dtype}")
    if out0.dtype not in _DT:
        raise HcirError(f"unsupported dtype {out0.dtype}")
    n, d = out0.shape
    if bank.dim() != 2 or bank.shape[1] != d or bank.dtype != torch.float32 or not bank.is_contiguous():
        raise HcirError(f"NTXentLoss memory bank must be a contiguous fp32 [K, {d}] tensor, got {tuple(bank.shape)} "
                        f"{bank.dtype}")
    k = bank.shape[0]
    L = _lib.lib()
    dt = _DT[out0.dtype]
    ws = _ws.get(out0.device, L.hcir_ntxent_bank_workspace_bytes(n, k, d, dt, 0))
    loss = torch.empty((), dtype=torch.float32, device=out0.device)
    k_unit = torch.empty((n, d), dtype=torch.float32, device=out0.device)
    lse = torch.empty(n, dtype=torch.float32, device=out0.device) if want_saved else None
    pos = torch.empty(n, dtype=torch.float32, device=out0.device) if want_saved else None
    check(L.hcir_ntxent_bank_fwd(out0.data_ptr(), out1.data_ptr(), bank.data_ptr(), n, k, d, dt, 1.0 / temperature,
                                 loss.data_ptr(), None if lse is None else lse.data_ptr(),
                                 None if pos is None else pos.data_ptr(), k_unit.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream(out0)), "hcir_ntxent_bank_fwd")
    return (loss, k_unit, lse, pos) if want_saved else (loss, k_unit)


def ntxent_bank_backward(out0, out1, bank, temperature, lse, pos, grad_out: float, want_dz1: bool = True):
    """hcir_ntxent_bank_bwd: (dL/dout0, dL/dout1 or None) for the loss of ntxent_bank_forward on the same bank."""
    n, d = out0.shape
    k = bank.shape[0]
    if k % 8:
        raise HcirError("hcir_ntxent_bank_bwd needs a bank size that is a multiple of 8")
    L = _lib.lib()
    dt = _DT[out0.dtype]
    ws = _ws.get(out0.device, L.hcir_ntxent_bank_workspace_bytes(n, k, d, dt, 1))
    g0 = torch.empty_like(out0)
    g1 = torch.empty_like(out1) if want_dz1 else None
    check(L.hcir_ntxent_bank_bwd(out0.data_ptr(), out1.data_ptr(), bank.data_ptr(), n, k, d, dt, 1.0 / temperature,
                                 lse.data_ptr(), pos.data_ptr(), float(grad_out), g0.data_ptr(),
                                 None if g1 is None else g1.data_ptr(), ws.data_ptr(), ws.numel(), _stream(out0)),
          "hcir_ntxent_bank_bwd")
    return g0, g1


class _NTXentBankFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out0, out1, bank, temperature):
        out0, out1 = out0.contiguous(), out1.contiguous()
        loss, k_unit, lse, pos = ntxent_bank_forward(out0, out1, bank, temperature, want_saved=True)
        # the caller enqueues into `bank` right after this call: the backward needs the rows the loss was taken against
        ctx.save_for_backward(out0, out1, bank.clone(), lse, pos)
        ctx.temperature = temperature
        ctx.mark_non_differentiable(k_unit)
        return loss, k_unit

    @staticmethod
    def backward(ctx, grad, _grad_k_unit):
        out0, out1, bank, lse, pos = ctx.saved_tensors
        g0, g1 = ntxent_bank_backward(out0, out1, bank, ctx.temperature, lse, pos, float(grad),  # one host read of dL
                                      want_dz1=ctx.needs_input_grad[1])
        return g0, g1, None, None


def bank_criterion(out0: torch.Tensor, out1: torch.Tensor, bank: torch.Tensor, temperature: float):
    """(loss, k_unit) of NT-Xent against `bank`, differentiable in out0 / out1 where they require a gradient.  HIP
    device only: there is no CPU path."""
    if not out0.is_cuda:
        raise HcirError(f"NTXentLoss got `out0` on {out0.device}; the loss runs on a HIP device only (no CPU fallback)")
    if torch.is_grad_enabled() and (out0.requires_grad or out1.requires_grad):
        if bank.shape[0] % 8:
            raise HcirError("hcir_ntxent_bank_bwd needs a bank size that is a multiple of 8")
        return _NTXentBankFn.apply(out0, out1, bank, temperature)
    return ntxent_bank_forward(out0.contiguous(), out1.contiguous(), bank, temperature)


class NTXentLoss(nn.Module):
    """NTXentLoss(temperature=0.5, memory_bank_size=0, gather_distributed=False).

    memory_bank_size (K, D), or an int K with the width taken from the first call, adds lightly's memory bank (the two
    criteria of the DenseCL step, HairPretraining/src/pretrain_engine.py:85-87): a non-persistent fp32 buffer `bank`
    [K, D] of unit rows, initialised as F.normalize(torch.randn(K, D), dim=-1).  forward(out0, out1) is the
    cross-entropy of [q_i.k_i, q_i.bank_0 ..] / T against the bank AS IT WAS BEFORE THE CALL (hcir_ntxent_bank_fwd /
    _bwd); then, where out0 requires a gradient (lightly's `update`), the normalised rows of out1 are enqueued at
    `bank_ptr`: if ptr + n >= K, bank[ptr:] = k[:K - ptr] and ptr = 0 (the rows that do not fit are dropped), else
    bank[ptr:ptr + n] = k and ptr += n.  `bank_ptr` is a Python int: nothing is read back from the device."""

    def __init__(self, temperature: float = 0.5, memory_bank_size=0, gather_distributed: bool = False):
        super().__init__()
        if abs(temperature) < 1e-8:
            raise ValueError("Illegal temperature: abs({}) < 1e-8".format(temperature))
        if gather_distributed:
            raise NotImplementedError("gather_distributed is never enabled by the reference "
                                      "(SURVEY.md §2.3)")
        self.temperature = temperature
        self.bank_size = 0
        self.bank_ptr = 0
        self.register_buffer("bank", None, persistent=False)
        if memory_bank_size not in (0, (0, 0)):
            if isinstance(memory_bank_size, bool) or not isinstance(memory_bank_size, (int, tuple, list)):
                raise ValueError(f"memory_bank_size must be an int K or a (K, D) pair, got {memory_bank_size!r}")
            if isinstance(memory_bank_size, int):
                size, dim = memory_bank_size, None
            else:
                if len(memory_bank_size) != 2 or not all(isinstance(v, int) and not isinstance(v, bool)
                                                         for v in memory_bank_size):
                    raise ValueError(f"memory_bank_size must be an int K or a (K, D) pair, got {memory_bank_size!r}")
                size, dim = memory_bank_size
            if size < 0 or (dim is not None and dim <= 0):
                raise ValueError(f"Illegal memory bank size {memory_bank_size!r}")
            self.bank_size = size
            if dim is not None:
                self._init_bank(dim, None)

    def _init_bank(self, dim: int, device) -> None:
        bank = torch.nn.functional.normalize(torch.randn(self.bank_size, dim), dim=-1)
        self.bank = bank if device is None else bank.to(device)
        self.bank_ptr = 0

    def _enqueue(self, k_unit: torch.Tensor) -> None:
        """lightly MemoryBankModule._dequeue_and_enqueue on rows (the bank is [K, D] here, [D, K] there)."""
        n, size, ptr = k_unit.shape[0], self.bank_size, self.bank_ptr
        with torch.no_grad():
            if ptr + n >= size:
                self.bank[ptr:] = k_unit[:size - ptr].detach()
                self.bank_ptr = 0
            else:
                self.bank[ptr:ptr + n] = k_unit.detach()
                self.bank_ptr = ptr + n

    def forward(self, out0: torch.Tensor, out1: torch.Tensor) -> torch.Tensor:
        if self.bank_size:
            if self.bank is None:
                self._init_bank(out0.shape[-1], out0.device)
            elif self.bank.device != out0.device:
                self.bank = self.bank.to(out0.device)
            loss, k_unit = bank_criterion(out0, out1, self.bank, self.temperature)
            if out0.requires_grad:
                self._enqueue(k_unit)
            return loss
        if torch.is_grad_enabled() and (out0.requires_grad or out1.requires_grad):
            if out0.shape[0] % 4:
                raise HcirError("hcir_ntxent_bwd needs a batch size that is a multiple of 4")
            return _NTXentFn.apply(out0, out1, self.temperature)
        return ntxent_forward(out0.contiguous(), out1.contiguous(), self.temperature)


def _msn_check(anchors: torch.Tensor, targets: torch.Tensor, prototypes: torch.Tensor) -> None:
    for t, name in ((anchors, "anchors"), (targets, "targets"), (prototypes, "prototypes")):
        _dev(t, name)
    if anchors.dim() != 2 or targets.dim() != 2 or prototypes.dim() != 2 or anchors.dtype != targets.dtype \
            or not (anchors.shape[1] == targets.shape[1] == prototypes.shape[1]):
        raise HcirError(f"MSNLoss expects anchors [N, D] and targets [B, D] of one dtype and prototypes [K, D], got "
                        f"{tuple(anchors.shape)} {anchors.dtype} / {tuple(targets.shape)} {targets.dtype} / "
                        f"{tuple(prototypes.shape)}")
    if anchors.dtype not in _DT:
        raise HcirError(f"unsupported dtype {anchors.dtype}")
    if prototypes.dtype != torch.float32 or not prototypes.is_contiguous():
        raise HcirError(f"MSNLoss prototypes must be a contiguous fp32 [K, D] tensor, got {prototypes.dtype}")


def msn_targets(targets: torch.Tensor, prototypes: torch.Tensor, temperature: float, sinkhorn_iterations: int = 3
                ) -> torch.Tensor:
    """hcir_msn_targets: fp32 [B, K] target probabilities, softmax_k(t_j.c_k / temperature) followed by
    `sinkhorn_iterations` Sinkhorn rounds.  `temperature` is the product T * Ts of the sharpened softmax."""
    b, d = targets.shape
    k = prototypes.shape[0]
    L = _lib.lib()
    dt = _DT[targets.dtype]
    ws = _ws.get(targets.device, L.hcir_msn_workspace_bytes(b, k, d, dt, 0))
    q = torch.empty((b, k), dtype=torch.float32, device=targets.device)
    check(L.hcir_msn_targets(targets.data_ptr(), prototypes.data_ptr(), b, k, d, dt, 1.0 / temperature,
                             int(sinkhorn_iterations), q.data_ptr(), ws.data_ptr(), ws.numel(), _stream(targets)),
          "hcir_msn_targets")
    return q


def msn_forward(anchors: torch.Tensor, prototypes: torch.Tensor, q: torch.Tensor, temperature: float,
                regularization_weight: float, want_saved: bool = False):
    """hcir_msn_fwd on contiguous anchors [N, D], fp32 prototypes [K, D] and the targets' q [B, K].  Returns the loss,
    or (loss, parts, row_lse, pbar) with want_saved; parts = (cross-entropy, regulariser without its weight)."""
    n, d = anchors.shape
    b, k = q.shape
    L = _lib.lib()
    dt = _DT[anchors.dtype]
    ws = _ws.get(anchors.device, L.hcir_msn_workspace_bytes(n, k, d, dt, 1))
    dev = anchors.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty(2, dtype=torch.float32, device=dev) if want_saved else None
    lse = torch.empty(n, dtype=torch.float32, device=dev) if want_saved else None
    pbar = torch.empty(k, dtype=torch.float32, device=dev) if want_saved else None
    check(L.hcir_msn_fwd(anchors.data_ptr(), prototypes.data_ptr(), q.data_ptr(), n, b, k, d, dt, 1.0 / temperature,
                         float(regularization_weight), loss.data_ptr(), None if parts is None else parts.data_ptr(),
                         None if lse is None else lse.data_ptr(), None if pbar is None else pbar.data_ptr(),
                         ws.data_ptr(), ws.numel(), _stream(anchors)), "hcir_msn_fwd")
    return (loss, parts, lse, pbar) if want_saved else loss


def msn_backward(anchors, prototypes, q, temperature, regularization_weight, lse, pbar, grad_out: float):
    """hcir_msn_bwd: dL/danchors for the loss of msn_forward on the same prototypes and q."""
    n, d = anchors.shape
    b, k = q.shape
    if k % 8:
        raise HcirError("hcir_msn_bwd needs a number of prototypes that is a multiple of 8")
    L = _lib.lib()
    dt = _DT[anchors.dtype]
    ws = _ws.get(anchors.device, L.hcir_msn_workspace_bytes(n, k, d, dt, 2))
    grad = torch.empty_like(anchors)
    check(L.hcir_msn_bwd(anchors.data_ptr(), prototypes.data_ptr(), q.data_ptr(), n, b, k, d, dt, 1.0 / temperature,
                         float(regularization_weight), lse.data_ptr(), pbar.data_ptr(), float(grad_out),
                         grad.data_ptr(), ws.data_ptr(), ws.numel(), _stream(anchors)), "hcir_msn_bwd")
    return grad


class _MSNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchors, targets, prototypes, temperature, sharpen, iterations, weight):
        anchors, targets = anchors.contiguous(), targets.contiguous()
        q = msn_targets(targets, prototypes, temperature * sharpen, iterations)
        loss, _parts, lse, pbar = msn_forward(anchors, prototypes, q, temperature, weight, want_saved=True)
        # the caller may step the prototypes' owner before the backward: keep the rows the loss was taken against
        ctx.save_for_backward(anchors, prototypes.clone(), q, lse, pbar)
        ctx.cfg = (temperature, weight)
        return loss

    @staticmethod
    def backward(ctx, grad):
        anchors, prototypes, q, lse, pbar = ctx.saved_tensors
        g = msn_backward(anchors, prototypes, q, *ctx.cfg, lse, pbar, float(grad))  # one host read of dL
        return g, None, None, None, None, None, None


class MSNLoss(nn.Module):
    """MSNLoss(temperature=0.1, sinkhorn_iterations=3, regularization_weight=1.0, gather_distributed=False) of lightly
    (the criterion of the MSN step, HairPretraining/src/pretrain_engine.py:91,262).
    forward(anchors [N, D], targets [B, D], prototypes [K, D], target_sharpen_temperature=0.25): the cross-entropy of
    the anchors' prototype softmax against the targets' sharpened, Sinkhorn-normalised one (row i of the anchors pairs
    with target i mod B) plus `regularization_weight` times the mean-entropy regulariser.  The gradient reaches the
    anchors only: the reference hands over `model.prototypes.data`."""

    def __init__(self, temperature: float = 0.1, sinkhorn_iterations: int = 3, regularization_weight: float = 1.0,
                 gather_distributed: bool = False):
        super().__init__()
        if temperature <= 0:
            raise ValueError(f"temperature must be in (0, inf) but is {temperature}.")
        if sinkhorn_iterations < 0:
            raise ValueError(f"sinkhorn_iterations must be >= 0 but is {sinkhorn_iterations}.")
        if gather_distributed:
            raise NotImplementedError("gather_distributed is never enabled by the reference "
                                      "(SURVEY.md §2.3)")
        self.temperature = temperature
        self.sinkhorn_iterations = sinkhorn_iterations
        self.regularization_weight = regularization_weight
        self.gather_distributed = False

    def forward(self, anchors: torch.Tensor, targets: torch.Tensor, prototypes: torch.Tensor,
                target_sharpen_temperature: float = 0.25) -> torch.Tensor:
        if prototypes.requires_grad:
            raise NotImplementedError("a gradient to the prototypes is never used by the reference (its one call site, "
                                      "HairPretraining/src/pretrain_engine.py:262, passes model.prototypes.data); pass "
                                      "prototypes.data or a detached tensor")
        if targets.shape[0] == 0 or anchors.shape[0] % targets.shape[0]:
            raise ValueError(f"the number of anchors ({anchors.shape[0]}) must be a multiple of the number of targets "
                             f"({targets.shape[0]})")
        if not anchors.is_cuda:
            raise HcirError(f"MSNLoss got `anchors` on {anchors.device}; the loss runs on a HIP device only "
                            "(no CPU fallback)")
        targets = targets.detach()
        if targets.dtype != anchors.dtype:
            targets = targets.to(anchors.dtype)
        prototypes = prototypes.detach()
        if prototypes.dtype != torch.float32 or not prototypes.is_contiguous():
            prototypes = prototypes.float().contiguous()
        _msn_check(anchors, targets, prototypes)
        if torch.is_grad_enabled() and anchors.requires_grad:
            if prototypes.shape[0] % 8:
                raise HcirError("hcir_msn_bwd needs a number of prototypes that is a multiple of 8")
            return _MSNFn.apply(anchors, targets, prototypes, self.temperature, target_sharpen_temperature,
                                self.sinkhorn_iterations, self.regularization_weight)
        q = msn_targets(targets.contiguous(), prototypes, self.temperature * target_sharpen_temperature,
                        self.sinkhorn_iterations)
        return msn_forward(anchors.contiguous(), prototypes, q, self.temperature, self.regularization_weight)
