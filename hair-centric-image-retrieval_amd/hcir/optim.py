"""hcir.optim — the optimizer tail of the training step on HIP: the reference's get_optimizer (HP/utils/utils.py:59-71,
called at HP/src/pretrain_engine.py:108), torch.optim.Adam with coupled L2 weight decay, and a GradScaler whose state
lives on the device, so that

    scaler.scale(total).backward(); scaler.unscale_(opt); clip_grad_norm_(params, 1.0); scaler.step(opt); scaler.update()
                                                                                        (HP/src/pretrain_engine.py:745-749)
becomes

    scaler.scale(total).backward(); opt.step_scaled(scaler, max_norm=1.0)

with three launches (hcir_grad_sumsq, hcir_optim_finalize, hcir_adam_step: csrc/optim.hip) over a cached device table of
chunks of every parameter, and no host read: found_inf, the clip coefficient, the step counts, the bias corrections,
the loss scale and its growth tracker are computed and consumed on the device.

The gradient buffers are NOT written: after step_scaled (and after step) every `.grad` still holds what backward() left
there - scaled by the loss scale, unclipped.  Code that reads gradients after the step must unscale them itself.

`Adam` is a torch.optim.Optimizer: param_groups, zero_grad, state_dict and load_state_dict are the base class's, the
per-parameter state uses torch's keys (`step`, `exp_avg`, `exp_avg_sq`), and a state_dict of torch.optim.Adam loads
into it and the reverse.  `lr` and `weight_decay` are read from the groups at every call, so a host-side schedule keeps
working.  fp32, contiguous parameters on a HIP device only; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import HcirError, check

_CHUNK = 16384          # elements per table row (the ABI allows up to 65 536): ResNet-18's 11.7 M parameters still
                        # make ~700 workgroups for 256 CUs
_MAX_GROUPS = 16        # hcir_optim_finalize takes the groups' lr by value


def get_optimizer(model, lr, weight_decay, beta1, beta2):
    """HP/utils/utils.py:59-71 with hcir.optim.Adam in place of torch.optim.Adam.  The name rule is the reference's,
    character for character - so the torchvision ViT's LayerNorm weights (`ln_1.weight`, `ln.weight`: neither "bn" nor
    "norm" in the name) and a ResNet's `downsample.1.weight` ARE decayed, as they are in the reference."""
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if param.requires_grad:
            if name.endswith(".bias") or "bn" in name or "norm" in name:
                no_decay.append(param)
            else:
                decay.append(param)
    param_groups = [
        {'params': decay, 'weight_decay': weight_decay},
        {'params': no_decay, 'weight_decay': 0.0}
    ]
    return Adam(param_groups, lr, betas=(beta1, beta2))


class GradScaler:
    """torch.amp.GradScaler's state (`scale` fp32, growth tracker int32) on the device, updated by
    Adam.step_scaled in the same launch that decides found_inf.  state_dict / load_state_dict use torch's keys, so the
    reference's `scaler_state_dict` checkpoints load."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        if growth_factor <= 1.0:
            raise HcirError("GradScaler: the growth factor must be > 1.0")
        if backoff_factor >= 1.0 or backoff_factor <= 0.0:
            raise HcirError("GradScaler: the backoff factor must be in (0, 1)")
        if int(growth_interval) <= 0:
            raise HcirError("GradScaler: growth_interval must be positive")
        self._init_scale = float(init_scale)
        self._init_growth_tracker = 0
        self._growth_factor = float(growth_factor)
        self._backoff_factor = float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._scale: Optional[torch.Tensor] = None
        self._growth_tracker: Optional[torch.Tensor] = None

    def _lazy_init(self, device) -> None:
        if self._scale is None:
            if torch.device(device).type != "cuda":
                raise HcirError(f"GradScaler: {device} is not a HIP device; there is no CPU path")
            self._scale = torch.full((), self._init_scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((), self._init_growth_tracker, dtype=torch.int32, device=device)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        self._lazy_init(loss.device)
        return loss * self._scale

    def get_scale(self) -> float:
        """Reads the device scale (synchronises: not for the step path)."""
        return self._init_scale if self._scale is None else float(self._scale.item())

    def _get_growth_tracker(self) -> int:
        return self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker.item())

    def state_dict(self) -> dict:
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor,
                "backoff_factor": self._backoff_factor, "growth_interval": self._growth_interval,
                "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict: dict) -> None:
        if len(state_dict) == 0:
            raise HcirError("GradScaler: the state dict is empty (saved from a disabled torch GradScaler?)")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (coupled L2 weight decay, bias correction; no amsgrad, no maximize) on the HIP kernels of
    csrc/optim.hip.  `step()` is the plain step; `step_scaled(scaler, max_norm)` is unscale + non-finite check +
    global-norm clip + conditional step + scaler update without a host read.  Neither writes the gradient buffers."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 amsgrad: bool = False, maximize: bool = False):
        if amsgrad or maximize:
            raise HcirError("hcir.optim.Adam: amsgrad and maximize are not supported")
        if isinstance(lr, torch.Tensor):
            raise HcirError("hcir.optim.Adam: lr must be a Python number")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise HcirError(f"hcir.optim.Adam: invalid lr / eps / weight_decay {lr} / {eps} / {weight_decay}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise HcirError(f"hcir.optim.Adam: invalid betas {betas}")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        if len(self.param_groups) > _MAX_GROUPS:
            raise HcirError(f"hcir.optim.Adam: at most {_MAX_GROUPS} parameter groups")
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_complex() or p.is_sparse or p.dtype != torch.float32:
                    raise HcirError(f"hcir.optim.Adam: fp32 dense real parameters only, got {p.dtype}"
                                    f"{' sparse' if p.is_sparse else ''}")
        self._cache = None          # (signature, table tensors, participants, device)
        self._steps = None          # fp32 [n_params] on the device; state[p]["step"] is a 0-d view of one element
        self._aux = None            # fp32 [2, n_params]: step_size, bc2_sqrt
        self.table_rebuilds = 0

    # ------------------------------------------------------------------ host side
    def _hyper(self):
        groups = self.param_groups
        b1, b2 = groups[0]["betas"]
        eps = groups[0]["eps"]
        for g in groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
                raise HcirError("hcir.optim.Adam: amsgrad, maximize and decoupled weight decay are not supported")
            if tuple(g["betas"]) != (b1, b2) or g["eps"] != eps:
                raise HcirError("hcir.optim.Adam: betas and eps must be the same in every parameter group")
            if isinstance(g["lr"], torch.Tensor):
                raise HcirError("hcir.optim.Adam: lr must be a Python number")
        return float(b1), float(b2), float(eps)

    def _participants(self):
        """[(flat index, group index, parameter)] of the parameters that have a gradient, in group order."""
        part, i = [], 0
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is not None:
                    g = p.grad
                    if not p.is_cuda or not g.is_cuda:
                        raise HcirError(f"hcir.optim.Adam: parameter on {p.device}; HIP device only, no CPU path")
                    if g.is_sparse or g.dtype != torch.float32 or p.dtype != torch.float32:
                        raise HcirError("hcir.optim.Adam: fp32 dense parameters and gradients only")
                    if not p.is_contiguous() or not g.is_contiguous():
                        raise HcirError("hcir.optim.Adam: parameters and gradients must be contiguous")
                    part.append((i, gi, p))
                i += 1
        return part, i

    def _ensure_state(self, part, n_params, device):
        """Per-parameter state in torch's layout; `step` gathered into one device array (a state loaded from a
        checkpoint carries its own 0-d step tensors: their values are copied into the array once)."""
        steps = self._steps
        stale = steps is None or steps.numel() != n_params or steps.device != device
        if not stale:
            base = steps.data_ptr()
            for i, _, p in part:
                st = self.state.get(p)
                if st and (not torch.is_tensor(st["step"]) or st["step"].data_ptr() != base + 4 * i):
                    stale = True
                    break
        if stale:
            steps = torch.zeros(n_params, dtype=torch.float32, device=device)
            i = 0
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st:
                        steps[i] = torch.as_tensor(st["step"], dtype=torch.float32).to(device)
                        st["step"] = steps[i]
                    i += 1
            self._steps = steps
            self._aux = torch.zeros(2, n_params, dtype=torch.float32, device=device)
            self._cache = None
        for i, _, p in part:
            st = self.state[p]
            if not st:
                st["step"] = steps[i]
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            else:
                for k in ("exp_avg", "exp_avg_sq"):
                    t = st[k]
                    if t.shape != p.shape or t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous():
                        raise HcirError(f"hcir.optim.Adam: state {k} does not match its parameter")

    def _signature(self):
        """What the cached table depends on: every p / grad / exp_avg / exp_avg_sq / step address (so also which
        parameters have a gradient, and every size, since a tensor that grows moves) and the groups' weight_decay."""
        sig, state = [], self.state
        for group in self.param_groups:
            sig.append(group["weight_decay"])
            for p in group["params"]:
                g = p.grad
                sig.append(p.data_ptr())
                if g is None:
                    sig.append(None)
                    continue
                sig.append(g.data_ptr())
                st = state.get(p)
                if st:
                    sig.append(st["exp_avg"].data_ptr())
                    sig.append(st["exp_avg_sq"].data_ptr())
                    t = st["step"]
                    sig.append(t.data_ptr() if torch.is_tensor(t) else t)
        return sig

    def _build_table(self, part, device):
        """The chunk table as ONE int64 device array, built in numpy and uploaded from pinned memory without waiting
        for the device (a training loop that frees its gradients every step moves them, and the table with them):
        rows 0-3 the p / grad / exp_avg / exp_avg_sq addresses per chunk, row 4 the counts, row 5 viewed as int32 the
        parameter indices followed by the weight decays' fp32 bits; then the participating parameters' indices."""
        n_part = len(part)
        idx = np.array([i for i, _, _ in part], dtype=np.int32)
        wd = np.array([self.param_groups[gi]["weight_decay"] for _, gi, _ in part], dtype=np.float32)
        counts = np.array([p.numel() for _, _, p in part], dtype=np.int64)
        base = np.array([[p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                          self.state[p]["exp_avg_sq"].data_ptr()] for _, _, p in part], dtype=np.int64)
        per = (counts + _CHUNK - 1) // _CHUNK                  # chunks per tensor (none for an empty one)
        n_chunks = int(per.sum())
        if n_chunks > 0x7fffffff:
            raise HcirError("hcir.optim.Adam: more than 2^31 - 1 chunks")
        host = np.zeros(6 * n_chunks + (n_part + 1) // 2, dtype=np.int64)
        if n_chunks:
            which = np.repeat(np.arange(n_part), per)          # the tensor of each chunk
            off = (np.arange(n_chunks) - (np.cumsum(per) - per)[which]) * _CHUNK     # its first element
            rows = host[:6 * n_chunks].reshape(6, n_chunks)
            rows[:4] = base[which].T + 4 * off
            rows[4] = np.minimum(_CHUNK, counts[which] - off)
            aux = rows[5].view(np.int32)
            aux[:n_chunks] = idx[which]
            aux[n_chunks:].view(np.float32)[:] = wd[which]
        host[6 * n_chunks:].view(np.int32)[:n_part] = idx
        dev = torch.from_numpy(host).pin_memory().to(device, non_blocking=True)
        tab = dict(n_chunks=n_chunks, n_part=n_part, part_idx=dev[6 * n_chunks:].view(torch.int32))
        if n_chunks:
            tab["ptr"] = dev[:6 * n_chunks].view(6, n_chunks)
            aux = tab["ptr"][5].view(torch.int32)
            tab["pidx"], tab["wd"] = aux[:n_chunks], aux[n_chunks:].view(torch.float32)
            tab["partial"] = torch.empty(n_chunks, dtype=torch.float32, device=device)
            tab["flags"] = torch.empty(n_chunks, dtype=torch.int32, device=device)
        ends, n = [], 0
        for gi in range(len(self.param_groups)):
            n += sum(1 for _, g, _ in part if g == gi)
            ends.append(n)
        tab["group_end"] = (ctypes.c_int32 * len(ends))(*ends)
        self.table_rebuilds += 1
        return tab

    def _run(self, scaler: Optional[GradScaler], use_norm: bool, max_norm: Optional[float]):
        if len(self.param_groups) > _MAX_GROUPS:
            raise HcirError(f"hcir.optim.Adam: at most {_MAX_GROUPS} parameter groups")
        b1, b2, eps = self._hyper()
        sig = self._signature()
        if self._cache is not None and self._cache[0] == sig:
            _, tab, part, device = self._cache         # nothing moved since the checks and the table below were made
        else:
            self._cache = None
            part, n_params = self._participants()
            if not part:
                return None
            device = part[0][2].device
            if any(p.device != device for _, _, p in part):
                raise HcirError("hcir.optim.Adam: all parameters must be on one device")
            self._ensure_state(part, n_params, device)
            tab = self._build_table(part, device)
            self._cache = (self._signature(), tab, part, device)
        L = _lib.lib()
        st = torch.cuda.current_stream(device).cuda_stream
        ctl = torch.empty(4, dtype=torch.float32, device=device)
        n_chunks = tab["n_chunks"]
        scale_ptr = tracker_ptr = None
        if scaler is not None:
            scaler._lazy_init(device)
            scale_ptr, tracker_ptr = scaler._scale.data_ptr(), scaler._growth_tracker.data_ptr()
        ptr = tab.get("ptr")
        n_norm = n_chunks if use_norm else 0
        if n_norm:
            check(L.hcir_grad_sumsq(ptr[1].data_ptr(), ptr[4].data_ptr(), n_chunks, scale_ptr,
                                    tab["partial"].data_ptr(), tab["flags"].data_ptr(), st), "hcir_grad_sumsq")
        lrs = (ctypes.c_double * len(self.param_groups))(*[float(g["lr"]) for g in self.param_groups])
        check(L.hcir_optim_finalize(
            tab["partial"].data_ptr() if n_norm else None, tab["flags"].data_ptr() if n_norm else None, n_norm,
            scale_ptr, tracker_ptr,
            scaler._growth_factor if scaler else 1.0, scaler._backoff_factor if scaler else 1.0,
            scaler._growth_interval if scaler else 1, int(use_norm and max_norm is not None),
            float(max_norm) if max_norm is not None else 0.0, tab["group_end"], lrs, len(self.param_groups), b1, b2,
            tab["part_idx"].data_ptr(), tab["n_part"], self._steps.data_ptr(), self._aux[0].data_ptr(),
            self._aux[1].data_ptr(), ctl.data_ptr(), st), "hcir_optim_finalize")
        if n_chunks:
            check(L.hcir_adam_step(ptr[0].data_ptr(), ptr[1].data_ptr(), ptr[2].data_ptr(), ptr[3].data_ptr(),
                                   ptr[4].data_ptr(), tab["pidx"].data_ptr(), tab["wd"].data_ptr(), n_chunks,
                                   self._aux[0].data_ptr(), self._aux[1].data_ptr(), ctl.data_ptr(),
                                   float(np.float32(b2)), float(np.float32(1.0 - b1)), float(np.float32(1.0 - b2)),
                                   float(np.float32(eps)), st), "hcir_adam_step")
        # the kernels wrote through raw pointers: bump the version counters, on which VitTrainer.refresh, conv_train's
        # weight caches and hcir.vit_engine.EngineCache key
        for _, _, p in part:
            torch.autograd.graph.increment_version(p)
        return ctl

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def step(self, closure=None):
        """The plain step: inv_scale = 1, no clip, found_inf forced false.  A parameter whose .grad is None is skipped
        and its step count does not advance, as in torch."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run(None, use_norm=False, max_norm=None)
        return loss

    @torch.no_grad()
    def step_scaled(self, scaler: Optional[GradScaler] = None, max_norm: Optional[float] = 1.0) -> torch.Tensor:
        """unscale_ + non-finite check + clip_grad_norm_(max_norm) over exactly this optimizer's parameters that have
        a gradient + the step (skipped on a non-finite gradient) + scaler.update(), on the current stream, with no
        host read.  Returns the total norm of the unscaled gradients as a 0-d device tensor.  `scaler=None`: no
        scaling, and - as with torch's clip_grad_norm_ + step() - the step is taken whatever the norm is;
        `max_norm=None`: no clip.  The gradient buffers are not written."""
        if scaler is not None and not isinstance(scaler, GradScaler):
            raise HcirError(f"step_scaled takes an hcir.optim.GradScaler, not {type(scaler).__name__}: with "
                            "torch.amp.GradScaler use its own unscale_ / step / update around Adam.step()")
        ctl = self._run(scaler, use_norm=True, max_norm=max_norm)
        if ctl is None:
            raise HcirError("step_scaled: no parameter of the optimizer has a gradient")
        return ctl[0]
