"""hcir.resnet_engine — the ResNet-18 / ResNet-50 trunk (nn.Sequential(children()[:-1]) of hcir._tv_resnet) in eval
mode on libhcir's convolution kernels (csrc/conv.hip): fused stem, implicit-GEMM convs with the folded BatchNorm,
residual add and ReLU in the epilogue, global average pool.  Activations NHWC fp16, inference only.

Replaces the torch trunk behind SHAM2.extract_features / extract_features_ema (HP/src/main_backbone.py:572-578,
624-629) and SimCLR.extract_features (HP/src/backbone.py:660-661) when the model's `hip_trunk` switch is on.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
from torch import nn

from . import ops
from ._lib import HcirError

GROUPS = ("stem", "layer1", "layer2", "layer3", "layer4", "avgpool")


def fold_bn(bn: nn.BatchNorm2d) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm as y = x * scale + bias: scale = gamma / sqrt(var + eps), bias = beta - mean * scale,
    computed in float64, stored fp32."""
    var = bn.running_var.detach().double()
    scale = bn.weight.detach().double() / torch.sqrt(var + bn.eps)
    bias = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return scale.float().contiguous(), bias.float().contiguous()


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [Cout, Cin, R, S] -> fp16 [Cout, R, S, Cin]: the GEMM's K order is (r, s, c), one tap = one
    contiguous NHWC pixel row."""
    return w.detach().permute(0, 2, 3, 1).contiguous().half()


def unpack_conv_weight(wp: torch.Tensor) -> torch.Tensor:
    """Inverse of pack_conv_weight (up to the fp16 rounding): [Cout, R, S, Cin] -> [Cout, Cin, R, S]."""
    return wp.permute(0, 3, 1, 2).contiguous()


def pack_stem_weight(w: torch.Tensor) -> torch.Tensor:
    """Stem weight [64, 3, 7, 7] -> fp16 [10, 2, 64, 8], the B-operand fragments of hcir_resnet_stem: element j of
    lane l at MFMA step kk, n tile nt is W[nt * 32 + (l & 31)][k = 16 kk + 8 (l >> 5) + j], k = (c * 7 + ky) * 7 + kx,
    zero for the padded k >= 147."""
    if tuple(w.shape) != (64, 3, 7, 7):
        raise HcirError(f"the stem kernel is Conv2d(3, 64, 7): got weight {tuple(w.shape)}")
    wk = torch.zeros(64, 160, dtype=torch.float32, device=w.device)
    wk[:, :147] = w.detach().float().reshape(64, 147)
    # [nt, r, kk, h, j] -> [kk, nt, h, r, j];  lane = h * 32 + r
    return wk.view(2, 32, 10, 2, 8).permute(2, 0, 3, 1, 4).contiguous().view(10, 2, 64, 8).half()


def conv_supported(r: int, s: int, stride: int, pad: int, cin: int, cout: int) -> bool:
    """The cases hcir_conv2d_f16 has a kernel for (csrc/conv_plan.h)."""
    return ((r, s, pad) in ((1, 1, 0), (3, 3, 1)) and stride in (1, 2) and cin > 0 and cout > 0
            and cin % 64 == 0 and cout % 64 == 0)


def trunk_out_hw(h: int, w: int) -> Tuple[int, int]:
    """Spatial size in front of the average pool: stem (two halvings), then the stride-2 convs of layer2..4
    (3x3 pad 1 and 1x1 pad 0 at stride 2 agree: (n - 1) // 2 + 1)."""
    h, w = ops.stem_out_size(h), ops.stem_out_size(w)
    for _ in range(3):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h, w


@dataclass
class ConvSpec:
    """One convolution of the trunk.  `inp` / `resid` / `out` name tensors inside the block: "x" is the block's
    input, "ds" the downsample branch, "o1" / "o2" the intermediate maps, "y" the block's output."""
    name: str
    group: str
    r: int
    stride: int
    pad: int
    cin: int
    cout: int
    relu: bool
    inp: str
    out: str
    resid: Optional[str]
    conv: nn.Conv2d
    bn: nn.BatchNorm2d


def _spec(name, group, conv, bn, relu, inp, out, resid=None) -> ConvSpec:
    r, s = conv.kernel_size
    st, pad = conv.stride[0], conv.padding[0]
    if (conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] or conv.groups != 1
            or conv.dilation != (1, 1) or conv.bias is not None
            or not conv_supported(r, s, st, pad, conv.in_channels, conv.out_channels)):
        raise HcirError(f"{name}: no HIP kernel for {conv} (hcir_conv2d_f16: 1x1 pad 0 or 3x3 pad 1, stride 1 or 2, "
                        "channels in multiples of 64)")
    _check_bn(name, bn)
    return ConvSpec(name, group, r, st, pad, conv.in_channels, conv.out_channels, relu, inp, out, resid, conv, bn)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _check_bn(name: str, bn) -> None:
    if (not isinstance(bn, nn.BatchNorm2d) or not bn.affine or not bn.track_running_stats
            or bn.running_mean is None or bn.running_var is None):
        raise HcirError(f"{name}: the engine folds an affine BatchNorm2d with running statistics, got {bn}")


def _check_stem(kids) -> None:
    """hcir_resnet_stem hard-codes Conv2d(3, 64, 7, stride 2, pad 3, no bias) -> BatchNorm2d -> ReLU ->
    MaxPool2d(3, stride 2, pad 1, floor) and the trunk ends in a global average pool: anything else is an error here,
    not another result."""
    conv, bn, relu, pool, avg = kids[0], kids[1], kids[2], kids[3], kids[8]
    if (conv.in_channels != 3 or conv.out_channels != 64 or _pair(conv.kernel_size) != (7, 7)
            or _pair(conv.stride) != (2, 2) or _pair(conv.padding) != (3, 3) or _pair(conv.dilation) != (1, 1)
            or conv.groups != 1 or conv.bias is not None):
        raise HcirError(f"stem: the HIP kernel is Conv2d(3, 64, 7, stride 2, pad 3, bias=False), got {conv}")
    _check_bn("stem", bn)
    if not isinstance(relu, nn.ReLU):
        raise HcirError(f"stem: expected ReLU after the BatchNorm, got {relu}")
    if (_pair(pool.kernel_size) != (3, 3) or _pair(pool.stride) != (2, 2) or _pair(pool.padding) != (1, 1)
            or _pair(pool.dilation) != (1, 1) or pool.ceil_mode):
        raise HcirError(f"stem: the HIP kernel pools 3 x 3 / stride 2 / pad 1 with floor sizes, got {pool}")
    if not isinstance(avg, nn.AdaptiveAvgPool2d) or _pair(avg.output_size) != (1, 1):
        raise HcirError(f"expected AdaptiveAvgPool2d((1, 1)) at the end of the trunk, got {avg}")


def block_table(blk: nn.Module, group: str = "", prefix: str = "") -> List[ConvSpec]:
    """The convolutions of one torchvision BasicBlock / Bottleneck, in execution order: the downsample conv first (it
    writes the residual); the last conv carries the residual add and the block's single ReLU.  The one description of
    a block's wiring: ResNetEngine.forward and conv_train.walk both run it."""
    table, resid = [], "x"
    if blk.downsample is not None:
        table.append(_spec(prefix + "downsample", group, blk.downsample[0], blk.downsample[1], False, "x", "ds"))
        resid = "ds"
    table.append(_spec(prefix + "conv1", group, blk.conv1, blk.bn1, True, "x", "o1"))
    if hasattr(blk, "conv3"):
        table.append(_spec(prefix + "conv2", group, blk.conv2, blk.bn2, True, "o1", "o2"))
        table.append(_spec(prefix + "conv3", group, blk.conv3, blk.bn3, True, "o2", "y", resid))
    else:
        table.append(_spec(prefix + "conv2", group, blk.conv2, blk.bn2, True, "o1", "y", resid))
    return table


def layer_table(trunk: nn.Sequential) -> List[ConvSpec]:
    """The trunk's convolutions after the stem, in execution order: block_table of every block of layer1..4."""
    kids = list(trunk.children())
    if len(kids) != 9 or not isinstance(kids[0], nn.Conv2d) or not isinstance(kids[3], nn.MaxPool2d):
        raise HcirError("expected nn.Sequential(conv1, bn1, relu, maxpool, layer1..4, avgpool)")
    _check_stem(kids)
    return [sp for li, layer in enumerate(kids[4:8], start=1) for bi, blk in enumerate(layer)
            for sp in block_table(blk, f"layer{li}", f"layer{li}.{bi}.")]


class ResNetEngine:
    """Packed fp16 weights + folded BatchNorms of one trunk on one device, and its activation buffers.

    Buffers are kept per (input shape, stream): five maps of the largest activation, handed round inside a block
    (x, ds, o1, o2, y - all five are live in a bottleneck with a downsample branch), so two streams never share one
    and a repeated shape allocates nothing.  Footprint of one entry: 5 x B x 56 x 56 x 256 x 2 B for ResNet-50 at 224^2
    = 8 MB per image (2 GB at B = 256), 2 MB per image for ResNet-18.  The MAX_SHAPES most recent (shape, stream)
    entries are kept (a loader's full batch and its last, smaller one); an older entry goes back to torch's allocator."""

    MAX_SHAPES = 2

    def __init__(self, trunk: nn.Sequential, device: torch.device):
        self.device = device
        kids = list(trunk.children())
        self.table = layer_table(trunk)
        self.stem_w = pack_stem_weight(kids[0].weight).to(device)
        s, b = fold_bn(kids[1])
        self.stem_scale, self.stem_bias = s.to(device), b.to(device)
        self.params = []
        for sp in self.table:
            s, b = fold_bn(sp.bn)
            self.params.append((pack_conv_weight(sp.conv.weight).to(device), s.to(device), b.to(device)))
        self.out_dim = self.table[-1].cout
        self._bufs = {}
        self.profiler = None   # an hcir.profiling.EventProfiler: mark() after every layer group

    def _shapes(self, b: int, h: int, w: int):
        """Output shape of every conv for a [b, 3, h, w] input, and the largest activation in elements."""
        hw = {"x": (ops.stem_out_size(h), ops.stem_out_size(w))}
        shapes, biggest = [], b * hw["x"][0] * hw["x"][1] * 64
        for sp in self.table:
            ih, iw = hw[sp.inp]
            oh, ow = ops.conv_out_size(ih, sp.r, sp.stride, sp.pad), ops.conv_out_size(iw, sp.r, sp.stride, sp.pad)
            hw[sp.out] = (oh, ow)
            if sp.out == "y":
                hw = {"x": (oh, ow)}
            shapes.append((b, oh, ow, sp.cout))
            biggest = max(biggest, b * oh * ow * sp.cout)
        return shapes, biggest

    def _buffers(self, b: int, h: int, w: int):
        key = (b, h, w, torch.cuda.current_stream(self.device).cuda_stream)
        ent = self._bufs.get(key)
        if ent is None:
            shapes, biggest = self._shapes(b, h, w)
            pool = [torch.empty(biggest, dtype=torch.float16, device=self.device) for _ in range(5)]
            ent = (shapes, pool, torch.empty((b, self.out_dim), dtype=torch.float32, device=self.device))
            if len(self._bufs) >= self.MAX_SHAPES:    # a sweep over shapes does not pin every shape's buffers
                self._bufs.pop(next(iter(self._bufs)))
            self._bufs[key] = ent
        return ent

    def forward(self, x: torch.Tensor, l2_normalize: bool = False) -> torch.Tensor:
        """x fp32 NCHW [B, 3, H, W] on the engine's device -> fp32 [B, 512 | 2048] (a fresh tensor)."""
        if x.device != self.device or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise HcirError(f"ResNetEngine.forward expects an fp32 [B,3,H,W] tensor on {self.device}, got "
                            f"{x.dtype} {tuple(x.shape)} on {x.device}")
        x = x.contiguous()
        b, _, h, w = x.shape
        shapes, pool, emb = self._buffers(b, h, w)
        prof = self.profiler
        free = list(pool)

        def take(shape):
            t = free.pop()
            return t[: shape[0] * shape[1] * shape[2] * shape[3]].view(shape), t

        cur, cur_store = take((b, ops.stem_out_size(h), ops.stem_out_size(w), 64))
        ops.resnet_stem(x, self.stem_w, self.stem_scale, self.stem_bias, out=cur)
        if prof is not None:
            prof.mark("stem")
        live = {"x": (cur, cur_store)}
        for i, (sp, (wt, scale, bias), shape) in enumerate(zip(self.table, self.params, shapes)):
            out, store = take(shape)
            resid = live[sp.resid][0] if sp.resid else None
            ops.conv2d_f16(live[sp.inp][0], wt, scale, bias, sp.stride, sp.pad, resid=resid, relu=sp.relu, out=out)
            live[sp.out] = (out, store)
            if sp.out == "y":      # end of the block: everything but its output goes back to the pool
                for k, (_, st) in live.items():
                    if k != "y":
                        free.append(st)
                live = {"x": live["y"]}
            if prof is not None and (i + 1 == len(self.table) or self.table[i + 1].group != sp.group):
                prof.mark(sp.group)
        ops.avgpool_nhwc(live["x"][0], l2_normalize=l2_normalize, out=emb)
        if prof is not None:
            prof.mark("avgpool")
        return emb.clone()


class ResNetEngineCache:
    """Builds the ResNetEngine lazily and rebuilds it when a parameter, a running statistic or the device changes:
    the rule of vit_engine.EngineCache, i.e. every call fingerprints (data_ptr, _version) of every tensor of the
    trunk - load_state_dict, optimizer steps, .to() and in-place ops bump one of the two.  A write through `p.data` or
    a raw pointer bumps neither: call invalidate() after such an edit."""

    def __init__(self):
        self._engine: Optional[ResNetEngine] = None
        self._key = None

    def invalidate(self) -> None:
        self._engine, self._key = None, None

    def get(self, trunk: nn.Sequential, device: torch.device) -> ResNetEngine:
        tensors = list(trunk.parameters()) + list(trunk.buffers())
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)
        if self._engine is None or key != self._key:
            prof = self._engine.profiler if self._engine is not None else None
            self._engine = ResNetEngine(trunk, device)
            self._engine.profiler = prof
            self._key = key
        return self._engine


def hip_trunk_active(enabled: bool, trunk: nn.Module, x: torch.Tensor) -> bool:
    """The conditions under which a model's `hip_trunk` switch routes a ResNet trunk through the engine: switched on,
    trunk in eval mode (running statistics), autograd and autocast off, and an input the kernels take - an fp32
    [B >= 1, 3, H >= 7, W >= 7] tensor on a HIP device.  Any other call keeps the torch path, whatever torch makes of it."""
    return (bool(enabled) and not trunk.training and not torch.is_grad_enabled() and x.is_cuda
            and not torch.is_autocast_enabled() and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1
            and x.shape[1] == 3 and x.shape[2] >= 7 and x.shape[3] >= 7)
