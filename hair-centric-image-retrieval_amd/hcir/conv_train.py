"""hcir.conv_train — training the ResNet-18 / ResNet-50 body on libhcir's convolution kernels: a differentiable
convolution over fp16 NHWC activations and the fp32 master weight, and the train-mode walk of the trunk that uses it.

Serves the forward and backward of the torchvision Conv2d modules behind HP/src/main_backbone.py:576-579 in the step
of HP/src/pretrain_engine.py:682-747, which runs under torch.autocast(fp16): fp16 conv operands with fp32
accumulation are the reference's own arithmetic.  Opt-in through the model's `hip_train` switch.

  forward   hcir_conv2d_f16 with the identity epilogue (scale 1, bias 0, no residual, no ReLU)
  dx        hcir_conv2d_f16 again, over dy with wT[c][r'][s'][n] = w[n][R-1-r'][S-1-s'][c]:
              stride 1           dx = conv(dy, wT, stride 1, same pad)
              1x1 stride 2       t = conv(dy, wT) at Ho x Wo, dx = spread2(t)   (dx[2i][2j] = t[i][j], zero elsewhere)
              3x3 stride 2       z = spread2(dy) at H x W, dx = conv(z, wT, stride 1, pad 1): 4x the useful flops on
                                 the three stride-2 3x3 layers of a trunk (a parity-class kernel is later work)
  dW        hcir_conv2d_wgrad_f16 (csrc/conv_bwd.hip), fp32 [Cout,R,S,Cin], permuted back to [Cout,Cin,R,S] and
            handed to autograd, whose own accumulation sums the views of a step

The stem (Conv 7x7, BatchNorm, ReLU, MaxPool: 3 % of the flops, Cin = 3 fits none of the kernels), every BatchNorm2d
(batch statistics, running-statistic updates), ReLU, the residual adds and the average pool stay the trunk's own torch
modules, called on channels-last fp16 tensors.  torch's batch norm takes fp16 input with fp32 parameters as it does
under autocast (batch_norm is on neither autocast list: it runs in its input's dtype), so no autocast region is needed.

With the model's second switch, `hip_train_norm`, on as well, the body's BatchNorm2d layers leave torch too
(train_trunk with fused_norm=True): bn_act_nhwc runs batch statistics, normalisation, the block's residual add and its
ReLU as one pass over the fp16 NHWC map, forward and backward (hcir_bn2d_fwd_nhwc_f16 / hcir_bn2d_bwd_nhwc_f16,
csrc/bn2d.hip), and updates the module's running statistics in the kernel.  The stem, the cast to fp16 NHWC and the
average pool stay torch's on that path.

With the third switch, `hip_train_stem` (independent of the second), the stem leaves torch as well (train_trunk with
fused_stem=True): stem_train maps the fp32 NCHW image to the fp16 NHWC [B,Hp,Wp,64] map the walk starts from, with no
permute or cast in between (csrc/stem_train.hip):

  forward   hcir_stem_conv_f16 (the pre-norm map c, fp16 NHWC), hcir_bn2d_stats_nhwc_f16 (batch statistics; running
            statistics updated in the kernel), hcir_stem_bn_relu_pool_f16 (normalise + ReLU + max pool in one pass)
  backward  hcir_stem_pool_relu_bwd_f16 (the gradient at the conv map: torch's first-maximum rule, found on c itself),
            hcir_bn2d_bwd_nhwc_f16 over it (dc, dgamma, dbeta), hcir_stem_wgrad_f16 (dW, fp32 [64,3,7,7])

The image needs no gradient, and there is no image-gradient kernel: when x.requires_grad, train_trunk keeps the torch
stem.  The packed stem weight is cached per parameter by _WeightCache's rule (stem_weights).

All paths are one walk (walk) over resnet_engine's table of the body - which conv feeds which, where the residual
enters, where the ReLU sits are written down there, once - with one of two `norm` callables: torch_norm or bn_act_nhwc.
"""
from __future__ import annotations

import weakref
from typing import Callable, Sequence, Tuple

import torch
from torch import nn

from . import ops
from ._lib import HcirError
from .resnet_engine import ConvSpec, layer_table, pack_conv_weight, pack_stem_weight


class _WeightCache:
    """Per parameter: the fp16 packed weight [Cout,R,S,Cin] and its flipped transpose [Cin,R,S,Cout], refreshed when
    the parameter's (_version, data_ptr, device) changes - an optimizer step, load_state_dict, .to() - as VitTrainer
    does for the ViT's operand copies.  A write through `p.data` bumps none of them: call clear() after such an edit."""

    def __init__(self, pack: Callable = None):
        self._ent = {}    # id(parameter) -> (weak reference, key, w16, wt16); a tensor's == is elementwise, so no
                          # WeakKeyDictionary
        # what is kept per parameter: a tuple of copies (the stem keeps one, in pack_stem_weight's layout)
        self._pack = pack or (lambda w: (pack_conv_weight(w), flip_transpose_packed(w)))

    def clear(self) -> None:
        self._ent.clear()

    def get(self, w: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        key = (w._version, w.data_ptr(), str(w.device))
        ent = self._ent.get(id(w))
        if ent is None or ent[0]() is not w or ent[1] != key:
            ents, i = self._ent, id(w)

            def drop(ref):    # the parameter died: forget its copies, unless the id already belongs to a new one
                if i in ents and ents[i][0] is ref:
                    del ents[i]

            ent = (weakref.ref(w, drop), key, *self._pack(w))
            ents[i] = ent
        return ent[2:]


def flip_transpose_packed(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,R,S] -> fp16 [Cin,R,S,Cout] with both taps reversed: the packed weight of the data-gradient conv."""
    return pack_conv_weight(w.detach().flip(2, 3).permute(1, 0, 2, 3))


weights = _WeightCache()
stem_weights = _WeightCache(lambda w: (pack_stem_weight(w),))
_identity = {}


def _identity_epilogue(device: torch.device, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (str(device), n)
    ent = _identity.get(key)
    if ent is None:
        ent = (torch.ones(n, dtype=torch.float32, device=device), torch.zeros(n, dtype=torch.float32, device=device))
        _identity[key] = ent
    return ent


def _conv(x: torch.Tensor, w16: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    one, zero = _identity_epilogue(x.device, w16.shape[0])
    return ops.conv2d_f16(x, w16, one, zero, stride, pad)


def conv2d_dgrad(dy: torch.Tensor, wt16: torch.Tensor, h: int, w: int, stride: int, pad: int) -> torch.Tensor:
    """dx fp16 [B,h,w,Cin] of a convolution whose input was h x w: dy fp16 [B,Ho,Wo,Cout], wt16 from
    flip_transpose_packed."""
    r = wt16.shape[1]
    if stride == 1:
        return _conv(dy, wt16, 1, pad)
    if stride != 2 or (r, pad) not in ((1, 0), (3, 1)):
        raise HcirError(f"conv2d_dgrad: no plan for a {r}x{r} / {stride} / pad {pad} convolution")
    if r == 1:
        return ops.spread2_nhwc(_conv(dy, wt16, 1, 0), h, w)
    return _conv(ops.spread2_nhwc(dy, h, w), wt16, 1, 1)


class _Conv2dNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.dtype != torch.float32:
            raise HcirError(f"conv2d_nhwc expects an fp32 [Cout,Cin,R,R] weight, got {weight.dtype} "
                            f"{tuple(weight.shape)}")
        x = x.contiguous()
        w16, wt16 = weights.get(weight)
        ctx.save_for_backward(x)
        ctx.wt16, ctx.r, ctx.stride, ctx.pad = wt16, weight.shape[2], stride, pad
        return _conv(x, w16, stride, pad)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(dy, ctx.wt16, x.shape[1], x.shape[2], ctx.stride, ctx.pad)
        if ctx.needs_input_grad[1]:
            dw = ops.conv2d_wgrad(x, dy, ctx.r, ctx.stride, ctx.pad).permute(0, 3, 1, 2).contiguous()
        return dx, dw, None, None


def conv2d_nhwc(x: torch.Tensor, weight: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """Differentiable convolution: x fp16 NHWC [B,H,W,Cin], weight the module's fp32 [Cout,Cin,R,R] parameter ->
    fp16 NHWC [B,Ho,Wo,Cout].  Shapes without a kernel raise HcirError."""
    return _Conv2dNHWC.apply(x, weight, stride, pad)


# --------------------------------------------- `hip_train_norm`: BatchNorm2d + residual + ReLU on HIP (bn_act_nhwc)
class _BnActNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, resid, bn, relu):
        x = x.contiguous()
        if resid is not None:
            resid = resid.contiguous()
        # the running statistics are updated by the kernel, in place, outside autograd's view (buffers, no gradient)
        y, mean, rstd = ops.bn2d_fwd(x, weight, bias, bn.eps, bn.momentum, resid, relu, bn.running_mean,
                                     bn.running_var)
        ctx.save_for_backward(x, weight, mean, rstd, *((y,) if relu else ()))
        ctx.relu, ctx.has_resid = relu, resid is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors[:4]
        y = ctx.saved_tensors[4] if ctx.relu else None
        dy = dy.contiguous()
        want_resid = ctx.has_resid and ctx.needs_input_grad[3]
        dx, dresid, dgamma, dbeta = ops.bn2d_bwd(dy, x, y, weight, mean, rstd, want_dresid=want_resid and ctx.relu)
        if want_resid and not ctx.relu:
            dresid = dy                                   # no mask: the residual branch's gradient is dy itself
        return dx, dgamma, dbeta, dresid, None, None


def bn_act_nhwc(x: torch.Tensor, bn: nn.BatchNorm2d, resid: torch.Tensor = None, relu: bool = False) -> torch.Tensor:
    """Differentiable train-mode `relu?(bn(x) (+ resid))`: x and resid fp16 NHWC [B,H,W,C] -> fp16 [B,H,W,C].  Batch
    statistics; bn.running_mean / running_var are updated with bn.momentum and bn.num_batches_tracked counts the call,
    as the module's own forward does.  A module this has no kernel for raises HcirError."""
    if not isinstance(bn, nn.BatchNorm2d) or bn.momentum is None or not bn.affine or not bn.track_running_stats \
            or not bn.training:
        raise HcirError("bn_act_nhwc needs a train-mode BatchNorm2d with affine=True, track_running_stats=True and a "
                        f"numeric momentum, got {bn!r} (training={getattr(bn, 'training', None)})")
    y = _BnActNHWC.apply(x, bn.weight, bn.bias, resid, bn, bool(relu))
    bn.num_batches_tracked.add_(1)
    return y


# ------------------------------------- `hip_train_stem`: conv 7x7 + BatchNorm2d + ReLU + MaxPool on HIP (stem_train)
class _StemTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bn):
        x = x.contiguous()
        (wp,) = stem_weights.get(weight)
        c = ops.stem_conv(x, wp)
        # the running statistics are updated by the kernel, in place, outside autograd's view (buffers, no gradient)
        mean, rstd = ops.bn2d_stats(c, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
        p = ops.stem_bn_relu_pool(c, gamma, beta, mean, rstd)
        ctx.save_for_backward(x, c, gamma, beta, mean, rstd)
        return p

    @staticmethod
    def backward(ctx, dp):
        x, c, gamma, beta, mean, rstd = ctx.saved_tensors
        g = ops.stem_pool_relu_bwd(dp.contiguous(), c, gamma, beta, mean, rstd)
        dc, _, dgamma, dbeta = ops.bn2d_bwd(g, c, None, gamma, mean, rstd)
        dw = ops.stem_wgrad(x, dc) if ctx.needs_input_grad[1] else None
        return None, dw, dgamma, dbeta, None


def stem_train(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d) -> torch.Tensor:
    """Differentiable train-mode `maxpool(relu(bn(conv(x))))` of the trunk's stem: x fp32 NCHW [B,3,H,W] -> fp16 NHWC
    [B,Hp,Wp,64], the walk's input as it is.  Differentiable in conv.weight, bn.weight and bn.bias, NOT in x: there
    is no image-gradient kernel, and a caller whose image requires a gradient must keep the torch stem (train_trunk
    does).  Batch statistics; bn.running_mean / running_var are updated with bn.momentum and bn.num_batches_tracked
    counts the call.  The conv / pool structure is layer_table's to check; a BatchNorm2d the kernels cannot serve
    raises HcirError, the conditions being bn_act_nhwc's."""
    if not isinstance(bn, nn.BatchNorm2d) or bn.momentum is None or not bn.affine or not bn.track_running_stats \
            or not bn.training:
        raise HcirError("stem_train needs a train-mode BatchNorm2d with affine=True, track_running_stats=True and a "
                        f"numeric momentum, got {bn!r} (training={getattr(bn, 'training', None)})")
    if x.requires_grad:
        raise HcirError("stem_train has no gradient with respect to the image")
    p = _StemTrain.apply(x, conv.weight, bn.weight, bn.bias, bn)
    bn.num_batches_tracked.add_(1)
    return p


# ------------------------------------------------------------------------------------ the train-mode walk of the body
def torch_norm(y: torch.Tensor, bn: nn.BatchNorm2d, resid: torch.Tensor = None, relu: bool = False) -> torch.Tensor:
    """bn_act_nhwc's contract on the module's own torch forward (`hip_train` alone): BatchNorm2d sees the logical
    [B,C,H,W] view of the NHWC map, as under channels-last; the ReLU is in place, as torchvision's block.relu is."""
    y = bn(y.permute(0, 3, 1, 2))
    if resid is not None:
        y = y + resid.permute(0, 3, 1, 2)
    if relu:
        y = torch.relu_(y)
    return y.permute(0, 2, 3, 1)


def conv_nhwc(a: torch.Tensor, sp: ConvSpec) -> torch.Tensor:
    return conv2d_nhwc(a, sp.conv.weight, sp.stride, sp.pad)


def walk(table: Sequence[ConvSpec], a: torch.Tensor, conv: Callable = conv_nhwc,
         norm: Callable = bn_act_nhwc) -> torch.Tensor:
    """The train-mode pass over resnet_engine's table (block_table of one block, layer_table of a trunk) on plain NHWC
    tensors [B,H,W,C]: per spec `norm(conv(input, spec), spec.bn, residual, spec.relu)`, the tensors named as in
    ConvSpec.  A block's output "y" is the next block's "x", and nothing else outlives the block."""
    live = {"x": a}
    for sp in table:
        live[sp.out] = norm(conv(live[sp.inp], sp), sp.bn, live[sp.resid] if sp.resid else None, sp.relu)
        if sp.out == "y":
            live = {"x": live["y"]}
    return live["x"]


def train_trunk(trunk: nn.Sequential, x: torch.Tensor, fused_norm: bool = False,
                fused_stem: bool = False) -> torch.Tensor:
    """The differentiable train-mode walk of nn.Sequential(children()[:-1]): x fp32 [B,3,H,W] -> fp32 [B,C].  The stem,
    the one cast to fp16 NHWC and the fp32 average pool are torch's; the body's BatchNorm2d, residual adds and ReLUs
    are torch's as well (torch_norm) unless `fused_norm` puts them on bn_act_nhwc.  `fused_stem` replaces the torch
    stem and the cast by stem_train, unless x requires a gradient (there is no image-gradient kernel: the torch stem
    runs then).  The table is rebuilt, and with it resnet_engine's structure checks (stem, pooling, every body conv
    has a kernel) are repeated, on every call: an edited trunk raises HcirError whenever the edit was made (host cost:
    DESIGN.md §3.4)."""
    a = _trunk_map(trunk, x, fused_norm, fused_stem)
    return list(trunk.children())[8](a.permute(0, 3, 1, 2).float()).flatten(start_dim=1)


def _trunk_map(trunk: nn.Sequential, x: torch.Tensor, fused_norm: bool, fused_stem: bool) -> torch.Tensor:
    table = layer_table(trunk)
    kids = list(trunk.children())
    if fused_stem and not x.requires_grad:
        a = stem_train(x, kids[0], kids[1])
    else:
        a = kids[3](kids[2](kids[1](kids[0](x)))).permute(0, 2, 3, 1).contiguous().half()
    return walk(table, a, norm=bn_act_nhwc if fused_norm else torch_norm)


def train_trunk_map(trunk: nn.Sequential, x: torch.Tensor, fused_norm: bool = False,
                    fused_stem: bool = False) -> torch.Tensor:
    """train_trunk without its final pool: x fp32 [B,3,H,W] -> the last stage's fp16 NHWC map [B,h,w,C], which read as
    [B, h*w, C] is the layout dense matching and a per-position head take (hcir.backbone.DenseCL).  `trunk` is the
    9-child nn.Sequential layer_table checks; its pool is not run.  Under no_grad (a momentum trunk) the same kernels
    run forward only: batch statistics, running-stat updates included."""
    return _trunk_map(trunk, x, fused_norm, fused_stem)


def hip_train_active(enabled: bool, trunk: nn.Module, x: torch.Tensor) -> bool:
    """The conditions under which a model's `hip_train` switch routes a ResNet trunk through train_trunk: switched
    on, trunk in train mode, autograd on, and an fp32 [B >= 1, 3, H >= 7, W >= 7] tensor on a HIP device.  Any other
    call keeps the code it had."""
    return (bool(enabled) and trunk.training and torch.is_grad_enabled() and x.is_cuda
            and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1 and x.shape[1] == 3
            and x.shape[2] >= 7 and x.shape[3] >= 7)
