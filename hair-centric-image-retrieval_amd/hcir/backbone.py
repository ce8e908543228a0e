"""hcir.backbone — the baseline wrappers of HP/src/backbone.py that are built,
with the reference's constructor signatures:

  SimCLR(model="resnet18")   HP/src/backbone.py:648-681  (the second definition, which wins)
  MAE(vit)                   HP/src/backbone.py:462-525  (pre-training forward on the kept tokens + the head_dim-32
                             decoder, fused masked-patch MSE loss, extract_features = encoder CLS; csrc/mae.hip,
                             csrc/attn_bwd32.hip)
  vit_base_patch16_224()     timm ctor the CLI passes to MAE (HP/knn_classification.py:146-147)
  SimMIM(vit)                HP/src/backbone.py:549-601  (pre-training forward, fused masked-patch L1 loss and
                             extract_features; the torchvision vit_b_16 of hcir.vit_train / hcir.vit_engine with
                             mask tokens in front of it and a Linear(768, 768) decoder behind it, csrc/mim.hip)
  random_token_mask(...)     lightly.models.utils.random_token_mask, which SimMIM draws its masks with
  DenseCL(backbone)          HP/src/backbone.py:123-161  (ResNet trunk without pool and fc, global and local heads, their
                             momentum twins; the trunk on hcir.conv_train.train_trunk_map / hcir.resnet_engine behind the
                             HipTrunkSwitches; the step's losses and matching are hcir.losses / hcir.dense)

  MSN(vit)                   HP/src/backbone.py:87-121   (target branch on the inference engine, anchor branch on the
                             kept tokens of hcir.vit_train's class-token exit with the position table interpolated for
                             focal views, MSNProjectionHead twins, prototypes; the criterion is hcir.losses.MSNLoss,
                             csrc/msn.hip)

The other SSL baselines of that file (BYOL, DINO, DINOv2, SiameseIMViT)
are comparison methods outside the hot path and are not built.
"""
from __future__ import annotations

import copy
from collections import OrderedDict
from functools import partial
from types import SimpleNamespace

import torch
from torch import nn

from . import _tv_resnet, models_vit, train_ops
from . import conv_train
from .main_backbone import HipTrunkSwitches, SimCLRProjectionHead, ViTWrapper, deactivate_requires_grad
from .resnet_engine import ResNetEngineCache, hip_trunk_active
from .vit_engine import EngineCache, VitLayer, VitSpec
from .vit_train import (MaeTrainer, VitTrainer, vit_cls_with_grad, vit_mae_mse_with_grad, vit_mae_with_grad,
                        vit_mim_l1_with_grad, vit_mim_with_grad)


class SimCLR(HipTrunkSwitches, nn.Module):
    def __init__(self, model="resnet18"):
        super().__init__()
        self.model = model
        print("Using backbone:", self.model)
        if model == "resnet18":
            backbone = _tv_resnet.resnet18(weights=None)
            self.backbone = nn.Sequential(*list(backbone.children())[:-1])
            proj_input_dim, output_dim = 512, 128
        elif model == "resnet50":
            backbone = _tv_resnet.resnet50(weights=None)
            self.backbone = nn.Sequential(*list(backbone.children())[:-1])
            proj_input_dim, output_dim = 2048, 1024
        elif model == "vit_b_16":
            self.backbone = ViTWrapper(weights=None)
            proj_input_dim, output_dim = 768, 512
        else:
            raise ValueError(f"Unsupported model: {model}")
        self.projection_head = SimCLRProjectionHead(proj_input_dim, proj_input_dim, output_dim)

    def forward(self, x):
        if "vit" in self.model:
            # The reference calls .flatten on ViTWrapper's (cls, pooled) TUPLE here and crashes
            # (HP/src/backbone.py:675-681).  Defined as SHAM2 does: project CLS.
            _, cls16 = self.backbone.forward_cls(x, want_f16=True)
            return self.projection_head.forward_hip(cls16)
        out = self._hip_features("backbone", x, self.projection_head)
        if out is not None:
            return out
        return self.projection_head(self.backbone(x).flatten(start_dim=1))

    def extract_features(self, x):
        if "vit" in self.model:
            return self.backbone.forward_cls(x)
        f = self._hip_features("backbone", x)
        if f is not None:
            return f
        return self.backbone(x).flatten(start_dim=1)


class _TimmViT(models_vit.VisionTransformer):
    """timm vit_base_patch16_224 container: like models_vit but WITH the final `norm`,
    a trainable pos_embed and no fc_norm (timm defaults: global_pool='token')."""

    def __init__(self, **kwargs):
        kwargs.setdefault("init_values", None)
        kwargs.setdefault("drop_path_rate", 0.0)
        super().__init__(global_pool=True, **kwargs)
        d = self.embed_dim
        del self.fc_norm
        self.norm = kwargs["norm_layer"](d)
        self.pos_embed = nn.Parameter(torch.randn(1, self.patch_embed.num_patches + 1, d) * 0.02)
        self.embed_dim = d


def vit_base_patch16_224(pretrained=False, **kwargs):
    if pretrained:
        raise ValueError("pretrained timm weights are not available offline; load a checkpoint")
    return _TimmViT(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                    norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


class _MaskedViT(nn.Module):
    """lightly MaskedVisionTransformerTIMM(vit=vit) container: keys backbone.vit.*, backbone.mask_token."""

    def __init__(self, vit):
        super().__init__()
        self.vit = vit
        self.mask_token = nn.Parameter(torch.zeros(1, 1, vit.embed_dim))
        self.sequence_length = vit.patch_embed.num_patches + 1


class _MaeDecoder(nn.Module):
    """lightly MAEDecoderTIMM, restated from its public sources (lightly is not installed: parity unpinned):
    decoder_embed Linear(embed_dim, dd), mask_token [1, 1, dd], decoder_pos_embed [1, T, dd] (2-D sin-cos, class token
    row zero, requires_grad=False), decoder_blocks = depth timm Blocks (qkv_bias, LayerNorm eps 1e-6), decoder_norm,
    decoder_pred Linear(dd, patch_size^2 in_chans).  Initialisation as lightly's _initialize_weights: mask_token normal
    std 0.02, Xavier-uniform Linear weights with zero biases, LayerNorm weights 1 and biases 0.  A parameter container:
    the arithmetic is hcir.vit_train.MaeTrainer."""

    def __init__(self, num_patches, patch_size, in_chans=3, embed_dim=768, decoder_embed_dim=512, decoder_depth=8,
                 decoder_num_heads=16, mlp_ratio=4.0):
        super().__init__()
        norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.num_heads = decoder_num_heads
        self.decoder_embed = nn.Linear(embed_dim, decoder_embed_dim, bias=True)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, decoder_embed_dim), requires_grad=False)
        self.decoder_blocks = nn.Sequential(*[
            models_vit.Block(decoder_embed_dim, decoder_num_heads, mlp_ratio, qkv_bias=True, norm_layer=norm_layer)
            for _ in range(decoder_depth)])
        self.decoder_norm = norm_layer(decoder_embed_dim)
        self.decoder_pred = nn.Linear(decoder_embed_dim, patch_size ** 2 * in_chans, bias=True)
        nn.init.normal_(self.mask_token, std=0.02)
        side = int(round(num_patches ** 0.5))
        if side * side == num_patches:
            self.decoder_pos_embed.data.copy_(sincos_2d_pos_embed(decoder_embed_dim, side))
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


def sincos_2d_pos_embed(dim: int, side: int) -> torch.Tensor:
    """The fixed 2-D sine-cosine position table of MAE (lightly's initialize_2d_sine_cosine_positional_embedding with a
    class token): [1, 1 + side^2, dim], row 0 zero; half the channels code one grid axis, half the other, each as
    [sin(p w_i), cos(p w_i)] with w_i = 10000^(-i / (dim / 4))."""
    if dim % 4:
        raise ValueError("sin-cos position embedding needs dim % 4 == 0")
    gh = torch.arange(side, dtype=torch.float64)
    grid = torch.meshgrid(gh, gh, indexing="xy")          # grid[0]: the column of a patch, grid[1]: its row

    def one_axis(pos):
        omega = 1.0 / 10000 ** (torch.arange(dim // 4, dtype=torch.float64) / (dim / 4.0))
        out = pos.reshape(-1)[:, None] * omega[None, :]
        return torch.cat([out.sin(), out.cos()], 1)

    emb = torch.cat([one_axis(grid[0]), one_axis(grid[1])], 1)
    return torch.cat([torch.zeros(1, dim, dtype=torch.float64), emb], 0).unsqueeze(0).float()


class MAE(nn.Module):
    """MAE(vit) of HP/src/backbone.py:462-525 on the HIP path; `vit` is vit_base_patch16_224() (timm's layout).
    State-dict keys are the reference's: backbone.vit.*, backbone.mask_token, decoder.* (lightly's MAEDecoderTIMM:
    decoder_embed, mask_token, decoder_pos_embed, decoder_blocks.{i}.*, decoder_norm, decoder_pred).  The decoder
    keywords are not reference arguments (it fixes 512 / 8 / 16); they let a test build a small model.

      forward(images)          -> (x_pred [b, n, P], target [b, n, P]) as the reference (:505-521), differentiable
      masked_loss(images)      -> nn.MSELoss()(x_pred, target) through hcir_mae_mse_fwd (the training step's path)
      extract_features(images) -> backbone.encode(images, idx_keep=None)[:, 0] (:523-525): timm forward (patch_embed,
                                  cls, + pos_embed, blocks, final norm), CLS row; inference-only
    idx_keep / idx_mask (int64 [b, k] / [b, n], lightly's random_token_mask pair) may be passed to the first two; they
    are validated here, on the host, before anything is launched: together they name every token of [0, T) once per
    image, and token 0 is kept (the reference's idx_mask - 1 would wrap for a masked class token).
    The encoder runs on the kept tokens only, the decoder (head_dim 32) on all of them: hcir.vit_train.MaeTrainer."""

    def __init__(self, vit, decoder_dim=512, decoder_depth=8, decoder_num_heads=16):
        super().__init__()
        self.mask_ratio = 0.75
        self.patch_size = vit.patch_embed.patch_size[0]
        self.backbone = _MaskedViT(vit)
        self.sequence_length = self.backbone.sequence_length
        self._cache = EngineCache()
        self.decoder = _MaeDecoder(num_patches=vit.patch_embed.num_patches, patch_size=self.patch_size,
                                   embed_dim=vit.embed_dim, decoder_embed_dim=decoder_dim,
                                   decoder_depth=decoder_depth, decoder_num_heads=decoder_num_heads, mlp_ratio=4.0)

    def _spec(self) -> VitSpec:
        vit = self.backbone.vit
        spec = models_vit.VisionTransformer._spec(vit)
        spec.final_ln_w, spec.final_ln_b = vit.norm.weight, vit.norm.bias
        return spec

    def _decoder_spec(self):
        dec = self.decoder
        layers = [VitLayer(ln1_w=blk.norm1.weight, ln1_b=blk.norm1.bias, qkv_w=blk.attn.qkv.weight,
                           qkv_b=blk.attn.qkv.bias, proj_w=blk.attn.proj.weight, proj_b=blk.attn.proj.bias,
                           ln2_w=blk.norm2.weight, ln2_b=blk.norm2.bias, fc1_w=blk.mlp.fc1.weight,
                           fc1_b=blk.mlp.fc1.bias, fc2_w=blk.mlp.fc2.weight, fc2_b=blk.mlp.fc2.bias)
                  for blk in dec.decoder_blocks]
        return SimpleNamespace(embed_w=dec.decoder_embed.weight, embed_b=dec.decoder_embed.bias,
                               mask_token=dec.mask_token, pos=dec.decoder_pos_embed, layers=layers,
                               heads=dec.num_heads, eps=dec.decoder_norm.eps, norm_w=dec.decoder_norm.weight,
                               norm_b=dec.decoder_norm.bias, pred_w=dec.decoder_pred.weight,
                               pred_b=dec.decoder_pred.bias)

    def trainer(self, device: torch.device) -> MaeTrainer:
        tr = getattr(self, "_trainer", None)
        if tr is None or tr.device != device:
            tr = MaeTrainer(self._spec(), self._decoder_spec(), device)
            self._trainer = tr
        return tr

    def _indices(self, images, idx_keep, idx_mask):
        """The index pair of a call: drawn here (trusted), or the caller's, checked on the host."""
        b, seq = images.shape[0], self.sequence_length
        if idx_keep is None and idx_mask is None:
            keep, mask = random_token_mask((b, seq), self.mask_ratio, device=images.device)
            return keep.contiguous(), mask.contiguous()
        for name, idx in (("idx_keep", idx_keep), ("idx_mask", idx_mask)):
            if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != b:
                raise ValueError(f"{name} must be an int64 tensor [{b}, k] (pass both or neither)")
        if idx_mask.shape[1] == 0:
            raise ValueError("no masked token: the loss over zero elements is undefined")
        both = torch.cat([idx_keep, idx_mask.to(idx_keep.device)], 1)
        if both.shape[1] != seq or not bool((both.sort(dim=1).values == torch.arange(seq, device=both.device)).all()):
            raise ValueError(f"idx_keep and idx_mask must together name every token of [0, {seq}) once per image")
        if not bool((idx_keep == 0).any(dim=1).all()):
            raise ValueError("token 0 (the class token) must be in idx_keep: it has no target patch")
        return idx_keep.to(images.device).contiguous(), idx_mask.to(images.device).contiguous()

    def forward(self, images, idx_keep=None, idx_mask=None):
        idx_keep, idx_mask = self._indices(images, idx_keep, idx_mask)                            # :507-511
        images = images.float().contiguous()
        x_pred = vit_mae_with_grad(self.trainer(images.device), images, idx_keep, idx_mask)      # :512-515
        b, n = idx_mask.shape
        target = train_ops.mim_patch_targets(images, idx_mask, self.patch_size).view(b, n, -1)   # :518-520
        return x_pred, target

    def masked_loss(self, images, idx_keep=None, idx_mask=None):
        """criterion(*model(images)) of the reference's step (nn.MSELoss, HP/src/pretrain_engine.py:330-331) as one
        differentiable 0-d loss: the target is never stored, the backward runs on the differences."""
        idx_keep, idx_mask = self._indices(images, idx_keep, idx_mask)
        return vit_mae_mse_with_grad(self.trainer(images.device), images, idx_keep, idx_mask)

    def extract_features(self, images):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("this model family is inference-only on the HIP path (the differentiable ViT is SHAM2 / ViTWrapper.forward_cls, hcir.vit_train): wrap the call in torch.no_grad()")
        eng = self._cache.get(list(self.backbone.vit.parameters()), self._spec, images.device)
        tok = eng.forward_tokens(images, cls_only_last=True)
        return eng.cls_embedding(tok, final_norm=True, l2_normalize=False)


def random_token_mask(size, mask_ratio: float = 0.6, mask_class_token: bool = False, device=None, generator=None):
    """lightly.models.utils.random_token_mask: (idx_keep [b, num_keep], idx_mask [b, T - num_keep]) token indices, a
    random permutation per image cut at num_keep = int(T (1 - mask_ratio)) (at least 1 where the class token is
    kept).  The class token (index 0) sorts first, so it is never masked, unless mask_class_token.  torch on the
    device: the table is [b, 197].  `generator` (not a lightly argument) makes the draw repeatable; one that lives on
    another device draws there."""
    b, seq = size
    num_keep = int(seq * (1 - mask_ratio))
    gdev = device if generator is None else generator.device
    noise = torch.rand(b, seq, device=gdev, generator=generator)
    if device is not None:
        noise = noise.to(device)
    if not mask_class_token and seq > 0:
        noise[:, 0] = -1
        num_keep = max(1, num_keep)
    indices = torch.argsort(noise, dim=1)
    return indices[:, :num_keep], indices[:, num_keep:]


class _MaskedTVViT(nn.Module):
    """lightly MaskedVisionTransformerTorchvision(vit=vit) container: keys backbone.vit.*, backbone.mask_token."""

    def __init__(self, vit):
        super().__init__()
        self.vit = vit
        self.mask_token = nn.Parameter(torch.zeros(1, 1, vit.hidden_dim))
        nn.init.normal_(self.mask_token, std=0.02)


class SimMIM(nn.Module):
    """SimMIM(vit) of HP/src/backbone.py:549-601 on the HIP path; `vit` is hcir._tv_vit.vit_b_16() (torchvision's
    layout).  State-dict keys are the reference's: backbone.vit.* (with heads.head.{weight,bias}, which its
    checkpoints carry because it hands lightly the whole vit_b_16; unused here and never given a gradient),
    backbone.mask_token, decoder.{weight,bias}.  lightly's encode() adds the position once (pos_mult = 1.0, unlike
    ViTWrapper).  Dropout is 0 in vit_b_16.

      forward(images)         -> (x_out [b, n, P], target [b, n, P]) as the reference, differentiable
      masked_loss(images)     -> nn.L1Loss()(x_out, target) through hcir_mim_l1_fwd (the training step's path)
      extract_features(images) -> class token after the final LayerNorm, of a forward with a FRESH random 75 % mask
                                 per call: a reference quirk (:570-578), kept; idx_mask [b, 0] embeds
                                 unmasked
    idx_mask (int64 [b, n], lightly's: token indices, distinct per image) may be passed to each; it is validated
    here, on the host, before anything is launched."""

    def __init__(self, vit):
        super().__init__()
        decoder_dim = vit.hidden_dim
        self.mask_ratio = 0.75
        self.patch_size = vit.patch_size
        self.sequence_length = vit.seq_length
        if not hasattr(vit, "heads"):       # the container omits torchvision's classification head; the checkpoints have it
            head = nn.Linear(vit.hidden_dim, 1000)
            nn.init.zeros_(head.weight)
            nn.init.zeros_(head.bias)
            vit.heads = nn.Sequential(OrderedDict([("head", head)]))
        self.backbone = _MaskedTVViT(vit)
        self.decoder = nn.Linear(decoder_dim, vit.patch_size ** 2 * 3)
        self._cache = EngineCache()

    # -- HIP engine / trainer ----------------------------------------------------------------------------------
    def _spec(self) -> VitSpec:
        vit = self.backbone.vit
        layers = []
        for blk in vit.encoder.layers:
            mha = blk.self_attention
            layers.append(VitLayer(
                ln1_w=blk.ln_1.weight, ln1_b=blk.ln_1.bias, qkv_w=mha.in_proj_weight, qkv_b=mha.in_proj_bias,
                proj_w=mha.out_proj.weight, proj_b=mha.out_proj.bias, ln2_w=blk.ln_2.weight, ln2_b=blk.ln_2.bias,
                fc1_w=blk.mlp[0].weight, fc1_b=blk.mlp[0].bias, fc2_w=blk.mlp[3].weight, fc2_b=blk.mlp[3].bias))
        return VitSpec(patch=vit.patch_size, dim=vit.hidden_dim, heads=vit.num_heads, eps=1e-6, pos_mult=1.0,
                       conv_w=vit.conv_proj.weight, conv_b=vit.conv_proj.bias, cls=vit.class_token,
                       pos=vit.encoder.pos_embedding, layers=layers, final_ln_w=vit.encoder.ln.weight,
                       final_ln_b=vit.encoder.ln.bias)

    def trainer(self, device: torch.device) -> VitTrainer:
        tr = getattr(self, "_trainer", None)
        if tr is None or tr.device != device:
            tr = VitTrainer(self._spec(), device, cls_only_last=False,
                            mim=(self.backbone.mask_token, self.decoder.weight, self.decoder.bias))
            self._trainer = tr
        return tr

    # -- masks -------------------------------------------------------------------------------------------------
    def _idx_mask(self, images, idx_mask, lowest: int, generator=None):
        """The mask of a call: drawn here (trusted), or the caller's, checked on the host: int64 [b, n] on the images'
        device, every index in [lowest, sequence_length), no index twice in a row."""
        b = images.shape[0]
        if idx_mask is None:
            return random_token_mask((b, self.sequence_length), self.mask_ratio, device=images.device,
                                     generator=generator)[1].contiguous()
        if not torch.is_tensor(idx_mask) or idx_mask.dtype != torch.int64 or idx_mask.dim() != 2 \
                or idx_mask.shape[0] != b:
            raise ValueError(f"idx_mask must be an int64 tensor [{b}, n]")
        if idx_mask.shape[1]:
            lo, hi = int(idx_mask.min()), int(idx_mask.max())
            if lo < lowest or hi >= self.sequence_length:
                raise ValueError(f"idx_mask holds token indices in [{lowest}, {self.sequence_length}); got {lo}..{hi}")
            s = idx_mask.sort(dim=1).values
            if bool((s[:, 1:] == s[:, :-1]).any()):
                raise ValueError("idx_mask names a token twice in one image")
        return idx_mask.to(images.device).contiguous()

    def _masked_idx(self, images, idx_mask):
        idx_mask = self._idx_mask(images, idx_mask, 1)       # a masked class token has no target patch
        if idx_mask.shape[1] == 0:
            raise ValueError("no masked token: the loss over zero elements is undefined")
        return idx_mask

    # -- the three calls ---------------------------------------------------------------------------------------
    def forward(self, images, idx_mask=None):
        idx_mask = self._masked_idx(images, idx_mask)
        images = images.float().contiguous()
        x_out = vit_mim_with_grad(self.trainer(images.device), images, idx_mask)                 # :589-593
        b, n = idx_mask.shape
        target = train_ops.mim_patch_targets(images, idx_mask, self.patch_size).view(b, n, -1)   # :596-599
        return x_out, target

    def masked_loss(self, images, idx_mask=None):
        """criterion(*model(images)) of the reference's step (nn.L1Loss, HP/src/pretrain_engine.py:83,520-522) as one
        differentiable 0-d loss: the target is never stored, the backward runs on the signs."""
        idx_mask = self._masked_idx(images, idx_mask)
        return vit_mim_l1_with_grad(self.trainer(images.device), images, idx_mask)

    def extract_features(self, images, idx_mask=None, generator=None):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("SimMIM.extract_features is inference-only on the HIP path: wrap the call in "
                                      "torch.no_grad(); forward / masked_loss are differentiable")
        idx_mask = self._idx_mask(images, idx_mask, 0, generator)
        eng = self._cache.get(list(self.backbone.vit.parameters()), self._spec, images.device)
        mask = None
        if idx_mask.shape[1]:
            mask = torch.zeros((images.shape[0], self.sequence_length), dtype=torch.uint8, device=images.device)
            mask.scatter_(1, idx_mask, 1)
        tok = eng.forward_tokens(images, cls_only_last=True, token_mask=mask, mask_token=self.backbone.mask_token)
        return eng.cls_embedding(tok, final_norm=True, l2_normalize=False)


def _tv_spec(vit) -> VitSpec:
    """The VitSpec of a torchvision-layout container as lightly's masked wrapper runs it: the position added once."""
    layers = []
    for blk in vit.encoder.layers:
        mha = blk.self_attention
        layers.append(VitLayer(
            ln1_w=blk.ln_1.weight, ln1_b=blk.ln_1.bias, qkv_w=mha.in_proj_weight, qkv_b=mha.in_proj_bias,
            proj_w=mha.out_proj.weight, proj_b=mha.out_proj.bias, ln2_w=blk.ln_2.weight, ln2_b=blk.ln_2.bias,
            fc1_w=blk.mlp[0].weight, fc1_b=blk.mlp[0].bias, fc2_w=blk.mlp[3].weight, fc2_b=blk.mlp[3].bias))
    return VitSpec(patch=vit.patch_size, dim=vit.hidden_dim, heads=vit.num_heads, eps=1e-6, pos_mult=1.0,
                   conv_w=vit.conv_proj.weight, conv_b=vit.conv_proj.bias, cls=vit.class_token,
                   pos=vit.encoder.pos_embedding, layers=layers, final_ln_w=vit.encoder.ln.weight,
                   final_ln_b=vit.encoder.ln.bias)


class MSNProjectionHead(nn.Module):
    """lightly.models.modules.MSNProjectionHead(input_dim=768, hidden_dim=2048, output_dim=256): Linear (no bias) -
    BatchNorm1d - GELU - Linear (no bias) - BatchNorm1d - GELU - Linear (bias); keys layers.{0,3}.weight,
    layers.{1,4}.{weight,bias,running_mean,running_var,num_batches_tracked}, layers.6.{weight,bias}.  A torch module,
    as DenseCL's heads are."""

    def __init__(self, input_dim: int = 768, hidden_dim: int = 2048, output_dim: int = 256):
        super().__init__()
        self.layers = nn.Sequential(
            nn.Linear(input_dim, hidden_dim, bias=False), nn.BatchNorm1d(hidden_dim), nn.GELU(),
            nn.Linear(hidden_dim, hidden_dim, bias=False), nn.BatchNorm1d(hidden_dim), nn.GELU(),
            nn.Linear(hidden_dim, output_dim, bias=True))

    def forward(self, x):
        return self.layers(x)


class MSN(nn.Module):
    """MSN(vit) of HP/src/backbone.py:87-121 on the HIP path; `vit` is hcir._tv_vit.vit_b_16() (torchvision's layout).
    State-dict keys are the reference's: backbone.vit.* (with heads.head.{weight,bias}, as SimMIM), backbone.mask_token,
    projection_head.layers.*, their anchor_backbone / anchor_projection_head twins, prototypes [1024, 256].  As in the
    reference the TARGET pair (backbone, projection_head) has requires_grad off and follows the anchor pair by
    update_momentum; the prototypes are a parameter the reference's step never gives a gradient (it passes
    prototypes.data to the criterion).  `hidden_dim` / `output_dim` / `num_prototypes` are not reference arguments
    (2048 / 256 / 1024 there); they let a test build a small model.

      forward(images)                 -> projection_head(backbone(images)): the target branch, no gradient, on the
                                         inference engine (hcir.vit_engine)
      forward_masked(images, idx_keep=None) -> anchor_projection_head(anchor_backbone(images, idx_keep)),
                                         differentiable: the blocks run on the kept tokens only
                                         (hcir.vit_train.vit_cls_with_grad), the position table is interpolated for
                                         an image whose patch grid differs from the stored one (focal views)
      extract_features(x)             -> backbone(x): the target branch's class token, under no_grad
    The reference draws the mask over (width // patch) ** 2 positions - the patch count, without the class token's
    slot - and applies the indices to the 1 + patches tokens: token 0 is always kept, the last patch never is, 166 of
    197 tokens are kept at 224 x 224 and 30 of 37 at 96 x 96.  Kept as it is.  A caller's idx_keep (int64
    [b, k], distinct token indices per image) is validated here, on the host, before anything is launched."""

    def __init__(self, vit, hidden_dim: int = 2048, output_dim: int = 256, num_prototypes: int = 1024):
        super().__init__()
        self.mask_ratio = 0.15
        if not hasattr(vit, "heads"):       # the container omits torchvision's classification head; the checkpoints have it
            head = nn.Linear(vit.hidden_dim, 1000)
            nn.init.zeros_(head.weight)
            nn.init.zeros_(head.bias)
            vit.heads = nn.Sequential(OrderedDict([("head", head)]))
        self.backbone = _MaskedTVViT(vit)
        self.projection_head = MSNProjectionHead(vit.hidden_dim, hidden_dim, output_dim)

        self.anchor_backbone = copy.deepcopy(self.backbone)
        self.anchor_projection_head = copy.deepcopy(self.projection_head)

        deactivate_requires_grad(self.backbone)
        deactivate_requires_grad(self.projection_head)

        self.prototypes = nn.Linear(output_dim, num_prototypes, bias=False).weight
        self._cache = EngineCache()

    def trainer(self, device: torch.device) -> VitTrainer:
        """The anchor branch's training walk (class-token exit, last block on the class-token rows)."""
        tr = getattr(self, "_trainer", None)
        if tr is None or tr.device != device:
            tr = VitTrainer(_tv_spec(self.anchor_backbone.vit), device, cls_only_last=True)
            self._trainer = tr
        return tr

    def _target_cls(self, images):
        vit = self.backbone.vit
        eng = self._cache.get(list(vit.parameters()), lambda: _tv_spec(vit), images.device)
        tok = eng.forward_tokens(images, cls_only_last=True)
        return eng.cls_embedding(tok, final_norm=True, l2_normalize=False)

    @torch.no_grad()
    def forward(self, images):
        return self.projection_head(self._target_cls(images))

    def _idx_keep(self, images, idx_keep):
        b, _, _, width = images.shape
        patch = self.anchor_backbone.vit.patch_size
        if idx_keep is None:
            seq_length = (width // patch) ** 2            # the reference's: no slot for the class token
            return random_token_mask((b, seq_length), self.mask_ratio, device=images.device)[0].contiguous()
        tokens = (images.shape[2] // patch) * (width // patch) + 1
        if not torch.is_tensor(idx_keep) or idx_keep.dtype != torch.int64 or idx_keep.dim() != 2 \
                or idx_keep.shape[0] != b or idx_keep.shape[1] == 0:
            raise ValueError(f"idx_keep must be an int64 tensor [{b}, k] with k >= 1")
        lo, hi = int(idx_keep.min()), int(idx_keep.max())
        if lo < 0 or hi >= tokens:
            raise ValueError(f"idx_keep holds token indices in [0, {tokens}); got {lo}..{hi}")
        srt = idx_keep.sort(dim=1).values
        if bool((srt[:, 1:] == srt[:, :-1]).any()):
            raise ValueError("idx_keep names a token twice in one image")
        return idx_keep.to(images.device).contiguous()

    def forward_masked(self, images, idx_keep=None):
        idx_keep = self._idx_keep(images, idx_keep)
        out = vit_cls_with_grad(self.trainer(images.device), images.float().contiguous(), idx_keep,
                                interpolate_pos=True)
        return self.anchor_projection_head(out)

    @torch.no_grad()
    def extract_features(self, x):
        return self._target_cls(x)


class DenseCLProjectionHead(nn.Module):
    """lightly.models.modules.DenseCLProjectionHead(input_dim, hidden_dim, output_dim): Linear -> ReLU -> Linear with
    biases and no BatchNorm; keys layers.{0,2}.{weight,bias}."""

    def __init__(self, input_dim: int = 2048, hidden_dim: int = 2048, output_dim: int = 512):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.ReLU(inplace=True),
                                    nn.Linear(hidden_dim, output_dim))

    def forward(self, x):
        return self.layers(x)


class DenseCL(HipTrunkSwitches, nn.Module):
    """DenseCL(backbone) of HP/src/backbone.py:123-161: `backbone` is a ResNet trunk without its pool and fc,
    nn.Sequential(*list(resnet50().children())[:-2]) (HP/mainpretrain.py:159-162), with a global and a local
    DenseCLProjectionHead(feature_dim, feature_dim, 512) and momentum twins of all three.  State-dict keys are the
    reference's: backbone.*, backbone_momentum.*, projection_head_{global,local}[_momentum].layers.{0,2}.{weight,bias}.
    `feature_dim` (not a reference argument; 2048 there) is the trunk's output width: 512 for a ResNet-18 trunk.

      forward(x)           -> (features [B, HW, C], global [B, 512], local [B, HW, 512]), differentiable
      forward_momentum(x)  -> the same three through the momentum modules, without gradient.  (The reference's method
                              runs the QUERY modules under no_grad, :150-157 - its momentum modules are updated and
                              never read.  Ours reads them, as lightly's DenseCL example and the method's name do.)
      extract_features(x)  -> pooled trunk features [B, C]

    HipTrunkSwitches: the 8-child trunk is handed to the 9-child code as a view
    nn.Sequential(*backbone.children(), pool) that shares the modules and is registered nowhere.  With hip_trunk an
    eval-mode extract_features under no_grad runs hcir.resnet_engine; with hip_train (and hip_train_norm /
    hip_train_stem on top) a train-mode forward / forward_momentum runs hcir.conv_train.train_trunk_map, whose fp16
    NHWC map IS the [B, HW, C] features: dense matching, the local head and the pool read it without a permute.  Off,
    everything is the torch path.  The two heads are torch modules either way."""

    def __init__(self, backbone, feature_dim: int = 2048):
        super().__init__()
        self.backbone = backbone
        self.projection_head_global = DenseCLProjectionHead(feature_dim, feature_dim, 512)
        self.projection_head_local = DenseCLProjectionHead(feature_dim, feature_dim, 512)

        self.backbone_momentum = copy.deepcopy(self.backbone)
        self.projection_head_global_momentum = copy.deepcopy(self.projection_head_global)
        self.projection_head_local_momentum = copy.deepcopy(self.projection_head_local)
        self.pool = nn.AdaptiveAvgPool2d((1, 1))

        deactivate_requires_grad(self.backbone_momentum)
        deactivate_requires_grad(self.projection_head_global_momentum)
        deactivate_requires_grad(self.projection_head_local_momentum)

    # -- the HIP paths -------------------------------------------------------------------------------------------
    def _trunk_view(self, which: str) -> nn.Sequential:
        """The 9-child trunk hcir.resnet_engine.layer_table expects, sharing the modules of attribute `which`; built
        per call (a few modules in a list) and never assigned to self, so it adds no state-dict key."""
        return nn.Sequential(*getattr(self, which).children(), self.pool)

    def trunk_engine(self, which: str, device: torch.device):
        caches = self.__dict__.setdefault("_trunk_caches", {})
        return caches.setdefault(which, ResNetEngineCache()).get(self._trunk_view(which), device)

    def _map_active(self, trunk: nn.Module, x: torch.Tensor, need_grad: bool) -> bool:
        # hip_train_active's conditions; a momentum trunk runs the same walk under no_grad
        return (bool(self.hip_train) and trunk.training and (torch.is_grad_enabled() or not need_grad) and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1 and x.shape[1] == 3
                and x.shape[2] >= 7 and x.shape[3] >= 7)

    def _three(self, which: str, head_global, head_local, x, need_grad: bool):
        trunk = getattr(self, which)
        if self._map_active(trunk, x, need_grad):
            fmap = conv_train.train_trunk_map(self._trunk_view(which), x, fused_norm=bool(self.hip_train_norm),
                                              fused_stem=bool(self.hip_train_stem))      # fp16 [B, h, w, C]
            b, h, w, c = fmap.shape
            features = fmap.view(b, h * w, c)
            pooled = self.pool(fmap.permute(0, 3, 1, 2).float()).flatten(start_dim=1)
            local_in = features if torch.is_autocast_enabled() else features.float()
            return features, head_global(pooled), head_local(local_in)
        features = trunk(x)
        glob = head_global(self.pool(features).flatten(start_dim=1))
        features = features.flatten(start_dim=2).permute(0, 2, 1)
        return features, glob, head_local(features)

    # -- the reference's three calls -----------------------------------------------------------------------------
    def forward(self, x):
        return self._three("backbone", self.projection_head_global, self.projection_head_local, x, True)

    @torch.no_grad()
    def forward_momentum(self, x):
        return self._three("backbone_momentum", self.projection_head_global_momentum,
                           self.projection_head_local_momentum, x, False)

    def extract_features(self, x):
        if hip_trunk_active(self.hip_trunk, self.backbone, x):
            return self.trunk_engine("backbone", x.device).forward(x)
        return self.pool(self.backbone(x)).flatten(start_dim=1)
