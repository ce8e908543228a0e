"""hcir.pretrain_engine — the HSimCLR training step of Trainer.train_one_epoch_SHAM on the MI355X hot path
(HP/src/pretrain_engine.py:602-757).

`SHAMTrainStep` is the body of the reference's batch loop (:618-751) with every hot operation on the HIP path:

    update_momentum(backbone / head -> momentum twins)        hcir.momentum         one launch (hcir_ema_update)
    NegSamplerRandomly / NegSamplerStatic                      hcir.neg_sampling     hcir_sim_topk
    model(neg), model(pos), model(anchor)                      hcir.vit_train        differentiable ViT forward
    positive_masking_transform(pos)                            hcir.transform        hcir_positive_masking
    model.forward_momentum(masked_pos)   (no grad)             hcir.vit_engine       inference engine
    F.normalize x 4                                            torch (B x 512 rows; autograd)
    TripletMarginLoss(margin, p=2, eps=1e-7)                   hcir.train_ops        hcir_triplet_margin_fwd / _bwd
    NTXentLoss(temperature)(pos, anchor)                       hcir.losses           hcir_ntxent_fwd / _bwd
    F.mse_loss(pos, masked_pos)                                hcir.train_ops        hcir_mse_fwd / _bwd
    total = contrastive + 0.5 triplet + 0.2 mse                (:735-742, ablation switches kept)
    scaler.scale(total).backward(); unscale_; clip_grad_norm_(1.0); scaler.step; scaler.update    (:745-749)
        with hcir.optim.Adam + hcir.optim.GradScaler           hcir.optim            hcir_grad_sumsq, hcir_optim_finalize,
                                                                                     hcir_adam_step: no host read
        with any other optimizer / scaler                      torch                 the five lines as written

    positive_transform(pos)  (RandomRotation + GaussianBlur)   hcir.transform        hcir_positive_transform
    projection head in train mode (Linear/BN/ReLU/Linear/BN)   hcir.head_train       hcir_gemm_f16 / _tn, hcir_bn1d_*

The step's DEFAULT path is the reference's default path: `positive_transform` on (ablation "No_pos_transform" turns
it off, :684-685), hard negatives mined once in the epoch that ends the warm-up with k from the previous epoch's margin
violations and cached per batch (:633-654), "fixed_hard" and "randomly" as in the reference.  The optimizer tail is
opt-in: with the optimizer of hcir.optim.get_optimizer (utils.get_optimizer, :108) and an hcir.optim.GradScaler (or no
scaler) unscale, clip, Adam and the loss-scale update run as three HIP launches with no host read, and the gradient
buffers keep what backward() left; with a torch.optim optimizer or a torch.amp.GradScaler those lines stay torch's.
What stays torch either way: the multiply of the loss by the scale and autograd's own bookkeeping — no vendor GEMM is
left in the step.  The data loader, the epoch bookkeeping, logging and checkpointing of the reference's Trainer are outside
the hot path.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch
import torch.nn.functional as F

from .dense import select_most_similar
from .losses import MSNLoss, NTXentLoss, SupConLoss
from . import optim as hcir_optim
from ._lib import HcirError
from .momentum import update_momentum
from .neg_sampling import NegSamplerRandomly, NegSamplerStatic
from .train_ops import TripletMarginLoss, mse_loss
from .transform import PositiveMaskingTransform, PositiveTransform


class SHAMTrainStep:
    def __init__(self, model, optimizer, scaler=None, temperature: float = 0.5, momentum: float = 0.99,
                 warm_up_epochs: int = 0, ablation: str = "None",
                 positive_transform: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 mask_ratio_range=(0.1, 0.5)):
        self.model = model
        self.optimizer = optimizer
        self.scaler = scaler
        self.momentum = momentum
        self.warm_up_epochs = warm_up_epochs
        self.ablation = ablation
        self.criterion1 = NTXentLoss(temperature=temperature)                                   # :93
        if ablation == "fixed_margin":
            self.triplet_loss_stage1 = self.triplet_loss_stage2 = TripletMarginLoss(margin=0.7, p=2, eps=1e-7)
        else:
            self.triplet_loss_stage1 = TripletMarginLoss(margin=0.7, p=2, eps=1e-7)             # :96
            self.triplet_loss_stage2 = TripletMarginLoss(margin=0.5, p=2, eps=1e-7)             # :97
        self.positive_masking_transform = PositiveMaskingTransform(mask_ratio_range=mask_ratio_range)   # :99
        # HP/utils/transform.py:21-24 applied at :686 unless ablation == "No_pos_transform" (:684-685); a caller may
        # pass its own callable
        self.positive_transform = positive_transform if positive_transform is not None else PositiveTransform()
        self.negative_batch_idx = []
        self.total_k = 0

    def hard_negative_k(self, prev_margin_violations: float, batch_size: int) -> int:
        """:636-642 — x = max(2, round((1 - v) * 10)) with v = the previous epoch's margin violations per sample
        (Python's round: ties to even, as in the reference)."""
        v = prev_margin_violations / batch_size
        return max(2, round((1 - v) * 10))

    def _negatives(self, x_pos_1, epoch, batch_id, prev_margin_violations, negative_idx):
        """:627-680.  Stage 1 (epoch + 1 < warm_up_epochs) and the "randomly" ablation draw random negatives.  In the
        epoch that ends the warm-up (epoch + 1 == warm_up_epochs) every batch is mined ONCE with the momentum model
        (NegSamplerStatic, k from the schedule above, fixed at batch 0) and its indices are cached; every later epoch
        re-uses the cache by batch id (the reference's loader order is fixed).  "fixed_hard" takes the cached / mined
        indices in every epoch — before the mining epoch the cache is empty and the reference raises IndexError."""
        model = self.model
        if negative_idx is not None:                       # caller-supplied indices (tests, external caches)
            return x_pos_1[negative_idx]
        stage1 = self.warm_up_epochs > epoch + 1
        if self.ablation == "randomly" or (stage1 and self.ablation != "fixed_hard"):
            return NegSamplerRandomly(x_pos_1)                                                  # :631,660
        if (epoch + 1) == self.warm_up_epochs:
            if batch_id == 0:
                self.negative_batch_idx = []                                                    # :635
                self.total_k = self.hard_negative_k(prev_margin_violations, x_pos_1.shape[0])   # :637-642
            self.negative_batch_idx.append(NegSamplerStatic(model, x_pos_1, k=self.total_k))    # :644,670
        if batch_id >= len(self.negative_batch_idx):
            raise IndexError(f"no cached hard-negative indices for batch {batch_id}: they are mined in epoch "
                             f"{self.warm_up_epochs - 1} (epoch + 1 == warm_up_epochs), HP/src/pretrain_engine.py:633-654")
        return x_pos_1[self.negative_batch_idx[batch_id]]                                       # :654,680

    def _check_clip_set(self):
        """The fused tail clips the optimizer's parameters that have a gradient; the reference clips
        model.parameters() (:747).  The two sets must be the same one."""
        in_opt = {id(p): (gi, k) for gi, g in enumerate(self.optimizer.param_groups)
                  for k, p in enumerate(g["params"]) if p.grad is not None}
        seen = set()
        for name, p in self.model.named_parameters():
            if p.grad is None:
                continue
            if id(p) not in in_opt:
                raise HcirError(f"fused optimizer tail: {name} has a gradient but is not a parameter of the optimizer; "
                                "clip_grad_norm_(model.parameters()) would include it")
            seen.add(id(p))
        for i, (gi, k) in in_opt.items():
            if i not in seen:
                p = self.optimizer.param_groups[gi]["params"][k]
                raise HcirError(f"fused optimizer tail: parameter {k} of optimizer group {gi} (shape "
                                f"{tuple(p.shape)}) has a gradient but is not in model.parameters(); "
                                "clip_grad_norm_(model.parameters()) would leave it out")

    def __call__(self, batch: Dict[str, torch.Tensor], epoch: int = 0, negative_idx: Optional[torch.Tensor] = None,
                 generator=None, batch_id: int = 0, prev_margin_violations: float = 0.0) -> Dict[str, float]:
        """One optimisation step on {'anchor', 'pos1'} image batches [B,3,224,224] (HIP device): the body of the
        reference's batch loop; `batch_id` and `prev_margin_violations` are the loop's own variables (:618, :602)."""
        model, opt, scaler = self.model, self.optimizer, self.scaler
        model.train()
        opt.zero_grad()
        update_momentum(model.backbone, model.backbone_momentum, m=self.momentum)                # :621
        update_momentum(model.projection_head, model.projection_head_momentum, m=self.momentum)  # :622
        x_anchor, x_pos_1 = batch["anchor"], batch["pos1"]
        stage1 = self.warm_up_epochs > epoch + 1
        negative_samples = self._negatives(x_pos_1, epoch, batch_id, prev_margin_violations, negative_idx)

        pos_samples = x_pos_1 if self.ablation == "No_pos_transform" else self.positive_transform(x_pos_1)   # :684-687
        # :683,689,690 — model(neg), model(pos), model(anchor): one 3B-row backbone pass, the head once per view
        if hasattr(model, "forward_views"):
            neg_batch, pos_batch, anchor_batch = model.forward_views([negative_samples, pos_samples, x_anchor])
        else:
            neg_batch, pos_batch, anchor_batch = model(negative_samples), model(pos_samples), model(x_anchor)
        if self.ablation == "No masked positive":
            masked_pos_samples = pos_samples
        else:
            masked_pos_samples = self.positive_masking_transform(pos_samples, generator=generator)   # :694
        with torch.no_grad():
            masked_pos_batch = model.forward_momentum(masked_pos_samples)                       # :696

        neg_batch = F.normalize(neg_batch.float(), p=2, dim=1)                                  # :699-702
        pos_batch = F.normalize(pos_batch.float(), p=2, dim=1)
        anchor_batch = F.normalize(anchor_batch.float(), p=2, dim=1)
        masked_pos_batch = F.normalize(masked_pos_batch.float(), p=2, dim=1)
        with torch.no_grad():                                                                   # :703-714
            pos_dist = torch.norm(anchor_batch - pos_batch, p=2, dim=1)
            neg_dist = torch.norm(anchor_batch - neg_batch, p=2, dim=1)
            margin = self.triplet_loss_stage1.margin if stage1 else self.triplet_loss_stage2.margin
            violations = (pos_dist - neg_dist + margin > 0)

        out = {}
        triplet_loss = mse = None
        if self.ablation != "No_Triplet":                                                       # :718-723
            crit = self.triplet_loss_stage1 if stage1 else self.triplet_loss_stage2
            triplet_loss = crit(anchor_batch, pos_batch, neg_batch)
        contrastive_loss = self.criterion1(pos_batch, anchor_batch)                             # :725
        if self.ablation != "No_MSE":
            mse = mse_loss(pos_batch, masked_pos_batch, reduction="mean")                      # :730
        if self.ablation == "No_Triplet":                                                       # :735-742
            total_loss = contrastive_loss + 0.2 * mse
        elif self.ablation == "No_MSE":
            total_loss = contrastive_loss + 0.5 * triplet_loss
        else:
            total_loss = contrastive_loss + 0.5 * triplet_loss + 0.2 * mse

        fused = isinstance(opt, hcir_optim.Adam) and (scaler is None or isinstance(scaler, hcir_optim.GradScaler))
        if fused:                       # :745-751 as three launches, no host read; the gradients stay scaled
            (scaler.scale(total_loss) if scaler is not None else total_loss).backward()
            self._check_clip_set()
            opt.step_scaled(scaler, max_norm=1.0)
        elif scaler is not None:                                                                # :745-749
            scaler.scale(total_loss).backward()
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
            scaler.step(opt)
            scaler.update()
        else:
            total_loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
            opt.step()
        zero = total_loss.new_zeros(())
        # one device-to-host read for the step's seven scalars
        vals = torch.stack([v.detach().float() for v in (
            total_loss, contrastive_loss, triplet_loss if triplet_loss is not None else zero,
            mse if mse is not None else zero, pos_dist.mean(), neg_dist.mean(), violations.sum())]).tolist()
        out.update(zip(("total", "contrastive", "triplet", "mse", "pos_dist", "neg_dist", "margin_violations"), vals))
        return out


class SupConTrainStep:
    """The body of Trainer.train_one_epoch_simclr_supcon's batch loop (HairPretraining/src/pretrain_engine.py:380-398),
    the reference CLIs' default --mode: the two SimCLR views through ONE model call, split and stacked to [B, 2, P],
    the criterion (hcir.losses.SupConLoss, hcir_supcon_fwd / _bwd) with the batch's labels, then
    scaler.scale(loss).backward(); scaler.step; scaler.update; zero_grad.  No gradient clipping: the reference does
    none here.  As in SHAMTrainStep the criterion sees fp32 features: the model runs its own precision, the loss
    kernels compute in the dtype they are handed.  -> {"loss": float}."""

    def __init__(self, model, optimizer, scaler=None, criterion=None):
        self.model = model
        self.optimizer = optimizer
        self.scaler = scaler
        self.criterion = criterion if criterion is not None else SupConLoss()                    # :76

    def __call__(self, batch: Dict[str, torch.Tensor], **_loop_state) -> Dict[str, float]:
        """One optimisation step on {'anchor', 'pos1', 'labels'}: image batches [B,3,H,W] and [B] integer labels on
        the HIP device.  The loop variables SHAMTrainStep takes (epoch, batch_id, ...) are accepted and unused."""
        model, opt, scaler = self.model, self.optimizer, self.scaler
        model.train()                                                                           # :377
        labels = batch["labels"]
        images = torch.cat([batch["anchor"], batch["pos1"]], dim=0)                             # :384
        bsz = labels.shape[0]                                                                   # :385
        features = model(images)                                                                # :387
        f1, f2 = torch.split(features, [bsz, bsz], dim=0)                                       # :388
        features = torch.cat([f1.unsqueeze(1), f2.unsqueeze(1)], dim=1).float()                 # :389
        loss = self.criterion(features, labels)                                                 # :390
        if scaler is not None:                                                                  # :394-397
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        opt.zero_grad()                                                                         # :398
        return {"loss": float(loss.detach())}


class SimMIMTrainStep:
    """The body of Trainer.train_one_epoch_simMIM's batch loop (HairPretraining/src/pretrain_engine.py:514-532) for an
    hcir.backbone.SimMIM model: one view per image, `predictions, targets = model(images)` and
    `criterion(predictions, targets)` (nn.L1Loss, :83) as the model's fused masked_loss (the walk, then
    hcir_mim_l1_fwd; the backward runs on the signs), then scaler.scale(loss).backward(); scaler.step; scaler.update;
    zero_grad.  No gradient clipping: the reference does none here.  -> {"loss": float}."""

    def __init__(self, model, optimizer, scaler=None):
        self.model = model
        self.optimizer = optimizer
        self.scaler = scaler

    def __call__(self, batch, **_loop_state) -> Dict[str, float]:
        """One optimisation step on an image batch [B,3,H,W] on the HIP device, or on a dict of views whose 'anchor'
        is that batch.  The loop variables SHAMTrainStep takes (epoch, batch_id, ...) are accepted and unused."""
        model, opt, scaler = self.model, self.optimizer, self.scaler
        model.train()
        images = batch["anchor"] if isinstance(batch, dict) else batch                          # :518-519
        loss = model.masked_loss(images)                                                        # :520-522
        if scaler is not None:                                                                  # :526-529
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        opt.zero_grad()                                                                         # :530
        return {"loss": float(loss.detach())}


class MAETrainStep:
    """The body of Trainer.train_one_epoch_mae's batch loop (HairPretraining/src/pretrain_engine.py:323-338) for an
    hcir.backbone.MAE model: one view per image, `predictions, targets = model(images)` and
    `criterion(predictions, targets)` (nn.MSELoss) as the model's fused masked_loss (the masked-encoder / decoder walk,
    then hcir_mae_mse_fwd; the backward runs on the differences), then scaler.scale(loss).backward(); scaler.step;
    scaler.update; zero_grad.  No gradient clipping: the reference does none here.  -> {"loss": float}."""

    def __init__(self, model, optimizer, scaler=None):
        self.model = model
        self.optimizer = optimizer
        self.scaler = scaler

    def __call__(self, batch, **_loop_state) -> Dict[str, float]:
        """One optimisation step on an image batch [B,3,H,W] on the HIP device, or on a dict of views whose 'anchor'
        is that batch.  The loop variables SHAMTrainStep takes (epoch, batch_id, ...) are accepted and unused."""
        model, opt, scaler = self.model, self.optimizer, self.scaler
        model.train()
        images = batch["anchor"] if isinstance(batch, dict) else batch                          # :328-329
        loss = model.masked_loss(images)                                                        # :330-331
        if scaler is not None:                                                                  # :334-337
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        opt.zero_grad()                                                                         # :338
        return {"loss": float(loss.detach())}


def cosine_schedule(step: int, max_steps: int, start_value: float, end_value: float) -> float:
    """lightly.utils.scheduler.cosine_schedule with its default period: the momentum of the DenseCL epoch,
    cosine_schedule(epoch, epochs, 0.996, 1) (HairPretraining/src/pretrain_engine.py:283)."""
    if step < 0 or max_steps < 1:
        raise ValueError("cosine_schedule needs step >= 0 and max_steps >= 1")
    if max_steps == 1:
        return end_value
    if step >= max_steps - 1:
        return end_value
    return end_value - (end_value - start_value) * (math.cos(math.pi * step / (max_steps - 1)) + 1) / 2


class DenseCLTrainStep:
    """The body of Trainer.train_one_epoch_densecl's batch loop (HairPretraining/src/pretrain_engine.py:284-315) for an
    hcir.backbone.DenseCL model: the three update_momentum calls (hcir.momentum, one launch each), the query view
    through the model and the key view through its momentum twins under fp16 autocast, the dense correspondence
    (hcir.dense.select_most_similar, hcir_dense_match_f16), the two criteria NTXentLoss(temperature,
    memory_bank_size=bank) on the [B, 512] global and the [B HW, 512] local rows (hcir_ntxent_bank_fwd / _bwd, each with
    its own queue), loss = (1 - lam) global + lam local, then scaler.scale(loss).backward(); scaler.step; scaler.update;
    zero_grad.  No gradient clipping: the reference does none here.  The caller supplies the epoch's `momentum`
    (cosine_schedule(epoch, epochs, 0.996, 1)).  The optimizer is whatever it is given: the reference's DenseCL branch
    (:109-115) names attributes this model does not have.  -> {"loss", "loss_global", "loss_local"}."""

    def __init__(self, model, optimizer, scaler=None, temperature: float = 0.5, bank=(4096, 512), lam: float = 0.5):
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lam weighs the local against the global loss and lies in [0, 1], got {lam}")
        self.model = model
        self.optimizer = optimizer
        self.scaler = scaler
        self.lam = lam
        self.criterion_global = NTXentLoss(temperature=temperature, memory_bank_size=bank)      # :85
        self.criterion_local = NTXentLoss(temperature=temperature, memory_bank_size=bank)       # :86

    def __call__(self, batch: Dict[str, torch.Tensor], momentum: float = 0.996, **_loop_state) -> Dict[str, float]:
        """One optimisation step on {'x_query', 'x_key'}: two views [B,3,H,W] of one image batch on the HIP device.
        The loop variables SHAMTrainStep takes (epoch, batch_id, ...) are accepted and unused."""
        model, opt, scaler = self.model, self.optimizer, self.scaler
        model.train()                                                                           # :279
        update_momentum(model.backbone, model.backbone_momentum, m=momentum)                    # :287-293
        update_momentum(model.projection_head_global, model.projection_head_global_momentum, m=momentum)
        update_momentum(model.projection_head_local, model.projection_head_local_momentum, m=momentum)
        x_query, x_key = batch["x_query"], batch["x_key"]
        with torch.autocast(device_type="cuda", dtype=torch.float16):                           # :285
            query_features, query_global, query_local = model(x_query)                          # :297
            key_features, key_global, key_local = model.forward_momentum(x_key)                 # :298
        key_local = select_most_similar(query_features, key_features, key_local)                # :300
        query_local = query_local.flatten(end_dim=1)                                            # :301-302
        key_local = key_local.flatten(end_dim=1)
        loss_global = self.criterion_global(query_global, key_global)                           # :304
        loss_local = self.criterion_local(query_local, key_local)                               # :305
        loss = (1 - self.lam) * loss_global + self.lam * loss_local                             # :306-307
        if scaler is not None:                                                                  # :312-314
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        opt.zero_grad()                                                                         # :315
        vals = torch.stack([loss.detach().float(), loss_global.detach(), loss_local.detach()]).tolist()   # one read
        return dict(zip(("loss", "loss_global", "loss_local"), vals))


class MSNTrainStep:
    """The body of Trainer.train_one_epoch_msn's batch loop (HairPretraining/src/pretrain_engine.py:246-270) for an
    hcir.backbone.MSN model: the two update_momentum calls at 0.996 (anchor -> target, hcir.momentum), views[0] through
    the target branch (no gradient, the inference engine), views[1] through forward_masked, views[2:] concatenated
    through a second forward_masked call (its own mask draw, its own BatchNorm batch statistics, the position table
    interpolated for the focal size), the criterion (hcir.losses.MSNLoss, hcir_msn_targets / _fwd / _bwd) on
    model.prototypes.data, then scaler.scale(loss).backward(); scaler.step; scaler.update; zero_grad.  The heads run
    under fp16 autocast as in the reference; the criterion sees fp32 rows, as in the other steps.  No gradient
    clipping: the reference does none here.  With no focal views the second call is skipped (the reference's
    torch.concat of an empty list would raise).  -> {"loss": float}."""

    def __init__(self, model, optimizer, scaler=None, criterion=None, momentum: float = 0.996):
        self.model = model
        self.optimizer = optimizer
        self.scaler = scaler
        self.momentum = momentum
        self.criterion = criterion if criterion is not None else MSNLoss()                       # :89

    @staticmethod
    def _views(batch):
        if isinstance(batch, dict):
            return [batch["anchor"], batch["pos1"]] + list(batch.get("focal", ()))
        views = list(batch)
        if len(views) < 2:
            raise ValueError("the MSN step needs a target view and an anchor view")
        return views

    def __call__(self, batch, **_loop_state) -> Dict[str, float]:
        """One optimisation step on a list of view batches [B,3,H,W] on the HIP device - views[0] the targets,
        views[1] the anchors, views[2:] the focal anchors, all of one size - or on a dict {'anchor', 'pos1'} (target,
        anchor) with an optional 'focal' list.  The loop variables SHAMTrainStep takes are accepted and unused."""
        model, opt, scaler = self.model, self.optimizer, self.scaler
        model.train()                                                                           # :243
        views = self._views(batch)
        update_momentum(model.anchor_backbone, model.backbone, m=self.momentum)                 # :248
        update_momentum(model.anchor_projection_head, model.projection_head, m=self.momentum)   # :249-251
        with torch.autocast(device_type="cuda", dtype=torch.float16):                           # :246
            targets_out = model(views[0])                                                       # :258-259
            anchors_out = model.forward_masked(views[1])                                        # :260
            if len(views) > 2:
                anchors_focal_out = model.forward_masked(torch.cat(views[2:], dim=0))           # :256,261
                anchors_out = torch.cat([anchors_out, anchors_focal_out], dim=0)                # :262
        loss = self.criterion(anchors_out.float(), targets_out.float(), model.prototypes.data)  # :264
        if scaler is not None:                                                                  # :267-269
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        opt.zero_grad()                                                                         # :270
        return {"loss": float(loss.detach())}
