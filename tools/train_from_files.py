#!/usr/bin/env python
"""An epoch of SHAMTrainStep (--mode supcon: SupConTrainStep, --mode simmim: SimMIMTrainStep, --mode densecl:
DenseCLTrainStep, --mode mae: MAETrainStep, --mode msn: MSNTrainStep) fed from an annotation CSV + image directory, input on the device.

    python tools/train_from_files.py --csv data/data_train.csv --img-dir data/train --batch-size 1024

The loader workers only read and stage the files (EncodedDataset + collate_train_views).  The H2D copy, the whole-image
decode, the crops and the SimCLR augmentations of batch i + 1 run on a side stream while the step of batch i runs on
the main stream (the stream / ownership pattern of hcir.pipeline): the consumer stream waits on the producer, and what
crosses is recorded on the consumer (record_stream) so the allocator does not hand it out under the step.
"""
import argparse
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))


def train_epoch(step, loader, device="cuda", generator=None, epoch: int = 0, prev_margin_violations: float = 0.0,
                on_step=None, with_labels: bool = False, view_kwargs=None, view_names=None, step_kwargs=None):
    """One pass over `loader` (batches are hcir.dataloader.TrainViewBatch).  -> list of the step's loss dicts.
    with_labels (--mode supcon): the batch's class labels travel with the views as views["labels"].
    view_kwargs: keywords of hcir.views.simclr_views (min_scale, cj_prob, ...) for the batch's views.
    view_names (--mode densecl): {"anchor": "x_query", "pos1": "x_key"} renames the two views for the step.
    step_kwargs: further keywords of every step call (--mode densecl: the epoch's momentum)."""
    device = torch.device(device)
    side = torch.cuda.Stream(device=device)
    main = torch.cuda.current_stream(device)

    def produce(batch):   # enqueue only: nothing here waits for the device
        with torch.cuda.stream(side):
            views, check = batch.views(device, generator, defer_check=True, **(view_kwargs or {}))
            if view_names:
                views = {view_names.get(k, k): v for k, v in views.items()}
            if with_labels:
                views["labels"] = batch.labels.to(device, non_blocking=True)
            return views, check

    it = iter(loader)
    first = next(it, None)
    pending = produce(first) if first is not None else None
    results, batch_id = [], 0
    while pending is not None:
        views, check = pending
        main.wait_stream(side)                # batch i is complete before the step reads it
        for t in views.values():
            t.record_stream(main)             # allocated on `side`, consumed on `main`
        nxt = next(it, None)
        pending = produce(nxt) if nxt is not None else None    # batch i + 1: runs beside the step below
        check()                               # batch i's decoder status (raises with the file names)
        out = step(views, epoch=epoch, batch_id=batch_id, prev_margin_violations=prev_margin_violations,
                   **(step_kwargs or {}))
        results.append(out)
        if on_step is not None:
            on_step(batch_id, out)
        batch_id += 1
    return results


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csv", required=True)
    ap.add_argument("--img-dir", required=True)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--model", default="vit_b_16")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--warm-up-epochs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mode", choices=("sham", "supcon", "simmim", "densecl", "mae", "msn"), default="sham",
                    help="sham: the HSimCLR step (SHAMTrainStep).  supcon: the reference's simclr_supcon step "
                         "(SupConTrainStep) on the batch's class labels, with SHAM2(model) as encoder plus projection "
                         "head and SupConLoss(normalize=True); the reference's SupConResNet, a CIFAR-style trunk "
                         "(HairPretraining/src/backbone.py:276-358), is not built.  simmim: the reference's simMIM step "
                         "(SimMIMTrainStep) on SimMIM(vit_b_16), one view per image with lightly's MAETransform "
                         "settings (min_scale 0.2, flip, no colour jitter, grayscale or blur) on the device view "
                         "kernel, which resamples bilinearly where MAETransform resamples bicubically.  densecl: the "
                         "reference's DenseCL step (DenseCLTrainStep) on DenseCL(resnet50 trunk) - or the resnet18 "
                         "trunk with --model resnet18 - with the two device SimCLR views as x_query / x_key; lightly's "
                         "DenseCLTransform is not built.  mae: the reference's mae step (MAETrainStep) on "
                         "MAE(vit_base_patch16_224()), one view per image exactly as --mode simmim gives it (the device "
                         "view kernel stands in for lightly's MAETransform).  msn: the reference's MSN step (MSNTrainStep) on "
                         "MSN(vit_b_16()) with the two device SimCLR views as target ('anchor') and anchor ('pos1'); "
                         "lightly's MSNTransform is not built and the device view kernel produces 224 x 224 only, so no "
                         "focal views are passed (the step itself accepts them)")
    ap.add_argument("--epoch", type=int, default=0, help="--mode densecl: the epoch of the momentum schedule")
    ap.add_argument("--epochs", type=int, default=100,
                    help="--mode densecl: momentum = cosine_schedule(epoch, epochs, 0.996, 1)")
    ap.add_argument("--max-steps", type=int, default=0)
    ap.add_argument("--hip-train", action="store_true",
                    help="ResNet models: body convolutions forward and backward on the HIP kernels (hcir.conv_train)")
    ap.add_argument("--hip-train-norm", action="store_true",
                    help="ResNet models: the body's BatchNorm2d + residual + ReLU on the HIP kernels as well "
                         "(implies --hip-train)")
    ap.add_argument("--hip-train-stem", action="store_true",
                    help="ResNet models: the stem (conv 7x7, BatchNorm2d, ReLU, max pool) on the HIP kernels as well "
                         "(implies --hip-train)")
    ap.add_argument("--fused-optim", action="store_true",
                    help="the reference's optimizer (get_optimizer: Adam, weight decay on all but biases and norm "
                         "layers) and loss scaler on the HIP kernels: unscale, clip, step and scale update without a "
                         "host read (hcir.optim)")
    ap.add_argument("--weight-decay", type=float, default=1e-4, help="with --fused-optim (reference default)")
    ap.add_argument("--beta1", type=float, default=0.9, help="with --fused-optim (reference default)")
    ap.add_argument("--beta2", type=float, default=0.999, help="with --fused-optim (reference default)")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    from hcir.dataloader import EncodedDataset, collate_train_views
    from hcir.main_backbone import SHAM2
    from hcir.pretrain_engine import (DenseCLTrainStep, MAETrainStep, MSNTrainStep, SHAMTrainStep, SimMIMTrainStep,
                                      SupConTrainStep, cosine_schedule)
    torch.manual_seed(a.seed)
    ds = EncodedDataset(a.csv, a.img_dir, return_names=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=a.batch_size, shuffle=False, drop_last=True,
                                         num_workers=a.workers, collate_fn=functools.partial(collate_train_views),
                                         pin_memory=False)
    if a.mode == "simmim":
        if a.model != "vit_b_16":
            ap.error("--mode simmim trains the torchvision vit_b_16")
        if a.fused_optim:
            ap.error("--mode simmim steps with torch's Adam and GradScaler (SimMIMTrainStep: scaler.step / update)")
        from hcir._tv_vit import vit_b_16
        from hcir.backbone import SimMIM
        model = SimMIM(vit_b_16()).cuda()
    elif a.mode == "mae":
        if a.model not in ("vit_b_16", "vit_base_patch16_224"):
            ap.error("--mode mae trains the timm vit_base_patch16_224 (HairPretraining/mainpretrain.py)")
        if a.fused_optim:
            ap.error("--mode mae steps with torch's Adam and GradScaler (MAETrainStep: scaler.step / update)")
        from hcir.backbone import MAE, vit_base_patch16_224
        model = MAE(vit_base_patch16_224()).cuda()
    elif a.mode == "msn":
        if a.model != "vit_b_16":
            ap.error("--mode msn trains the torchvision vit_b_16")
        if a.fused_optim:
            ap.error("--mode msn steps with torch's Adam and GradScaler (MSNTrainStep: scaler.step / update)")
        from hcir._tv_vit import vit_b_16
        from hcir.backbone import MSN
        model = MSN(vit_b_16()).cuda()
    elif a.mode == "densecl":
        if a.model == "vit_b_16":
            a.model = "resnet50"                  # the reference's DenseCL trunk (HP/mainpretrain.py:159-162)
        if a.model not in ("resnet18", "resnet50"):
            ap.error("--mode densecl trains a resnet18 or resnet50 trunk")
        if a.fused_optim:
            ap.error("--mode densecl steps with hcir.optim.Adam's plain step() under torch's GradScaler "
                     "(DenseCLTrainStep: scaler.step / update); the fused tail is SHAMTrainStep's")
        from torch import nn
        from hcir import _tv_resnet
        from hcir.backbone import DenseCL
        trunk = nn.Sequential(*list(getattr(_tv_resnet, a.model)(weights=None).children())[:-2])
        model = DenseCL(trunk, feature_dim=512 if a.model == "resnet18" else 2048).cuda()
        model.hip_train = a.hip_train or a.hip_train_norm or a.hip_train_stem
        model.hip_train_norm = a.hip_train_norm
        model.hip_train_stem = a.hip_train_stem
    else:
        model = SHAM2(a.model).cuda()
        model.hip_train = a.hip_train or a.hip_train_norm or a.hip_train_stem
        model.hip_train_norm = a.hip_train_norm
        model.hip_train_stem = a.hip_train_stem
    if a.fused_optim:
        from hcir import optim
        opt, scaler = optim.get_optimizer(model, a.lr, a.weight_decay, a.beta1, a.beta2), optim.GradScaler()
    elif a.mode == "densecl":
        # the reference's get_optimizer over the trainable parameters: hcir.optim.Adam, whose plain
        # step() torch's GradScaler calls after its own unscale_; the frozen momentum twins are skipped
        from hcir import optim
        opt = optim.get_optimizer(model, a.lr, a.weight_decay, a.beta1, a.beta2)
        scaler = torch.amp.GradScaler("cuda")
    else:
        opt, scaler = torch.optim.Adam(model.parameters(), lr=a.lr), torch.amp.GradScaler("cuda")
    view_kwargs = view_names = step_kwargs = None
    if a.mode == "simmim":
        step = SimMIMTrainStep(model, opt, scaler)
        view_kwargs = dict(min_scale=0.2, cj_prob=0.0, random_gray_scale=0.0, gaussian_blur=0.0)
    elif a.mode == "mae":
        step = MAETrainStep(model, opt, scaler)
        view_kwargs = dict(min_scale=0.2, cj_prob=0.0, random_gray_scale=0.0, gaussian_blur=0.0)
    elif a.mode == "msn":
        step = MSNTrainStep(model, opt, scaler)
    elif a.mode == "densecl":
        step = DenseCLTrainStep(model, opt, scaler)
        view_names = {"anchor": "x_query", "pos1": "x_key"}
        step_kwargs = dict(momentum=cosine_schedule(a.epoch, a.epochs, 0.996, 1))
    elif a.mode == "supcon":
        from hcir.losses import SupConLoss
        step = SupConTrainStep(model, opt, scaler, SupConLoss(normalize=True))
    else:
        step = SHAMTrainStep(model, opt, scaler, warm_up_epochs=a.warm_up_epochs)

    class Stop(Exception):
        pass

    def report(i, out):
        print(f"step {i}: " + " ".join(f"{k}={v:.4f}" for k, v in out.items() if isinstance(v, float)), flush=True)
        if a.max_steps and i + 1 >= a.max_steps:
            raise Stop

    try:
        train_epoch(step, loader, "cuda", torch.Generator().manual_seed(a.seed), on_step=report,
                    with_labels=a.mode == "supcon", view_kwargs=view_kwargs, view_names=view_names,
                    step_kwargs=step_kwargs)
    except Stop:
        pass


if __name__ == "__main__":
    main()
