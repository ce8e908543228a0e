#!/usr/bin/env python
"""Measurements of the SimMIM path at ViT-B/16, 224 x 224, batch 256 (197 tokens, 148 masked per image):

  * the four kernels of csrc/mim.hip: time per call and bytes per second, the bytes counted from the shapes (what
    the kernel has to read and write once, not what the memory system moved);
  * hcir_mim_l1_fwd (loss and sign matrix: everything the backward needs) next to a plain-torch restatement under fp16
    autocast - patchify, gather, F.l1_loss - forward and forward + backward to the prediction's gradient;
  * one full SimMIMTrainStep (forward walk, loss, backward walk, torch Adam with a torch GradScaler).

Method: candidates alternate, round after round, in one process; each round times a window of `--iters` calls with
device events after a warm-up; the figure is the median over `--rounds` rounds with the min .. max spread next to it.
This is a capability, not a speed-up: the kernels are memory-bound passes far below a millisecond in a step of
hundreds of milliseconds, and nothing here is compared with a torch training step.

    python tools/bench_simmim.py > profiles/simmim_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hcir import train_ops as ops  # noqa: E402
from hcir._tv_vit import vit_b_16  # noqa: E402
from hcir.backbone import SimMIM, random_token_mask  # noqa: E402
from hcir.pretrain_engine import SimMIMTrainStep  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # microseconds per call


def torch_l1(pred, images, idx, ps):
    """The reference's target and loss as plain torch ops under fp16 autocast (lightly's patchify + get_at_index)."""
    with torch.autocast("cuda", dtype=torch.float16):
        n, c, h, w = images.shape
        patches = torch.einsum("nchpwq->nhwpqc", images.reshape(n, c, h // ps, ps, w // ps, ps))
        patches = patches.reshape(n, (h // ps) * (w // ps), ps * ps * c)
        target = torch.gather(patches, 1, (idx - 1).unsqueeze(-1).expand(-1, -1, patches.shape[-1]))
        return F.l1_loss(pred, target)


def stat(xs):
    return f"{statistics.median(xs):9.1f} us ({min(xs):.1f} .. {max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-rounds", type=int, default=7)
    a = ap.parse_args()
    b, t, d, ps, size = a.batch, 197, 768, 16, 224
    p = 3 * ps * ps
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    images = torch.randn(b, 3, size, size, device=dev, generator=g)
    idx = random_token_mask((b, t), 0.75, device=dev, generator=g)[1].contiguous()
    n = idx.shape[1]
    rows, m, npat = b * n, b * t, b * (t - 1)
    mask = torch.zeros((b, t), dtype=torch.uint8, device=dev).scatter_(1, idx, 1)
    tok = torch.randn(m, d, device=dev, generator=g).half()
    mt, pos = torch.randn(d, device=dev, generator=g), torch.randn(t, d, device=dev, generator=g)
    dtok = torch.randn(m, d, device=dev, generator=g)
    gmt, dpatch = torch.empty(d, device=dev), torch.empty((npat, d), dtype=torch.float16, device=dev)
    pred = torch.randn(rows, p, device=dev, generator=g).half()
    leaf = pred.view(b, n, p).clone().requires_grad_(True)
    print(f"# ViT-B/16, {size} x {size}, batch {b}: {t} tokens, {n} masked per image, P = {p}; microseconds per call: "
          f"median of {a.rounds} alternated rounds of {a.iters} calls (min .. max)")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print("# a call's time includes its launch (back-to-back calls of one kernel); the working sets of 59 - 233 MB fit "
          "the 256 MB Infinity Cache in part or whole, so the rates are not HBM rates")

    def fb():
        leaf.grad = None
        torch_l1(leaf, images, idx, ps).backward()

    cands = {
        # bytes from the shapes: rows written / read once
        "hcir_mim_mask_tokens": (lambda: ops.mim_mask_tokens(tok, b, t, mask, mt, pos, 1.0),
                                 rows * d * 2 + t * d * 4 + m),
        "hcir_mim_mask_bwd": (lambda: ops.mim_mask_bwd(dtok, b, t, mask, gmt, dpatch), npat * d * 4 + npat * d * 2 + m),
        "hcir_mim_patch_targets": (lambda: ops.mim_patch_targets(images, idx, ps), rows * p * 8 + rows * 8),
        "hcir_mim_l1_fwd": (lambda: ops.mim_l1_fwd(pred, images, idx, ps), rows * p * (2 + 4 + 2) + rows * 8),
        "torch l1 fwd": (lambda: torch_l1(pred.view(b, n, p), images, idx, ps), None),
        "torch l1 fwd+bwd": (fb, None),
    }
    for fn, _ in cands.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, (fn, _) in cands.items():
            times[k].append(window(fn, a.iters))
    for k, (_, nbytes) in cands.items():
        rate = "" if nbytes is None else f"   {nbytes / 1e6:8.1f} MB -> {nbytes / statistics.median(times[k]) / 1e6:6.2f} TB/s"
        print(f"  {k:24s} {stat(times[k])}{rate}")
    got = float(ops.mim_l1_fwd(pred, images, idx, ps)[0])
    want = float(torch_l1(pred.view(b, n, p).float(), images, idx, ps))
    l1 = statistics.median(times["hcir_mim_l1_fwd"])
    print(f"  loss hcir {got:.6f}  torch {want:.6f};   torch fwd / hcir l1_fwd {statistics.median(times['torch l1 fwd']) / l1:.2f}, "
          f"torch fwd+bwd / hcir l1_fwd {statistics.median(times['torch l1 fwd+bwd']) / l1:.2f} "
          f"(hcir_mim_l1_fwd leaves the sign matrix: its backward is a scalar multiply)")

    del tok, dtok, dpatch, pred, leaf
    model = SimMIM(vit_b_16()).cuda()
    step = SimMIMTrainStep(model, torch.optim.Adam(model.parameters(), lr=1e-4), torch.amp.GradScaler("cuda"))
    for _ in range(2):
        step(images)
    torch.cuda.synchronize()
    ms = [window(lambda: step(images), 1) / 1e3 for _ in range(a.step_rounds)]
    print(f"  SimMIMTrainStep (torch Adam + GradScaler, one host read of the loss per step): "
          f"{statistics.median(ms):.1f} ms ({min(ms):.1f} .. {max(ms):.1f}), "
          f"{b / statistics.median(ms) * 1e3:.0f} images/s")


if __name__ == "__main__":
    main()
