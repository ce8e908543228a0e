#!/usr/bin/env python
"""Micro-benchmark of the MSN pieces on the HIP path, fp16, next to a plain-torch restatement under fp16 autocast in
the same process:

  * the MSN criterion (hcir_msn_targets / _fwd / _bwd through hcir.losses.MSNLoss), forward (anchors without a
    gradient) and forward + backward (the prototypes' clone and the host read of grad_out included), at
    (B, V, K, D) = (256, 11, 1024, 256) - one anchor view plus MSNTransform's ten focal views at batch 256 - and
    (256, 1, 1024, 256) - the shape tools/train_from_files.py --mode msn gives;
  * one whole MSNTrainStep on MSN(vit_b_16()) at batch 256, with and without ten 96 x 96 focal views, against the same
    step composed in plain torch on the same parameters: lightly's update_momentum loop, the torchvision blocks on the
    kept tokens under autocast, the heads, lightly's loss formula, GradScaler and Adam.

Method: the candidates alternate, round after round, in one process; each round times a window of `--iters` calls with
device events after a warm-up of every candidate; the figure is the median over `--rounds` rounds, with the min .. max
spread next to it.  Boxes of this kind differ by +-3 %: a ratio inside 0.97 .. 1.03 is no difference.

    python tools/bench_msn.py > profiles/msn_bench.txt
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hcir.losses import MSNLoss  # noqa: E402


def torch_msn_loss(anchors, targets, prototypes, t=0.1, ts=0.25, iterations=3, weight=1.0):
    """lightly's MSNLoss.forward as plain torch ops (under the caller's autocast): three [rows, K] softmax matrices,
    the pow, the Sinkhorn loop."""
    num_views = anchors.shape[0] // targets.shape[0]
    anchors, targets = F.normalize(anchors, dim=1), F.normalize(targets, dim=1)
    prototypes = F.normalize(prototypes, dim=1)
    anchor_probs = F.softmax(torch.matmul(anchors, prototypes.t()) / t, dim=1)
    with torch.no_grad():
        q = F.softmax(torch.matmul(targets, prototypes.t()) / t, dim=1) ** (1.0 / ts)
        q = q / q.sum(dim=1, keepdim=True)
        if iterations > 0:
            b, k = q.shape
            qq = q.t() / q.sum()
            for _ in range(iterations):
                qq = qq / qq.sum(dim=1, keepdim=True)
                qq = qq / k
                qq = qq / qq.sum(dim=0, keepdim=True)
                qq = qq / b
            q = (qq * b).t()
        q = q.repeat((num_views, 1))
    loss = torch.mean(torch.sum(torch.log(anchor_probs ** (-q)), dim=1))
    if weight > 0:
        pbar = torch.mean(anchor_probs, dim=0)
        loss = loss + weight * (-torch.sum(torch.log(pbar ** (-pbar))) + math.log(float(len(pbar))))
    return loss


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # microseconds per call


def alternate(cands, rounds, iters, warm=5):
    times = {k: [] for k in cands}
    for fn in cands.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(window(fn, iters))
    return times


def line(k, us, unit="us", div=1.0):
    return f"  {k:28s} {statistics.median(us) / div:10.1f} {unit} ({min(us) / div:.1f} .. {max(us) / div:.1f})"


def verdict(ratio):
    return "inside the +-3 % box" if 0.97 <= ratio <= 1.03 else ("hcir faster" if ratio > 1 else "hcir SLOWER")


def bench_loss(a):
    for b, v, k, d in ((256, 11, 1024, 256), (256, 1, 1024, 256)):
        g = torch.Generator(device="cuda").manual_seed(3)
        anchors = torch.randn(b * v, d, device="cuda", generator=g).half()
        targets = torch.randn(b, d, device="cuda", generator=g).half()
        protos = torch.randn(k, d, device="cuda", generator=g) * 0.05
        crit = MSNLoss()
        leaf = anchors.clone().requires_grad_(True)

        def torch_loss(x):
            with torch.autocast("cuda", dtype=torch.float16):
                return torch_msn_loss(x, targets, protos)

        def fb(loss_fn):
            def run():
                leaf.grad = None
                loss_fn().backward()
            return run

        cands = {
            "hcir msn loss fwd": lambda: crit(anchors, targets, protos),
            "torch autocast fwd": lambda: torch_loss(anchors),
            "hcir msn loss fwd+bwd": fb(lambda: crit(leaf, targets, protos)),
            "torch autocast fwd+bwd": fb(lambda: torch_loss(leaf)),
        }
        got, want = float(crit(anchors, targets, protos)), float(torch_msn_loss(anchors.double(), targets.double(),
                                                                                   protos.double()))
        times = alternate(cands, a.rounds, a.iters)
        print(f"msn loss B={b} V={v} K={k} D={d} T=0.1 Ts=0.25 sinkhorn 3: loss hcir {got:.5f}  torch float64 {want:.5f}")
        for name, us in times.items():
            print(line(name, us))
        m = {name: statistics.median(us) for name, us in times.items()}
        rf, rb = m["torch autocast fwd"] / m["hcir msn loss fwd"], m["torch autocast fwd+bwd"] / m["hcir msn loss fwd+bwd"]
        print(f"  torch / hcir: fwd {rf:.2f} ({verdict(rf)})  fwd+bwd {rb:.2f} ({verdict(rb)})")


# ---------------------------------------------------------------------------------------------------------------
# the whole step in plain torch on an hcir.backbone.MSN's own parameters
# ---------------------------------------------------------------------------------------------------------------
def _interpolated_pos(pos, npatch):
    n0 = pos.shape[1] - 1
    if npatch == n0:
        return pos
    g0, d = int(math.sqrt(n0)), pos.shape[-1]
    grid = F.interpolate(pos[:, 1:].reshape(1, g0, g0, d).permute(0, 3, 1, 2), scale_factor=math.sqrt(npatch / n0),
                         mode="bicubic")
    return torch.cat((pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, d)), dim=1)


def torch_masked_vit(vit, images, idx_keep):
    """lightly's MaskedVisionTransformerTorchvision.forward(images, idx_keep) on a torchvision-layout container."""
    x = vit.conv_proj(images).flatten(2).transpose(1, 2)
    x = torch.cat((vit.class_token.expand(x.shape[0], -1, -1), x), 1)
    x = x + _interpolated_pos(vit.encoder.pos_embedding, x.shape[1] - 1)
    if idx_keep is not None:
        x = torch.gather(x, 1, idx_keep.unsqueeze(-1).expand(-1, -1, x.shape[-1]))
    for blk in vit.encoder.layers:
        h = blk.ln_1(x)
        h, _ = blk.self_attention(h, h, h, need_weights=False)
        x = x + h
        x = x + blk.mlp(blk.ln_2(x))
    return vit.encoder.ln(x)[:, 0]


class TorchMSNStep:
    """The reference's train_one_epoch_msn body (HairPretraining/src/pretrain_engine.py:246-270) in plain torch."""

    def __init__(self, model, optimizer, scaler):
        self.model, self.optimizer, self.scaler = model, optimizer, scaler

    @staticmethod
    def _ema(src, dst, m):
        for p, e in zip(src.parameters(), dst.parameters()):      # lightly.models.utils.update_momentum
            e.data = e.data * m + p.data * (1.0 - m)

    def _masked(self, images):
        from hcir.backbone import random_token_mask
        m = self.model
        seq = (images.shape[-1] // m.anchor_backbone.vit.patch_size) ** 2
        keep, _ = random_token_mask((images.shape[0], seq), m.mask_ratio, device=images.device)
        return m.anchor_projection_head(torch_masked_vit(m.anchor_backbone.vit, images, keep))

    def __call__(self, views):
        m, opt, scaler = self.model, self.optimizer, self.scaler
        m.train()
        with torch.autocast("cuda", dtype=torch.float16):
            self._ema(m.anchor_backbone, m.backbone, 0.996)
            self._ema(m.anchor_projection_head, m.projection_head, 0.996)
            targets_out = m.projection_head(torch_masked_vit(m.backbone.vit, views[0], None))
            anchors_out = self._masked(views[1])
            if len(views) > 2:
                anchors_out = torch.cat([anchors_out, self._masked(torch.cat(views[2:], dim=0))], dim=0)
            loss = torch_msn_loss(anchors_out, targets_out, m.prototypes.data)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        return {"loss": float(loss.detach())}


def bench_step(a):
    from hcir._tv_vit import vit_b_16
    from hcir.backbone import MSN
    from hcir.pretrain_engine import MSNTrainStep
    b = a.step_batch
    g = torch.Generator(device="cuda").manual_seed(5)
    big = [torch.randn(b, 3, 224, 224, device="cuda", generator=g) for _ in range(2)]
    focal = [torch.randn(b, 3, 96, 96, device="cuda", generator=g) for _ in range(a.focal)]
    steps = {}
    for name, cls in (("hcir MSNTrainStep", MSNTrainStep), ("torch autocast step", TorchMSNStep)):
        torch.manual_seed(0)
        model = MSN(vit_b_16()).cuda()
        step = cls(model, torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4),
                   torch.amp.GradScaler("cuda"))
        steps[name] = step
    for label, views in ((f"with {a.focal} focal views 96 x 96", big + focal), ("without focal views", big)):
        cands = {name: (lambda s=step, v=views: s(v)) for name, step in steps.items()}
        times = alternate(cands, a.step_rounds, a.step_iters, warm=2)
        print(f"whole step, MSN(vit_b_16), batch {b}, 224 x 224, {label}, torch Adam + GradScaler (includes the "
              f"step's one host read)")
        for k, us in times.items():
            print(line(k, us, "ms", 1e3))
        mm = {k: statistics.median(v) for k, v in times.items()}
        r = mm["torch autocast step"] / mm["hcir MSNTrainStep"]
        print(f"  torch / hcir: {r:.3f} ({verdict(r)})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-batch", type=int, default=256)
    ap.add_argument("--focal", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    print(f"# fp16; per call: median of {a.rounds} alternated rounds of {a.iters} calls (min .. max); whole step: "
          f"{a.step_rounds} rounds of {a.step_iters}")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    bench_loss(a)
    if not a.skip_step:
        bench_step(a)


if __name__ == "__main__":
    main()
