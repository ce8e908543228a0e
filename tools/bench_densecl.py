#!/usr/bin/env python
"""Micro-benchmark of the DenseCL pieces on the HIP path, fp16, next to a plain-torch restatement under fp16 autocast
in the same process:

  * NT-Xent against a memory bank (hcir_ntxent_bank_fwd / _bwd through hcir.losses.NTXentLoss(memory_bank_size=...)),
    forward (inputs without a gradient: nothing is enqueued) and forward + backward (queue update, bank clone and the
    host read of grad_out included), at the step's two shapes (N, K, D) = (256, 4096, 512) -
    the global rows at batch 256 - and (12544, 4096, 512) - the local rows, 256 x 49;
  * dense matching (hcir_dense_match_f16 through hcir.dense.select_most_similar) at (B, N, M, C, Dv) =
    (256, 49, 49, 2048, 512);
  * one whole DenseCLTrainStep, ResNet-50 trunk at batch 256 and 224 x 224, with hip_train + hip_train_norm +
    hip_train_stem on and off (off: torch / MIOpen trunk; losses and matching are the HIP kernels either way).

Method: the candidates alternate, round after round, in one process; each round times a window of `--iters` calls with
device events after a warm-up of every shape; the figure is the median over `--rounds` rounds, with the min .. max
spread next to it.

    python tools/bench_densecl.py > profiles/densecl_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from hcir.dense import select_most_similar  # noqa: E402
from hcir.losses import NTXentLoss  # noqa: E402


def torch_bank_loss(out0, out1, bank, t):
    """lightly's NTXentLoss.forward with a bank, as plain torch ops under fp16 autocast: the [N, K + 1] logits are
    materialised."""
    with torch.autocast("cuda", dtype=torch.float16):
        q, k = F.normalize(out0, dim=1), F.normalize(out1, dim=1)
        negatives = bank.clone().detach()
        logits = torch.cat([(q * k).sum(1, keepdim=True), q @ negatives.to(q.dtype).t()], 1) / t
        return F.cross_entropy(logits, torch.zeros(q.shape[0], dtype=torch.long, device=q.device))


def torch_select_most_similar(x, y, y_values):
    """lightly.models.utils.select_most_similar as plain torch ops under fp16 autocast."""
    with torch.autocast("cuda", dtype=torch.float16):
        sim = torch.einsum("bnc,bmc->bnm", F.normalize(x, dim=-1), F.normalize(y, dim=-1))
        idx = sim.argmax(dim=2)
        return torch.gather(y_values, 1, idx.unsqueeze(-1).expand(-1, -1, y_values.shape[2]))


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


def bench_loss(a):
    t = 0.5
    for n, kb, d in ((256, 4096, 512), (12544, 4096, 512)):
        g = torch.Generator(device="cuda").manual_seed(3)
        z0 = torch.randn(n, d, device="cuda", generator=g).half()
        z1 = (z0.float() + 0.5 * torch.randn(n, d, device="cuda", generator=g)).half()
        crit = NTXentLoss(t, memory_bank_size=(kb, d)).cuda()
        bank = crit.bank.clone()
        leaf = z0.clone().requires_grad_(True)

        def fb(loss_fn):
            def run():
                leaf.grad = None
                loss_fn().backward()
            return run

        cands = {
            "hcir bank loss fwd": lambda: crit(z0, z1),
            "torch autocast fwd": lambda: torch_bank_loss(z0, z1, bank, t),
            "hcir bank loss fwd+bwd": fb(lambda: crit(leaf, z1)),
            "torch autocast fwd+bwd": fb(lambda: torch_bank_loss(leaf, z1, bank, t)),
        }
        crit.bank.copy_(bank)
        got, want = float(crit(z0, z1)), float(torch_bank_loss(z0.float(), z1.float(), bank, t))
        times = alternate(cands, a.rounds, a.iters)
        print(f"bank loss N={n} K={kb} D={d} T={t}: loss hcir {got:.5f}  torch {want:.5f}")
        for k, us in times.items():
            print(line(k, us))
        m = {k: statistics.median(v) for k, v in times.items()}
        print(f"  torch / hcir: fwd {m['torch autocast fwd'] / m['hcir bank loss fwd']:.2f}  "
              f"fwd+bwd {m['torch autocast fwd+bwd'] / m['hcir bank loss fwd+bwd']:.2f}")


def bench_match(a):
    b, n, m, c, dv = 256, 49, 49, 2048, 512
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(b, n, c, device="cuda", generator=g).relu().half()
    y = torch.randn(b, m, c, device="cuda", generator=g).relu().half()
    v = torch.randn(b, m, dv, device="cuda", generator=g).half()
    cands = {"hcir select_most_similar": lambda: select_most_similar(x, y, v),
             "torch autocast": lambda: torch_select_most_similar(x, y, v)}
    same = float((select_most_similar(x, y, v) == torch_select_most_similar(x, y, v)).all(dim=2).float().mean())
    times = alternate(cands, a.rounds, a.iters)
    print(f"dense match B={b} N={n} M={m} C={c} Dv={dv}: rows equal to torch's {100 * same:.2f} %")
    for k, us in times.items():
        print(line(k, us))
    mm = {k: statistics.median(v) for k, v in times.items()}
    print(f"  torch / hcir: {mm['torch autocast'] / mm['hcir select_most_similar']:.2f};  hcir reads "
          f"{(x.numel() + y.numel()) * 2 / 1e6:.0f} MB: {(x.numel() + y.numel()) * 2 / mm['hcir select_most_similar'] / 1e3:.0f} GB/s")


def bench_step(a):
    from hcir import _tv_resnet
    from hcir.backbone import DenseCL
    from hcir.pretrain_engine import DenseCLTrainStep
    b = a.step_batch
    g = torch.Generator(device="cuda").manual_seed(5)
    xq = torch.randn(b, 3, 224, 224, device="cuda", generator=g)
    batch = {"x_query": xq, "x_key": xq + 0.3 * torch.randn(b, 3, 224, 224, device="cuda", generator=g)}
    steps = {}
    for name, on in (("switches on", True), ("switches off", False)):
        torch.manual_seed(0)
        model = DenseCL(nn.Sequential(*list(_tv_resnet.resnet50(weights=None).children())[:-2])).cuda()
        model.hip_train = model.hip_train_norm = model.hip_train_stem = on
        params = [p for p in model.parameters() if p.requires_grad]
        step = DenseCLTrainStep(model, torch.optim.Adam(params, lr=1e-4), torch.amp.GradScaler("cuda"))
        steps[name] = (lambda s=step: s(batch, momentum=0.996))
    times = alternate(steps, a.step_rounds, a.step_iters, warm=2)
    print(f"whole step, ResNet-50 trunk, batch {b}, 224 x 224, bank (4096, 512), torch Adam + GradScaler "
          f"(includes the step's one host read)")
    for k, us in times.items():
        print(line(k, us, "ms", 1e3))
    mm = {k: statistics.median(v) for k, v in times.items()}
    print(f"  off / on: {mm['switches off'] / mm['switches on']:.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-batch", type=int, default=256)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    print(f"# fp16; per call: median of {a.rounds} alternated rounds of {a.iters} calls (min .. max); whole step: "
          f"{a.step_rounds} rounds of {a.step_iters}")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    bench_loss(a)
    bench_match(a)
    if not a.skip_step:
        bench_step(a)


if __name__ == "__main__":
    main()
