#!/usr/bin/env python
"""Micro-benchmark of hcir SupConLoss (hcir_supcon_fwd / _bwd), fp16, forward and forward + backward, next to

  * a plain-torch restatement of the reference's SupConLoss on the same GPU under fp16 autocast (the path a user of
    the labelled mode had before: materialised [2B, 2B] logits, three masks, a vendor GEMM), and
  * hcir NT-Xent at the same B, D: the yardstick - the same MFMA work without the label epilogue.

Method: the three candidates alternate, round after round, in one process; each round times a window of `--iters`
calls with device events after a warm-up of every shape; the figure is the median over `--rounds` rounds, with the
min .. max spread next to it.

    python tools/bench_supcon.py > profiles/supcon_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hcir.losses import NTXentLoss, SupConLoss  # noqa: E402


def torch_supcon(features, labels, t, t_base):
    """The reference loss (contrast_mode 'all', labels) restated as plain torch ops, under fp16 autocast."""
    with torch.autocast("cuda", dtype=torch.float16):
        b, v = features.shape[:2]
        x = F.normalize(torch.cat(torch.unbind(features, 1), 0), dim=1)
        logits = (x @ x.t()) / t
        logits = logits - logits.max(1, keepdim=True).values.detach()
        same = (labels[:, None] == labels[None, :]).float().repeat(v, v)
        off = 1.0 - torch.eye(b * v, device=features.device)
        same = same * off
        log_prob = logits - torch.log((torch.exp(logits) * off).sum(1, keepdim=True))
        cnt = same.sum(1)
        cnt = torch.where(cnt < 1e-6, torch.ones_like(cnt), cnt)
        return -(t / t_base) * ((same * log_prob).sum(1) / cnt).mean()


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # microseconds per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--classes", type=int, default=64)
    a = ap.parse_args()
    t, t_base, dt = 0.07, 0.07, torch.float16
    print(f"# fp16, V = 2, T = T_base = {t}, {a.classes} classes; microseconds per call: median of {a.rounds} "
          f"alternated rounds of {a.iters} calls (min .. max)")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    for b, d in ((1024, 128), (1024, 512), (256, 1024)):
        g = torch.Generator(device="cuda").manual_seed(3)
        feat = torch.randn(b, 2, d, device="cuda", generator=g).to(dt)
        labels = torch.randint(0, a.classes, (b,), device="cuda", generator=g)
        leaf = feat.clone().requires_grad_(True)
        l0, l1 = feat[:, 0].contiguous().requires_grad_(True), feat[:, 1].contiguous().requires_grad_(True)
        z0, z1 = l0.detach(), l1.detach()      # contiguous: no slice copy inside the yardstick's forward
        sup, nt = SupConLoss(t, "all", t_base, normalize=True), NTXentLoss(t)

        def fb(loss_fn, leaves):
            def run():
                for x in leaves:
                    x.grad = None
                loss_fn().backward()
            return run

        cands = {
            "hcir supcon": (lambda: sup(feat, labels), fb(lambda: sup(leaf, labels), [leaf])),
            "torch autocast": (lambda: torch_supcon(feat, labels, t, t_base),
                               fb(lambda: torch_supcon(leaf, labels, t, t_base), [leaf])),
            "hcir ntxent": (lambda: nt(z0, z1), fb(lambda: nt(l0, l1), [l0, l1])),
        }
        times = {k: ([], []) for k in cands}
        for fwd, fwdbwd in cands.values():     # warm every shape
            for _ in range(10):
                fwd()
                fwdbwd()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, (fwd, fwdbwd) in cands.items():
                times[k][0].append(window(fwd, a.iters))
                times[k][1].append(window(fwdbwd, a.iters))
        got, want = float(sup(feat, labels)), float(torch_supcon(feat.float(), labels, t, t_base))
        print(f"B={b} V=2 D={d}: loss hcir {got:.5f}  torch {want:.5f}")
        for k, (f_us, fb_us) in times.items():
            print(f"  {k:15s} fwd {statistics.median(f_us):8.1f} us ({min(f_us):.1f} .. {max(f_us):.1f})   "
                  f"fwd+bwd {statistics.median(fb_us):8.1f} us ({min(fb_us):.1f} .. {max(fb_us):.1f})")
        ms, mn = statistics.median(times["hcir supcon"][0]), statistics.median(times["hcir ntxent"][0])
        mt = statistics.median(times["torch autocast"][0])
        bs, bn = statistics.median(times["hcir supcon"][1]), statistics.median(times["hcir ntxent"][1])
        bt = statistics.median(times["torch autocast"][1])
        print(f"  supcon / ntxent: fwd {ms / mn:.3f}  fwd+bwd {bs / bn:.3f};   torch / supcon: fwd {mt / ms:.2f}  "
              f"fwd+bwd {bt / bs:.2f}")


if __name__ == "__main__":
    main()
