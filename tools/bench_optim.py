"""The optimizer tail alone, on the parameter sets of SHAM2("vit_b_16"), SHAM2("resnet50") and SHAM2("resnet18") with
synthetic finite gradients: torch's lines

    scaler.unscale_(opt); clip_grad_norm_(params, 1.0); scaler.step(opt); scaler.update()

(torch.optim.Adam built by the reference's get_optimizer rule, torch.amp.GradScaler) against
hcir.optim.Adam.step_scaled(hcir.optim.GradScaler), alternated in one process, HIP-event time per call, median of
`--iters` after `--warmup`, in two regimes: with the device idle when the tail is called (the time then contains the
host's time to enqueue) and with the tail queued behind device work that is still running, as it is behind backward()
in a training step.  Prints both times, the fused tail's achieved bytes/s against its algorithmic traffic
(4 B/param for the norm pass, 16 B read + 12 B written for the Adam pass) and the table rebuilds during the timed calls.

    python tools/bench_optim.py [--iters 25] [--warmup 5] [--models vit_b_16 resnet50 resnet18]
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch  # noqa: E402


def torch_pair(model, lr, wd):
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (no_decay if (n.endswith(".bias") or "bn" in n or "norm" in n) else decay).append(p)
    opt = torch.optim.Adam([{"params": decay, "weight_decay": wd}, {"params": no_decay, "weight_decay": 0.0}], lr)
    return opt, torch.amp.GradScaler("cuda", init_scale=1024.0)


def bench(name, iters, warmup):
    from hcir import optim
    from hcir.main_backbone import SHAM2
    torch.manual_seed(0)
    model_t = SHAM2(name).cuda()
    model_f = copy.deepcopy(model_t)
    gen = torch.Generator(device="cuda").manual_seed(1)
    params_t = [p for p in model_t.parameters() if p.requires_grad]
    params_f = [p for p in model_f.parameters() if p.requires_grad]
    grads0 = [1024.0 * 1e-2 * torch.randn(p.shape, device="cuda", generator=gen) for p in params_t]
    for pt, pf, g in zip(params_t, params_f, grads0):
        pt.grad, pf.grad = g.clone(), g.clone()
    opt_t, scaler_t = torch_pair(model_t, 1e-4, 1e-4)
    opt_f, scaler_f = optim.get_optimizer(model_f, 1e-4, 1e-4, 0.9, 0.999), optim.GradScaler(init_scale=1024.0)
    scaler_t.scale(torch.ones((), device="cuda"))          # initialises torch's scaler state

    def tail_torch():
        scaler_t.unscale_(opt_t)
        torch.nn.utils.clip_grad_norm_(params_t, max_norm=1.0)
        scaler_t.step(opt_t)
        scaler_t.update()

    def tail_fused():
        opt_f.step_scaled(scaler_f, max_norm=1.0)

    tails = {"torch": (tail_torch, params_t), "fused": (tail_fused, params_f)}
    # two regimes: the device idle when the tail is called (its time then includes the host's time to enqueue), and
    # the tail queued behind device work that is still running, as it is behind backward() in a training step
    blocker = torch.randn(8192, 8192, device="cuda", generator=gen)
    dev = {(k, q): [] for k in tails for q in (False, True)}
    host = {k: [] for k in tails}
    rebuilds0 = None
    for i in range(warmup + iters):
        if i == warmup:
            rebuilds0 = opt_f.table_rebuilds
        for queued in (False, True):
            for k, (fn, params) in tails.items():
                torch._foreach_copy_([p.grad for p in params], grads0)     # torch's tail unscales in place: refill
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                if queued:
                    torch.mm(blocker, blocker)
                a.record()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                b.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    dev[k, queued].append(a.elapsed_time(b))
                    if not queued:
                        host[k].append((t1 - t0) * 1e3)
    n = sum(p.numel() for p in params_f)
    traffic = n * (4 + 16 + 12)
    assert scaler_f.get_scale() == scaler_t.get_scale()
    print(f"{name}: {n / 1e6:.1f} M parameters in {len(params_f)} tensors, {iters} timed calls per row, alternated; "
          f"fused tail: {traffic / 1e6:.1f} MB algorithmic traffic")
    for queued in (False, True):
        print("  queued behind running device work (HIP events after the blocker):" if queued else
              "  device idle at the call (HIP events around the call):")
        med = {}
        for k in tails:
            v = dev[k, queued]
            med[k] = statistics.median(v)
            print(f"    {k} tail: median {med[k] * 1e3:8.1f} us  (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})"
                  + ("" if queued else f"; host time of the call: median {statistics.median(host[k]) * 1e3:.1f} us"))
        print(f"    fused / torch = {med['fused'] / med['torch']:.3f}  ({med['torch'] / med['fused']:.2f}x); fused tail "
              f"{traffic / (med['fused'] * 1e-3) / 1e12:.2f} TB/s of its algorithmic traffic")
    print(f"  table rebuilds during the timed calls: {opt_f.table_rebuilds - rebuilds0}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=["vit_b_16", "resnet50", "resnet18"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a HIP device")
    for name in a.models:
        bench(name, a.iters, a.warmup)


if __name__ == "__main__":
    main()
