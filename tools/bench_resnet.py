"""ResNet-18 / ResNet-50 trunk timings on one GPU (recorded in DESIGN.md §3.4, not gated; bench.py is the contract).

For each (model, batch) at 224 x 224, in one process, median over --reps runs after --warmup (HIP events):
  hip               SHAM2.extract_features with hip_trunk on: hcir.resnet_engine (HIP convolution kernels, NHWC fp16)
                    as a user calls it, the per-call parameter fingerprint of ResNetEngineCache included
  hip_engine_only   ResNetEngine.forward alone (no fingerprint): what the kernels and their launches take
  torch_fp32        the torch trunk as the default path runs it (fp32 NCHW, MIOpen)
  torch_fp16        the torch trunk in fp16 channels_last: the fair vendor yardstick
  torch_fp16_tuned  the same with torch.backends.cudnn.benchmark = True (MIOpen searches its kernels per shape)
plus the engine's time per layer group (hcir.profiling.EventProfiler), img/s, and achieved TFLOP/s as a fraction of the
2.5 PFLOP/s dense fp16 figure at 8.2 (ResNet-50) / 3.6 (ResNet-18) GFLOP per image.  One JSON line per point.

  python tools/bench_resnet.py [--reps 20] [--warmup 5] [--models resnet50,resnet18] [--batches 64,256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))

GFLOP_PER_IMAGE = {"resnet50": 8.2, "resnet18": 3.6}
PEAK_TFLOPS = 2500.0


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="resnet50,resnet18")
    ap.add_argument("--batches", default="64,256")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20 (the recorded figure is a median of >= 20 runs)")

    import copy

    from hcir.main_backbone import SHAM2
    from hcir.profiling import EventProfiler
    from hcir.resnet_engine import GROUPS

    dev = torch.device("cuda", 0)
    for name in args.models.split(","):
        torch.manual_seed(0)
        model = SHAM2(name).eval().to(dev)
        model.hip_trunk = True
        trunk = model.backbone
        trunk16 = copy.deepcopy(trunk).half().to(memory_format=torch.channels_last)
        eng = model.trunk_engine("backbone", dev)   # the model's own engine
        for b in (int(v) for v in args.batches.split(",")):
            x = torch.randn(b, 3, 224, 224, device=dev)
            x16 = x.half().contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                ms = {
                    "hip": median_ms(lambda: model.extract_features(x), args.warmup, args.reps),
                    "hip_engine_only": median_ms(lambda: eng.forward(x), args.warmup, args.reps),
                    "torch_fp32": median_ms(lambda: trunk(x).flatten(1), args.warmup, args.reps),
                    "torch_fp16": median_ms(lambda: trunk16(x16).flatten(1), args.warmup, args.reps),
                }
                with torch.backends.cudnn.flags(enabled=True, benchmark=True):
                    ms["torch_fp16_tuned"] = median_ms(lambda: trunk16(x16).flatten(1), args.warmup, args.reps)
                # per layer group: median over the same number of profiled runs (events between the launches)
                per = {g: [] for g in GROUPS}
                for _ in range(args.reps):
                    prof = EventProfiler()
                    eng.profiler = prof
                    prof.start()
                    eng.forward(x)
                    for g, d in prof.summary().items():
                        per[g].append(d["ms"])
                eng.profiler = None
                cos = torch.nn.functional.cosine_similarity(eng.forward(x).double(), trunk(x).flatten(1).double(), dim=1)
            gf = GFLOP_PER_IMAGE[name]
            out = {"model": name, "batch": b, "reps": args.reps,
                   "ms": {k: round(v, 3) for k, v in ms.items()},
                   "img_per_s": {k: round(b / v * 1e3, 1) for k, v in ms.items()},
                   "tflops": {k: round(b * gf / v, 1) for k, v in ms.items()},
                   "frac_of_2.5PF": {k: round(b * gf / v / PEAK_TFLOPS, 4) for k, v in ms.items()},
                   "hip_group_ms": {g: round(statistics.median(v), 3) for g, v in per.items()},
                   "fastest": min((k for k in ms if k != "hip_engine_only"), key=ms.get),
                   "hip_vs_torch_fp32_one_minus_cos": float((1 - cos).abs().max())}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
