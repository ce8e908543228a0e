"""ResNet-18 / ResNet-50 trunk TRAINING timings on one GPU: forward + backward of the trunk at 224 x 224 (recorded in
DESIGN.md §3.4, not gated; bench.py is the contract).

Six paths, same process, same machine, same input; median over --steps iterations after --warmup (HIP events around
forward + backward of loss = features.sum(); gradients are dropped between iterations, no optimizer):
  torch_fp32                 the torch trunk as SHAMTrainStep runs it today (fp32 NCHW, MIOpen)
  torch_autocast             torch.autocast(fp16), the reference's way (HP/src/pretrain_engine.py:681)
  torch_autocast_chlast      the same on a channels_last trunk and input: the fair vendor yardstick
  hip_train                  the model's `hip_train` switch: hcir.conv_train (body convolutions on the HIP kernels)
  hip_train_norm             `hip_train` and `hip_train_norm`: the body's BatchNorm2d + residual + ReLU on HIP as well
  hip_train_stem             all three switches: the stem (conv 7x7, BatchNorm2d, ReLU, max pool) on HIP as well
then ONE more iteration of each of the last three with every libhcir call bracketed by HIP events, which splits its
device time into forward convolutions, data gradients by plan (stride 1; 1x1 stride 2; the 3x3 stride 2 that does 4x
the useful flops - each with its spread-by-2 copy), weight gradients, BatchNorm forward / backward (HIP; the second
and third path), stem forward / stem backward (HIP; the third path only) and the rest (torch: casts, pool and, where
the switches leave them to it, the stem, BatchNorm, ReLU, adds).  Events, not a
profiler's kernel trace: forward and data gradient run the SAME kernel and only the call site tells them apart.
One JSON line per (model, batch).  --bn2d-bandwidth adds one line: the BatchNorm2d entry points alone at ResNet-50's
layer1 shape (M = 256 * 56 * 56, C = 256), in bytes the algorithm must move per second.  --stem-bandwidth adds the
same for the stem entry points at (256, 224, 224).

  python tools/bench_resnet_train.py [--model resnet50,resnet18] [--batch 64,256] [--steps 10] [--warmup 3]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))


def median_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def fwd_bwd(features, params):
    def run():
        for p in params:
            p.grad = None
        features().float().sum().backward()
    return run


def kernel_shares(model, x):
    """Device time of one hip_train forward + backward by kind of libhcir work (HIP events around every forward
    convolution, every data gradient - its spread-by-2 copy included - every weight gradient and, with
    `hip_train_norm` on, every BatchNorm forward and backward)."""
    from hcir import conv_train, ops
    spans = []
    inside = {"dgrad": False}

    def bracket(label, fn, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **k)
        e1.record()
        spans.append((label, e0, e1))
        return out

    real_conv, real_wgrad, real_dgrad = ops.conv2d_f16, ops.conv2d_wgrad, conv_train.conv2d_dgrad
    real_bn_fwd, real_bn_bwd = ops.bn2d_fwd, ops.bn2d_bwd
    stem_names = ("stem_conv", "bn2d_stats", "stem_bn_relu_pool", "stem_pool_relu_bwd", "stem_wgrad")
    real_stem = {n: getattr(ops, n) for n in stem_names}

    def conv(*a, **k):
        return real_conv(*a, **k) if inside["dgrad"] else bracket("forward", real_conv, *a, **k)

    def dgrad(dy, wt16, h, w, stride, pad):
        label = "dgrad_stride1" if stride == 1 else ("dgrad_1x1_stride2" if wt16.shape[1] == 1 else "dgrad_3x3_stride2")
        inside["dgrad"] = True
        try:
            return bracket(label, real_dgrad, dy, wt16, h, w, stride, pad)
        finally:
            inside["dgrad"] = False

    ops.conv2d_f16, conv_train.conv2d_dgrad = conv, dgrad
    ops.conv2d_wgrad = lambda *a, **k: bracket("wgrad", real_wgrad, *a, **k)
    ops.bn2d_fwd = lambda *a, **k: bracket("bn_forward_hip", real_bn_fwd, *a, **k)

    def bn_bwd(*a, **k):    # the BatchNorm backward that follows the stem's pool backward is the stem's
        label = "stem_backward_hip" if inside.pop("stem_bwd", False) else "bn_backward_hip"
        return bracket(label, real_bn_bwd, *a, **k)

    def pool_bwd(*a, **k):
        inside["stem_bwd"] = True
        return bracket("stem_backward_hip", real_stem["stem_pool_relu_bwd"], *a, **k)

    ops.bn2d_bwd, ops.stem_pool_relu_bwd = bn_bwd, pool_bwd
    for n in ("stem_conv", "bn2d_stats", "stem_bn_relu_pool"):
        setattr(ops, n, lambda *a, _f=real_stem[n], **k: bracket("stem_forward_hip", _f, *a, **k))
    ops.stem_wgrad = lambda *a, **k: bracket("stem_backward_hip", real_stem["stem_wgrad"], *a, **k)
    try:
        for p in model.backbone.parameters():
            p.grad = None
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        model.extract_features(x).float().sum().backward()
        t1.record()
        torch.cuda.synchronize()
    finally:
        ops.conv2d_f16, ops.conv2d_wgrad, conv_train.conv2d_dgrad = real_conv, real_wgrad, real_dgrad
        ops.bn2d_fwd, ops.bn2d_bwd = real_bn_fwd, real_bn_bwd
        for n in stem_names:
            setattr(ops, n, real_stem[n])
    total = t0.elapsed_time(t1)
    by = {}
    for label, e0, e1 in spans:
        by[label] = by.get(label, 0.0) + e0.elapsed_time(e1)
    by["torch_rest"] = total - sum(by.values())
    return {"total_ms": round(total, 3), "ms": {k: round(v, 3) for k, v in sorted(by.items())},
            "share": {k: round(v / total, 4) for k, v in sorted(by.items())}}


def bn2d_bandwidth(dev, warmup, steps, b=256, hw=56, c=256):
    """ops.bn2d_fwd / ops.bn2d_bwd alone (residual + ReLU, the block-closing form): median ms and the bytes the
    algorithm must move (forward: x twice, resid, y; backward: dy, x, y twice each, dx, dresid) per second."""
    from hcir import ops
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (b, hw, hw, c)
    x, r, dy = (torch.randn(shape, device=dev, dtype=torch.float16, generator=g) for _ in range(3))
    gamma = torch.rand(c, device=dev, generator=g) + 0.5
    beta = torch.randn(c, device=dev, generator=g) * 0.2
    y, mean, rstd = ops.bn2d_fwd(x, gamma, beta, 1e-5, 0.1, r, True)
    nbytes = x.numel() * 2
    f_ms = median_ms(lambda: ops.bn2d_fwd(x, gamma, beta, 1e-5, 0.1, r, True), warmup, steps)
    b_ms = median_ms(lambda: ops.bn2d_bwd(dy, x, y, gamma, mean, rstd, want_dresid=True), warmup, steps)
    return {"bn2d_bandwidth": {"shape": list(shape), "chunks": ops.bn2d_chunks(b * hw * hw, c),
                               "fwd_ms": round(f_ms, 4), "fwd_TBps": round(4 * nbytes / f_ms / 1e9, 3),
                               "bwd_ms": round(b_ms, 4), "bwd_TBps": round(8 * nbytes / b_ms / 1e9, 3),
                               "counted_bytes": {"fwd": 4 * nbytes, "bwd": 8 * nbytes}}}


def stem_bandwidth(dev, warmup, steps, b=256, hw=224):
    """The stem entry points alone at (b, hw, hw): median ms and the bytes the algorithm must move per second, with
    N = the fp16 conv-level map and I = the fp32 image: conv I + N; pool N + N / 4; pool backward N / 4 + 2 N; weight
    gradient I + N (its partials, 37 KB a part, are not counted)."""
    from hcir import ops
    from hcir.resnet_engine import pack_stem_weight
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(b, 3, hw, hw, device=dev, generator=g)
    wp = pack_stem_weight(torch.randn(64, 3, 7, 7, device=dev, generator=g) / 12.0)
    gamma = torch.rand(64, device=dev, generator=g) + 0.5
    beta = torch.randn(64, device=dev, generator=g) * 0.2
    c = ops.stem_conv(x, wp)
    mean, rstd = ops.bn2d_stats(c, 1e-5, 0.1)
    p = ops.stem_bn_relu_pool(c, gamma, beta, mean, rstd)
    dp = torch.randn(p.shape, device=dev, dtype=torch.float16, generator=g)
    gy = ops.stem_pool_relu_bwd(dp, c, gamma, beta, mean, rstd)
    n_b, i_b = c.numel() * 2, x.numel() * 4
    runs = {"conv": (lambda: ops.stem_conv(x, wp, out=c), i_b + n_b),
            "stats": (lambda: ops.bn2d_stats(c, 1e-5, 0.1), n_b),
            "bn_relu_pool": (lambda: ops.stem_bn_relu_pool(c, gamma, beta, mean, rstd, out=p), n_b + n_b // 4),
            "pool_relu_bwd": (lambda: ops.stem_pool_relu_bwd(dp, c, gamma, beta, mean, rstd, out=gy),
                              n_b // 4 + 2 * n_b),
            "bn_bwd": (lambda: ops.bn2d_bwd(gy, c, None, gamma, mean, rstd), 5 * n_b),
            "wgrad": (lambda: ops.stem_wgrad(x, gy), i_b + n_b)}
    out = {"shape": [b, hw, hw], "wgrad_parts": ops.stem_wgrad_parts(b, hw, hw), "peak_TBps": 6.3}
    for k, (fn, nbytes) in runs.items():
        ms = median_ms(fn, warmup, steps)
        out[k] = {"ms": round(ms, 4), "TBps": round(nbytes / ms / 1e9, 3), "of_peak": round(nbytes / ms / 1e9 / 6.3, 3),
                  "counted_bytes": nbytes}
    return {"stem_bandwidth": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50,resnet18")
    ap.add_argument("--batch", default="64,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bn2d-bandwidth", action="store_true")
    ap.add_argument("--stem-bandwidth", action="store_true")
    args = ap.parse_args()

    from hcir.main_backbone import SHAM2

    dev = torch.device("cuda", 0)
    for name in args.model.split(","):
        torch.manual_seed(0)
        model = SHAM2(name).train().to(dev)
        trunk = model.backbone
        trunk_cl = copy.deepcopy(trunk).to(memory_format=torch.channels_last)
        for b in (int(v) for v in args.batch.split(",")):
            x = torch.randn(b, 3, 224, 224, device=dev)
            x_cl = x.contiguous(memory_format=torch.channels_last)

            def autocast(t, inp):
                def f():
                    with torch.autocast("cuda", dtype=torch.float16):
                        return t(inp).flatten(1)
                return f

            model.hip_train = False
            ms = {"torch_fp32": median_ms(fwd_bwd(lambda: trunk(x).flatten(1), list(trunk.parameters())),
                                          args.warmup, args.steps),
                  "torch_autocast": median_ms(fwd_bwd(autocast(trunk, x), list(trunk.parameters())),
                                              args.warmup, args.steps),
                  "torch_autocast_chlast": median_ms(fwd_bwd(autocast(trunk_cl, x_cl), list(trunk_cl.parameters())),
                                                     args.warmup, args.steps)}
            model.hip_train = True
            ms["hip_train"] = median_ms(fwd_bwd(lambda: model.extract_features(x), list(trunk.parameters())),
                                        args.warmup, args.steps)
            shares = kernel_shares(model, x)
            model.hip_train_norm = True
            ms["hip_train_norm"] = median_ms(fwd_bwd(lambda: model.extract_features(x), list(trunk.parameters())),
                                             args.warmup, args.steps)
            shares_norm = kernel_shares(model, x)
            model.hip_train_stem = True
            ms["hip_train_stem"] = median_ms(fwd_bwd(lambda: model.extract_features(x), list(trunk.parameters())),
                                             args.warmup, args.steps)
            shares_stem = kernel_shares(model, x)
            model.hip_train_norm = model.hip_train_stem = False
            out = {"model": name, "batch": b, "steps": args.steps,
                   "ms": {k: round(v, 3) for k, v in ms.items()},
                   "img_per_s": {k: round(b / v * 1e3, 1) for k, v in ms.items()},
                   "fastest": min(ms, key=ms.get),
                   "hip_train_vs": {k: round(ms["hip_train"] / v, 3) for k, v in ms.items()
                                    if k not in ("hip_train", "hip_train_norm", "hip_train_stem")},
                   "hip_train_norm_vs": {k: round(ms["hip_train_norm"] / v, 3) for k, v in ms.items()
                                         if k not in ("hip_train_norm", "hip_train_stem")},
                   "hip_train_stem_vs": {k: round(ms["hip_train_stem"] / v, 3) for k, v in ms.items()
                                         if k != "hip_train_stem"},
                   "hip_train_breakdown": shares, "hip_train_norm_breakdown": shares_norm,
                   "hip_train_stem_breakdown": shares_stem}
            print(json.dumps(out), flush=True)
    if args.bn2d_bandwidth:
        print(json.dumps(bn2d_bandwidth(dev, args.warmup, args.steps)), flush=True)
    if args.stem_bandwidth:
        print(json.dumps(stem_bandwidth(dev, args.warmup, args.steps)), flush=True)


if __name__ == "__main__":
    main()
