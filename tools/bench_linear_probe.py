"""Linear-probe timings on one GPU (recorded in DESIGN.md "Linear probe", not gated).

For each (n, d, c): median ms of one loss-and-gradient evaluation (hcir_softmax_xent_fwd_bwd, HIP events, warm-up +
repetitions), that time as a fraction of 8 TB/s on the algorithmic 4 n d bytes and of 157 TF on 4 n d c FLOP, wall
time and iteration count of a whole LogisticRegression.fit on the device, and (unless --no-sklearn) the same fit in
scikit-learn on the host as the reference-path figure.  One JSON line per shape.

  python tools/bench_linear_probe.py [--reps 20] [--warmup 5] [--no-sklearn] [--shapes 103945x768x10,...]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))

SHAPES = "103945x768x10,103945x768x64,11269x2048x27"


def clustered(n, d, c, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((c, d)).astype(np.float32)
    y = rng.integers(0, c, n)
    x = centers[y] + np.float32(0.35 * np.sqrt(d)) * rng.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), y.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--shapes", default=SHAPES)
    a = ap.parse_args()
    import hcir
    from hcir import linear_probe as lp
    for shape in a.shapes.split(","):
        n, d, c = (int(v) for v in shape.split("x"))
        x, y = clustered(n, d, c, 0)
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        w = (0.5 * torch.randn(c, d, device="cuda")).contiguous()
        b = torch.zeros(c, device="cuda")
        buf = lp._Workspace(xd, c)
        for _ in range(a.warmup):
            lp._xent(xd, yd, w, b, buf)
        times = []
        for _ in range(max(a.reps, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lp._xent(xd, yd, w, b, buf)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf = lp.LogisticRegression(max_iter=5000).fit(xd, yd)
        torch.cuda.synchronize()
        fit_s = time.perf_counter() - t0
        res = {"n": n, "d": d, "c": c, "eval_ms_median": round(ms, 4), "eval_ms_min": round(min(times), 4),
               "frac_of_8TBps": round(4.0 * n * d / (ms * 1e-3) / 8e12, 4),
               "frac_of_157TF": round(4.0 * n * d * c / (ms * 1e-3) / 157e12, 4),
               "fit_s": round(fit_s, 3), "fit_n_iter": clf.n_iter_, "build_id": hcir._lib.build_id()}
        if not a.no_sklearn:
            from sklearn.linear_model import LogisticRegression
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sk = LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial").fit(x, y)
            res["sklearn_fit_s"] = round(time.perf_counter() - t0, 3)
            res["sklearn_n_iter"] = int(sk.n_iter_[0])
            res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
