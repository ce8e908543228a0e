#!/usr/bin/env python
"""Input side of the pretrain step, measured: compressed files -> {"anchor", "pos1"} on the device.

    python tools/bench_train_input.py [--files 1024] [--distinct 64] [--size 1024] [--reps 5] [--step]

Writes `--distinct` hair-like size x size PNG files into a temporary directory (a batch of `--files` reads them in
turn), then reports, per batch of `--files` files (2 x files views):
  - host staging (16 threads), and with HIP events on one stream: H2D, decode, resample (crop + bilinear resize), view
    kernel; the view kernel's bytes/s against its algorithmic 150 528 B in + 602 112 B out per view;
  - wall clock of the whole producer (collate_train_views + views), pinned blobs, warm;
  - the same composition in Pillow on 16 host threads over the same files;
  - peak device memory the producer adds;
  - with --step: the time of one SHAMTrainStep on a batch of --files images (config C3's step), alone and with the
    producer of the next batch on a side stream, in this process.
One JSON line at the end.  Medians over --reps after one warm-up.
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
VIEW_BYTES = 224 * 224 * 3 + 224 * 224 * 3 * 4
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def hair_like(rng, size):
    small = rng.integers(0, 256, (size // 16, size // 16, 3)).astype(np.uint8)
    a = np.asarray(Image.fromarray(small).resize((size, size), Image.BICUBIC)).copy()
    a = np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:size, 0:size]
    a[((yy - size * 0.45) / (size * 0.4)) ** 2 + ((xx - size * 0.5) / (size * 0.33)) ** 2 > 1.0] = 0
    return a


def pillow_views(data, boxes, params):
    """The reference's work for one file: decode, then two views (torchvision's PIL ops, lightly's blur)."""
    with Image.open(io.BytesIO(data)) as im:
        im = im.convert("RGB")
    out = []
    for (top, left, h, w), p in zip(boxes, params):
        v = im.crop((left, top, left + w, top + h)).resize((224, 224), Image.BILINEAR)
        if p["flip"]:
            v = v.transpose(Image.FLIP_LEFT_RIGHT)
        if p["jitter"]:
            for op in p["order"]:
                if op == 0:
                    v = ImageEnhance.Brightness(v).enhance(float(p["brightness"]))
                elif op == 1:
                    v = ImageEnhance.Contrast(v).enhance(float(p["contrast"]))
                elif op == 2:
                    v = ImageEnhance.Color(v).enhance(float(p["saturation"]))
                else:
                    h_, s_, v_ = v.convert("HSV").split()
                    nh = (np.array(h_, dtype=np.int32) + (int(float(p["hue"]) * 255) & 255)).astype(np.uint8)
                    v = Image.merge("HSV", (Image.fromarray(nh, "L"), s_, v_)).convert("RGB")
        if p["gray"]:
            l = np.array(v.convert("L"))
            v = Image.fromarray(np.dstack([l, l, l]))
        if p["blur"]:
            v = v.filter(ImageFilter.GaussianBlur(radius=float(p["sigma"])))
        a = np.asarray(v, dtype=np.uint8).astype(np.float32) / np.float32(255)
        out.append(np.ascontiguousarray(((a - MEAN) / STD).transpose(2, 0, 1)))
    return out


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    return r, (e0, e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--skip-pillow", action="store_true")
    a = ap.parse_args()
    import hcir
    from hcir import _lib, png, resize, views
    from hcir.dataloader import collate_train_views
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    tmp = tempfile.mkdtemp(prefix="hcir_train_input_")
    distinct = []
    for k in range(a.distinct):
        b = io.BytesIO()
        Image.fromarray(hair_like(rng, a.size)).save(b, "PNG")
        with open(os.path.join(tmp, f"{k}_hair.png"), "wb") as f:
            f.write(b.getvalue())
        distinct.append(np.fromfile(os.path.join(tmp, f"{k}_hair.png"), dtype=np.uint8))
    files = [distinct[k % a.distinct] for k in range(a.files)]
    items = [(torch.from_numpy(f), 0, f"{k % a.distinct}_hair.png") for k, f in enumerate(files)]
    gen = torch.Generator().manual_seed(0)
    boxes = views.random_resized_crop_boxes([(a.size, a.size)] * (2 * a.files), gen)
    params = views.draw_view_params(2 * a.files, gen)
    stream = torch.cuda.current_stream(dev)
    res = {"build_id": _lib.build_id(), "files": a.files, "distinct_files": a.distinct, "size": a.size,
           "views": 2 * a.files, "file_bytes_mean": int(np.mean([f.size for f in distinct]))}

    # ---- phases, HIP events on one stream ----
    phases = {k: [] for k in ("stage_host_ms", "h2d_ms", "decode_ms", "resample_ms", "view_kernel_ms")}
    for rep in range(a.reps + 1):
        t_stage, ev = 0.0, {k: [] for k in ("h2d_ms", "decode_ms")}
        images = []
        for s in range(0, a.files, a.chunk):
            t0 = time.perf_counter()
            staged = png.stage_batch(files[s:s + a.chunk], pin=True, threads=16)
            t_stage += time.perf_counter() - t0
            on_dev, e = timed(stream, lambda: staged.to(dev))
            ev["h2d_ms"].append(e)
            whole, e = timed(stream, lambda: png.decode_windows(on_dev, (a.size, a.size), check_status=False))
            ev["decode_ms"].append(e)
            images += list(whole.unbind(0))
        index = list(range(a.files)) * 2
        crops, e_rs = timed(stream, lambda: torch.cat([
            resize.resize_boxes(images, boxes[s:s + views.RESIZE_CHUNK], 224, "bilinear", index[s:s + views.RESIZE_CHUNK])
            for s in range(0, 2 * a.files, views.RESIZE_CHUNK)]))
        out, e_v = timed(stream, lambda: views.apply_view_params(crops, params))
        torch.cuda.synchronize()
        if rep:
            phases["stage_host_ms"].append(t_stage * 1e3)
            for k in ev:
                phases[k].append(sum(x.elapsed_time(y) for x, y in ev[k]))
            phases["resample_ms"].append(e_rs[0].elapsed_time(e_rs[1]))
            phases["view_kernel_ms"].append(e_v[0].elapsed_time(e_v[1]))
        del images, crops, out, whole, on_dev
    for k, v in phases.items():
        res[k] = round(statistics.median(v), 3)
    res["view_kernel_GBps"] = round(2 * a.files * VIEW_BYTES / (res["view_kernel_ms"] * 1e-3) / 1e9, 1)
    res["device_phases_ms"] = round(sum(res[k] for k in ("h2d_ms", "decode_ms", "resample_ms", "view_kernel_ms")), 3)

    # ---- the whole producer, wall clock, and the memory it adds ----
    torch.cuda.empty_cache()
    resize._ws.clear(), png._ws.clear()
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    walls = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        batch = collate_train_views(items, chunk=a.chunk, threads=16, pin=True)
        t1 = time.perf_counter()
        out = batch.views(dev, boxes=boxes, params=params)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            walls.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3))
        if rep < a.reps:
            del out
    res["producer_wall_ms"] = round(statistics.median(w[0] for w in walls), 2)
    res["producer_collate_ms"] = round(statistics.median(w[1] for w in walls), 2)
    res["views_per_s"] = round(2 * a.files / (res["producer_wall_ms"] * 1e-3))
    res["producer_peak_GiB"] = round((torch.cuda.max_memory_allocated() - base_mem) / 2**30, 2)

    # ---- Pillow, 16 host threads, same files / boxes / parameters ----
    if not a.skip_pillow:
        bx = boxes.reshape(2, a.files, 4)
        pr = params.reshape(2, a.files)
        with ThreadPoolExecutor(16) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda k: pillow_views(files[k].tobytes(), (bx[0][k], bx[1][k]), (pr[0][k], pr[1][k])),
                          range(a.files)))
            res["pillow_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 1)

    # ---- the step it feeds ----
    if a.step:
        from hcir.main_backbone import SHAM2
        from hcir.pretrain_engine import SHAMTrainStep
        torch.manual_seed(0)
        model = SHAM2("vit_b_16").cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-5)
        step = SHAMTrainStep(model, opt, torch.amp.GradScaler("cuda", init_scale=256.0), warm_up_epochs=2)
        side = torch.cuda.Stream(device=dev)

        def run(with_producer):
            ts = []
            for rep in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if with_producer:
                    b2 = collate_train_views(items, chunk=a.chunk, threads=16, pin=True)
                    with torch.cuda.stream(side):
                        nxt, check = b2.views(dev, boxes=boxes, params=params, defer_check=True)
                step(out, epoch=0, batch_id=0)
                if with_producer:
                    check()
                torch.cuda.synchronize()
                if rep:
                    ts.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(ts), 1)

        res["step_alone_ms"] = run(False)
        res["step_with_producer_beside_ms"] = run(True)
        res["peak_with_step_GiB"] = round(torch.cuda.max_memory_allocated() / 2**30, 1)
    for f in os.listdir(tmp):
        os.unlink(os.path.join(tmp, f))
    os.rmdir(tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
