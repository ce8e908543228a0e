#!/usr/bin/env python
"""Measurements of the MAE path at ViT-B/16, 224 x 224, batch 256 (197 tokens, 49 kept and 148 masked per image; decoder
dim 512, 16 heads of 32, 8 blocks):

  * attention at head_dim 32 and (b h, t) = (256 * 16, 197): hcir_attn_fwd_lse and hcir_attn_bwd next to torch's
    scaled_dot_product_attention in fp16 at the same shape, forward and forward + backward (torch's backward alone is
    the difference of the two);
  * the kernels of csrc/mae.hip: time per call and bytes per second, the bytes counted from the shapes (what the kernel
    has to read and write once, not what the memory system moved);
  * one full MAETrainStep (forward walk, loss, backward walk, torch Adam with a torch GradScaler) next to a plain-torch
    restatement of the same model and step under fp16 autocast (F.scaled_dot_product_attention, nn.MSELoss), on a copy
    of the same weights and the same index pair, alternated step by step in this process.

Method: candidates alternate, round after round, in one process; each round times a window of `--iters` calls with
device events after a warm-up; the figure is the median over `--rounds` rounds with the min .. max spread next to it.
Nothing here is a threshold: the figures say what was measured, a launch that loses to torch included.

    python tools/bench_mae.py > profiles/mae_bench.txt
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
from hcir.backbone import MAE, random_token_mask, vit_base_patch16_224  # noqa: E402
from hcir.pretrain_engine import MAETrainStep  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # microseconds per call


def stat(xs, unit="us"):
    return f"{statistics.median(xs):9.1f} {unit} ({min(xs):.1f} .. {max(xs):.1f})"


def alternate(cands, rounds, iters, warm=3):
    for fn in cands.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(window(fn, iters))
    return times


# ---------------------------------------------------------------------------------------------------------------
# the model and the step in plain torch, on the hcir model's parameter names
# ---------------------------------------------------------------------------------------------------------------
def _block(p, pre, x, heads):
    b, t, d = x.shape
    y = F.layer_norm(x, (d,), p[pre + "norm1.weight"], p[pre + "norm1.bias"], 1e-6)
    qkv = F.linear(y, p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"]).reshape(b, t, 3, heads, d // heads)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    att = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, t, d)
    x = x + F.linear(att, p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"])
    y = F.layer_norm(x, (d,), p[pre + "norm2.weight"], p[pre + "norm2.bias"], 1e-6)
    y = F.linear(F.gelu(F.linear(y, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"])), p[pre + "mlp.fc2.weight"],
                 p[pre + "mlp.fc2.bias"])
    return x + y


def _at(x, idx):
    return torch.gather(x, 1, idx.unsqueeze(-1).expand(-1, -1, x.shape[-1]))


def torch_mae_loss(p, images, idx_keep, idx_mask, ps, depth, ddepth):
    """MAE.forward + nn.MSELoss of the reference (HairPretraining/src/backbone.py:505-521) in plain torch."""
    e, dc = "backbone.vit.", "decoder."
    x = F.conv2d(images, p[e + "patch_embed.proj.weight"], p[e + "patch_embed.proj.bias"], stride=ps)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((p[e + "cls_token"].expand(x.shape[0], -1, -1), x), 1) + p[e + "pos_embed"]
    x = _at(x, idx_keep)
    for i in range(depth):
        x = _block(p, f"{e}blocks.{i}.", x, 12)
    x = F.layer_norm(x, (x.shape[-1],), p[e + "norm.weight"], p[e + "norm.bias"], 1e-6)
    x = F.linear(x, p[dc + "decoder_embed.weight"], p[dc + "decoder_embed.bias"])
    seq = p[dc + "decoder_pos_embed"].shape[1]
    full = p[dc + "mask_token"].repeat(x.shape[0], seq, 1).to(x.dtype)
    full = torch.scatter(full, 1, idx_keep.unsqueeze(-1).expand(-1, -1, x.shape[-1]), x)
    x = full + p[dc + "decoder_pos_embed"]
    for i in range(ddepth):
        x = _block(p, f"{dc}decoder_blocks.{i}.", x, 16)
    x = F.layer_norm(x, (x.shape[-1],), p[dc + "decoder_norm.weight"], p[dc + "decoder_norm.bias"], 1e-6)
    pred = F.linear(_at(x, idx_mask), p[dc + "decoder_pred.weight"], p[dc + "decoder_pred.bias"])
    n, c, h, w = images.shape
    patches = torch.einsum("nchpwq->nhwpqc", images.reshape(n, c, h // ps, ps, w // ps, ps))
    target = _at(patches.reshape(n, (h // ps) * (w // ps), ps * ps * c), idx_mask - 1)
    return F.mse_loss(pred.float(), target)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mae.py measures on a HIP device; none found")
    b, t, ps, size, de, dd, hd, heads = a.batch, 197, 16, 224, 768, 512, 32, 16
    p = 3 * ps * ps
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    print(f"# MAE, ViT-B/16, {size} x {size}, batch {b}: {t} tokens; median of {a.rounds} alternated rounds of {a.iters} "
          f"calls (min .. max); device: {torch.cuda.get_device_name(0)}")

    # ---- attention at head_dim 32 -----------------------------------------------------------------------------
    m = b * t
    qkv = (0.5 * torch.randn(m, 3 * heads * hd, device=dev, generator=g)).half()
    out, lse = torch.empty(m, heads * hd, dtype=torch.float16, device=dev), torch.empty(b, heads, t, device=dev)
    dout = (0.1 * torch.randn(m, heads * hd, device=dev, generator=g)).half()
    dqkv = torch.empty_like(qkv)
    scale = hd ** -0.5
    q, k, v = (x.contiguous().requires_grad_(True)
               for x in qkv.view(b, t, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0))       # [b, h, t, hd] each
    do4 = dout.view(b, t, heads, hd).transpose(1, 2).contiguous()

    def sdpa_fb():
        q.grad = k.grad = v.grad = None
        F.scaled_dot_product_attention(q, k, v).backward(do4)

    def sdpa_f():
        with torch.no_grad():
            F.scaled_dot_product_attention(q, k, v)
    ops.attn_fwd_lse(qkv, b, t, heads, scale, out, lse)
    times = alternate({"hcir_attn_fwd_lse hd32": lambda: ops.attn_fwd_lse(qkv, b, t, heads, scale, out, lse),
                       "hcir_attn_bwd hd32": lambda: ops.attn_bwd(qkv, out, dout, lse, b, t, heads, scale, dqkv),
                       "torch SDPA fp16 fwd": sdpa_f, "torch SDPA fp16 fwd+bwd": sdpa_fb}, a.rounds, a.iters)
    flop_f = 4.0 * b * heads * t * t * hd
    print(f"# attention, head_dim {hd}, (b h, t) = ({b} * {heads}, {t}); {flop_f / 1e9:.1f} GFLOP forward, 2.5 x that "
          "backward (5 products)")
    for kk, xs in times.items():
        print(f"  {kk:26s} {stat(xs)}")
    med = {kk: statistics.median(xs) for kk, xs in times.items()}
    hf, hb = med["hcir_attn_fwd_lse hd32"], med["hcir_attn_bwd hd32"]
    tf, tfb = med["torch SDPA fp16 fwd"], med["torch SDPA fp16 fwd+bwd"]
    print(f"  forward: torch / hcir {tf / hf:.2f};  backward: torch (fwd+bwd - fwd) / hcir {(tfb - tf) / hb:.2f};  "
          f"forward + backward: torch / hcir {tfb / (hf + hb):.2f}   (a ratio below 1: the hcir launch loses)")
    ref = F.scaled_dot_product_attention(q, k, v).detach().transpose(1, 2).reshape(m, heads * hd)
    print(f"  max |out_hcir - out_torch| {float((out.float() - ref.float()).abs().max()):.2e}")
    del q, k, v, do4, ref

    # ---- the kernels of mae.hip -------------------------------------------------------------------------------
    images = torch.randn(b, 3, size, size, device=dev, generator=g)
    idx_keep, idx_mask = (x.contiguous() for x in random_token_mask((b, t), 0.75, device=dev, generator=g))
    kk_, n = idx_keep.shape[1], idx_mask.shape[1]
    rk, rn, pad = b * kk_, b * n, lambda r: (r + 63) // 64 * 64
    tok = torch.randn(m, de, device=dev, generator=g).half()
    comp_k = torch.empty(pad(rk), de, dtype=torch.float16, device=dev)
    dcomp = torch.randn(pad(rk), de, device=dev, generator=g)
    dtok = torch.empty(m, de, device=dev)
    emb = torch.randn(pad(rk), dd, device=dev, generator=g).half()
    mt, pos = torch.randn(dd, device=dev, generator=g), torch.randn(t, dd, device=dev, generator=g)
    xd = torch.empty(m, dd, dtype=torch.float16, device=dev)
    dres = torch.randn(m, dd, device=dev, generator=g)
    demb, gmt = torch.empty(pad(rk), dd, dtype=torch.float16, device=dev), torch.empty(dd, device=dev)
    xc = torch.empty(pad(rn), dd, dtype=torch.float16, device=dev)
    pred = torch.randn(pad(rn), p, device=dev, generator=g).half()
    cands = {
        "hcir_mae_gather_rows (kept, d 768)": (lambda: ops.mae_gather_rows(tok, b, t, idx_keep, comp_k),
                                               2 * pad(rk) * de * 2 + rk * 8),
        "hcir_mae_scatter_rows (kept, d 768)": (lambda: ops.mae_scatter_rows(dcomp, b, t, idx_keep, dtok),
                                                rk * de * 4 + m * de * 4 + rk * 8),
        "hcir_mae_decoder_input": (lambda: ops.mae_decoder_input(emb, b, t, idx_keep, mt, pos, xd),
                                   rk * dd * 2 + m * dd * 2 + t * dd * 4 + rk * 8),
        "hcir_mae_gather_rows (masked, d 512)": (lambda: ops.mae_gather_rows(xd, b, t, idx_mask, xc),
                                                 2 * pad(rn) * dd * 2 + rn * 8),
        "hcir_mae_decoder_input_bwd": (lambda: ops.mae_decoder_input_bwd(dres, b, t, idx_keep, demb, gmt),
                                       m * dd * 4 + rk * dd * 2 + rk * 8),
        "hcir_mae_mse_fwd": (lambda: ops.mae_mse_fwd(pred, images, idx_mask, ps), rn * p * (2 + 4 + 2) + rn * 8),
    }
    times = alternate({k_: fn for k_, (fn, _) in cands.items()}, a.rounds, a.iters)
    print("# csrc/mae.hip; a call's time includes its launch (back-to-back calls of one kernel); the working sets fit "
          "the 256 MB Infinity Cache in part or whole, so the rates are not HBM rates")
    for k_, (_, nbytes) in cands.items():
        print(f"  {k_:38s} {stat(times[k_])}   {nbytes / 1e6:8.1f} MB -> "
              f"{nbytes / statistics.median(times[k_]) / 1e6:6.2f} TB/s")
    del tok, comp_k, dcomp, dtok, emb, xd, dres, demb, xc, pred, qkv, out, dout, dqkv

    # ---- the whole step -----------------------------------------------------------------------------------------
    torch.manual_seed(0)
    model = MAE(vit_base_patch16_224()).cuda()
    trainable = {k_ for k_, v_ in model.named_parameters() if v_.requires_grad}
    params = {k_: v_.detach().clone().requires_grad_(k_ in trainable) for k_, v_ in model.state_dict().items()}
    step = MAETrainStep(model, torch.optim.Adam(model.parameters(), lr=1e-4), torch.amp.GradScaler("cuda"))
    topt = torch.optim.Adam([v_ for v_ in params.values() if v_.requires_grad], lr=1e-4)
    tscaler = torch.amp.GradScaler("cuda")
    keep_mask = {}

    def hcir_step():
        keep_mask["loss_hcir"] = step(images)["loss"]

    def torch_step():
        ik, im = random_token_mask((b, t), 0.75, device=dev)
        with torch.autocast("cuda", dtype=torch.float16):
            loss = torch_mae_loss(params, images, ik, im, ps, 12, 8)
        tscaler.scale(loss).backward()
        tscaler.step(topt)
        tscaler.update()
        topt.zero_grad()
        keep_mask["loss_torch"] = float(loss.detach())
    ms = {k_: [x / 1e3 for x in xs] for k_, xs in
          alternate({"MAETrainStep (hcir)": hcir_step, "plain-torch step, fp16 autocast": torch_step}, a.step_rounds, 1,
                    warm=2).items()}
    print("# one optimisation step, torch Adam + GradScaler and one host read of the loss in both; ms per step")
    for k_, xs in ms.items():
        print(f"  {k_:34s} {stat(xs, 'ms')}   {b / statistics.median(xs) * 1e3:.0f} images/s")
    h_, t_ = statistics.median(ms["MAETrainStep (hcir)"]), statistics.median(ms["plain-torch step, fp16 autocast"])
    print(f"  torch / hcir {t_ / h_:.2f}   (last losses: hcir {keep_mask['loss_hcir']:.4f}, torch "
          f"{keep_mask['loss_torch']:.4f}; different random masks, both after {a.step_rounds + 2} steps)")


if __name__ == "__main__":
    main()
