"""One sha256 line per tensor of the ViT host walks (hcir.vit_train.VitTrainer, hcir.vit_engine.VitEngine), fixed seeds.
The kernels behind them use no atomics, so two trees whose walks issue the same launches print the same lines: run it
on both sides of a change to the host code and diff.   usage: vit_digest.py [small] [vitb] [infer]   (default: all)
  small   a hand-made spec (dim 256, 4 heads, mlp 512, depth 3, 64 x 64 images, batch 3: pad rows in both row sets),
          the four (keep_recomputable, cls_only_last) trainers: class token and every gradient
  vitb    ViT-B/16 at 224 x 224, the default trainer, at the smallest batch whose fc1 takes the dual-output GEMM
  infer   forward_cls under no_grad, fp32 and fp16 residual stream, batch 3 and the smallest LayerNorm-fold batch"""
import hashlib
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch
import hcir
from hcir import vit_engine
from hcir.main_backbone import SHAM2
from hcir.vit_train import VitTrainer

DEV = torch.device("cuda")


def line(case, name, t):
    torch.cuda.synchronize()
    h = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
    print(f"{case} {name} {tuple(t.shape)} {h}", flush=True)


def walk(case, trainer, x, wgt):
    cls, saved = trainer.forward(x)
    line(case, "cls", cls)
    for i, g in enumerate(trainer.backward(saved, wgt)):
        line(case, f"grad{i:03d}", g)


def small_spec():
    g = torch.Generator().manual_seed(5)
    r = lambda *s, scale=0.05, shift=0.0: shift + scale * torch.randn(*s, generator=g)
    gain = lambda n: r(n, scale=0.2, shift=1.0)
    d, mlp = 256, 512
    layers = [vit_engine.VitLayer(gain(d), r(d), r(3 * d, d), r(3 * d), r(d, d), r(d), gain(d), r(d), r(mlp, d), r(mlp),
                                  r(d, mlp), r(d)) for _ in range(3)]
    return vit_engine.VitSpec(16, d, 4, 1e-6, 2.0, r(d, 3, 16, 16), r(d), r(1, 1, d), r(1, 17, d), layers, gain(d),
                              r(d))


def fused_batch():
    """Smallest batch of 197-token images every GEMM shape of a ViT-B/16 block takes the persistent kernel at."""
    L = hcir.lib()
    shapes = ((3072, 768), (2304, 768), (768, 768), (768, 3072))
    return next(b for b in range(1, 64) if all(L.hcir_gemm_fused_supported(b * 197, n, k) for n, k in shapes))


def main():
    groups = sys.argv[1:] or ["small", "vitb", "infer"]
    gen = torch.Generator().manual_seed(6)
    if "small" in groups:
        spec = small_spec()
        x, wgt = torch.randn(3, 3, 64, 64, generator=gen).to(DEV), torch.randn(3, 256, generator=gen).to(DEV)
        for keep in (True, False):
            for cls_only in (True, False):
                walk(f"small/keep={int(keep)}/cls_only={int(cls_only)}",
                     VitTrainer(spec, DEV, keep_recomputable=keep, cls_only_last=cls_only), x, wgt)
    if "vitb" in groups or "infer" in groups:
        torch.manual_seed(7)
        model = SHAM2("vit_b_16").to(DEV)
        nb = fused_batch()
        x = torch.randn(nb, 3, 224, 224, generator=gen).to(DEV)
    if "vitb" in groups:
        walk(f"vitb/b={nb}", model.backbone.trainer(DEV), x, torch.randn(nb, 768, generator=gen).to(DEV))
    if "infer" in groups:
        for rd in (torch.float32, torch.float16):
            vit_engine.DEFAULT_RESID_DTYPE = rd                 # part of the engine cache's key: a new engine
            for b in (3, nb):
                with torch.no_grad():
                    line(f"infer/{str(rd).split('.')[1]}/b={b}", "emb", model.backbone.forward_cls(x[:b]))


if __name__ == "__main__":
    main()
