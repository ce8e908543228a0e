#!/usr/bin/env python3
"""Generates tests/golden/supcon_ref.npz (build container only; never runs on the GPU box).

    python tests/golden/make_supcon_golden.py <checkout of the reference project>

What executes here: the reference's own SupConLoss class, imported at run time from
HairPretraining/utils/losses.py of that checkout (torch only), in float64, with torch autograd for the gradients.
Only inputs, labels, losses and gradients are written; no reference source text is copied.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# (B, V, D, T, T_base, labels): V = 1, 2, 3; rows without positives (V = 1 singletons); labels None; T != T_base;
# classes that differ only above bit 31
CASES = [
    (8, 2, 16, 0.07, 0.07, "three"),
    (8, 2, 16, 0.5, 0.07, None),
    (12, 1, 8, 0.3, 0.07, "mixed"),
    (6, 3, 24, 0.07, 0.07, "three"),
    (16, 2, 40, 0.2, 0.1, "wide"),
    (20, 2, 8, 0.1, 0.07, "one"),
]


def load_ref_supcon(ref_root):
    path = os.path.join(ref_root, "HairPretraining/utils/losses.py")
    spec = importlib.util.spec_from_file_location("ref_supcon_losses", path)
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except ModuleNotFoundError:
        # the file goes on to import `lightly` for its other losses, which is not installed here; SupConLoss, the
        # first class of the file, is complete by then
        pass
    return mod.SupConLoss


def labels_of(kind, b, g):
    if kind is None:
        return None
    if kind == "three":
        return torch.randint(0, 3, (b,), generator=g)
    if kind == "one":
        return torch.full((b,), 4, dtype=torch.int64)
    if kind == "mixed":
        return torch.tensor([2 * (i // 3) + (1 if i % 3 == 2 else 0) for i in range(b)])[torch.randperm(b, generator=g)]
    return torch.tensor([5, 5 + 2 ** 32, -1])[torch.arange(b) % 3][torch.randperm(b, generator=g)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    SupConLoss = load_ref_supcon(sys.argv[1])
    out = {"n": np.int64(len(CASES))}
    for i, (b, v, d, t, tb, kind) in enumerate(CASES):
        g = torch.Generator().manual_seed(100 + i)
        f = torch.randn(b, v, d, generator=g, dtype=torch.float64)
        f = f / f.norm(dim=2, keepdim=True) * (1.0 if i % 2 == 0 else 1.5)   # bounded logits, norms 1 and 1.5
        labels = labels_of(kind, b, g)
        x = f.clone().requires_grad_(True)
        loss = SupConLoss(temperature=t, base_temperature=tb)(x, labels)
        loss.backward()
        out[f"features_{i}"] = f.numpy()
        out[f"labels_{i}"] = labels.numpy() if labels is not None else np.zeros(0, dtype=np.int64)
        out[f"has_labels_{i}"] = np.bool_(labels is not None)
        out[f"t_{i}"], out[f"t_base_{i}"] = np.float64(t), np.float64(tb)
        out[f"loss_{i}"], out[f"grad_{i}"] = loss.detach().numpy(), x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "supcon_ref.npz"), **out)


if __name__ == "__main__":
    main()
