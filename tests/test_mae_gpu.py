"""hcir.backbone.MAE on an MI355X against the fp32 CPU restatement (tests/_mae_ref.py) and torch's autograd through it:
forward(images, idx_keep, idx_mask), the fused masked_loss and MAETrainStep.

Bars (those of tests/test_simmim_gpu.py): every x_pred row within cosine 1e-3 of the restatement; every gradient within
1e-2 in relative norm and cosine >= 0.9999, error norms taken against the gradient's own norm plus a floor of 1e-3 of
the largest per-element gradient RMS times sqrt(numel), and the cosine only asked of tensors whose reference norm is
above that floor.  The MSE is smooth, so the fused gradients are compared with autograd of the restatement's own
nn.MSELoss.  The loss must lie within the triangle inequality's slack, mean(|x_gpu - x_ref| (|x_gpu - t| + |x_ref - t|)),
plus the kernel's own bound of the loss (tests/_mae_ref.mse_k).

The small model is the walk test's shape (encoder dim 256, 4 heads, mlp 512, depth 2; decoder dim 512, 16 heads of 32,
depth 2; 64 x 64, patch 16, batch 3: 4 kept and 13 masked tokens per image); one case runs the whole
MAE(vit_base_patch16_224()) at batch 2 (197 tokens, 49 kept, 148 masked, the 8-block decoder).

Measured on an MI355X (profiles/mae_errors.txt): x_pred rows within 3.6e-7 cosine; worst relative gradient error 1.45e-3
(small) and 1.25e-3 (ViT-B/16); loss differences 5.2e-7 and 1.7e-5 inside slacks of 1.2e-3 and 1.6e-3."""
import os
import sys
from functools import partial

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mae_ref as aref

pytestmark = pytest.mark.gpu
_CACHE = {}


def _unused(name):
    """Parameters the reference's forward never reads (timm's classification head, lightly's encoder-side mask token)
    or never trains (decoder_pos_embed, requires_grad=False)."""
    return ".vit.head." in name or name == "backbone.mask_token" or name.endswith("decoder_pos_embed")


def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if _unused(n):
                continue
            if n.endswith(("norm1.weight", "norm2.weight", "norm.weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        model.backbone.vit.cls_token.copy_(0.02 * torch.randn(model.backbone.vit.cls_token.shape, generator=g))


def _setup(kind):
    """(model on the CPU, its reference state dict, heads, images, idx_keep, idx_mask), built once."""
    if kind in _CACHE:
        return _CACHE[kind]
    from hcir.backbone import MAE, _TimmViT, vit_base_patch16_224
    torch.manual_seed(5)
    if kind == "small":
        vit = _TimmViT(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4, mlp_ratio=2, qkv_bias=True,
                       norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
        model, heads, b, size = MAE(vit, decoder_dim=512, decoder_depth=2, decoder_num_heads=16), 4, 3, 64
    else:
        model, heads, b, size = MAE(vit_base_patch16_224()), 12, 2, 224
    _perturb(model, 9)
    g = torch.Generator().manual_seed(21)
    images = torch.randn(b, 3, size, size, generator=g)
    idx_keep, idx_mask = aref.random_token_mask(torch.rand(b, model.sequence_length, generator=g), 0.75)
    idx_keep = idx_keep.flip(1).contiguous()              # not sorted: the class token last
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _CACHE[kind] = (model, sd0, heads, images, idx_keep, idx_mask.contiguous())
    return _CACHE[kind]


def _leaves(sd0):
    return {k: v.clone().requires_grad_(True) for k, v in sd0.items()}


def _check_grads(model, sd, what):
    named = dict(model.named_parameters())
    refs = {n: sd[n].grad for n in named if not _unused(n)}
    assert all(r is not None for r in refs.values())
    rms = max((r.norm() / r.numel() ** 0.5).item() for r in refs.values())
    worst = ("", 0.0)
    for n, p in named.items():
        if _unused(n):
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        got, ref = p.grad.detach().cpu().double(), refs[n].double()
        floor = 1e-3 * rms * ref.numel() ** 0.5
        err = ((got - ref).norm() / (ref.norm() + floor)).item()
        assert err <= 1e-2, (what, n, err)
        if ref.norm().item() > floor:
            cos = F.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
            assert cos >= 0.9999, (what, n, cos)
        if err > worst[1]:
            worst = (n, err)
    print(f"{what}: worst relative gradient error {worst[1]:.2e} ({worst[0]})")


def _forward_and_gradients(kind):
    model, sd0, heads, images, idx_keep, idx_mask = _setup(kind)
    sd = _leaves(sd0)
    ref_out, ref_target = aref.mae_forward(sd, images, idx_keep, idx_mask, heads, 16)
    wgt = torch.randn(ref_out.shape, generator=torch.Generator().manual_seed(2))
    (ref_out * wgt).sum().backward()
    model = model.cuda().train()
    model.zero_grad()
    x_pred, target = model(images.cuda(), idx_keep.cuda(), idx_mask.cuda())
    assert x_pred.requires_grad and not target.requires_grad and x_pred.shape == target.shape == ref_out.shape
    assert target.dtype == torch.float32 and torch.equal(target.cpu().view(torch.int32), ref_target.view(torch.int32))
    cos = 1 - F.cosine_similarity(x_pred.detach().cpu().double(), ref_out.detach().double(), dim=2)
    print(f"{kind}: worst x_pred row cosine error {cos.max().item():.2e}")
    assert cos.max() <= 1e-3
    (x_pred * wgt.cuda()).sum().backward()
    _check_grads(model, sd, f"{kind} forward")
    model.cpu()


def _fused(kind):
    model, sd0, heads, images, idx_keep, idx_mask = _setup(kind)
    model = model.cuda().train()
    with torch.no_grad():
        x_gpu, target = (t.cpu().double() for t in model(images.cuda(), idx_keep.cuda(), idx_mask.cuda()))
    sd = _leaves(sd0)
    ref_out, ref_target = aref.mae_forward(sd, images, idx_keep, idx_mask, heads, 16)
    ref_loss_t = aref.mse_loss(ref_out, ref_target)
    ref_loss_t.backward()
    x_ref = ref_out.detach().double()
    ref_loss = aref.mse_loss(x_ref, ref_target.double()).item()
    model.zero_grad()
    loss = model.masked_loss(images.cuda(), idx_keep.cuda(), idx_mask.cuda())
    assert loss.dim() == 0 and loss.requires_grad and loss.dtype == torch.float32
    slack = ((x_gpu - x_ref).abs() * ((x_gpu - target).abs() + (x_ref - target).abs())).mean().item()
    n = x_gpu.shape[0] * x_gpu.shape[1]
    bound = aref.gamma(aref.mse_k(n, x_gpu.shape[2])) * aref.mse_loss(x_gpu, target).item()
    print(f"{kind}: loss {loss.item():.6f} ref {ref_loss:.6f}, |diff| {abs(loss.item() - ref_loss):.2e} <= "
          f"{slack:.2e} + {bound:.2e}")
    assert abs(loss.item() - ref_loss) <= slack + bound
    loss.backward()
    _check_grads(model, sd, f"{kind} fused")
    model.cpu()


def test_small_forward_and_gradients(hcir_built):
    _forward_and_gradients("small")


def test_small_fused_loss_and_gradients(hcir_built):
    _fused("small")


def test_small_random_mask_and_loss_scale(hcir_built):
    """No indices given: the model draws lightly's pair; gradients stay finite under a GradScaler's 2^16."""
    model, _, _, images, _, _ = _setup("small")
    model = model.cuda().train()
    model.zero_grad()
    x_pred, target = model(images.cuda())
    assert tuple(x_pred.shape) == tuple(target.shape) == (3, 13, 768)
    loss = model.masked_loss(images.cuda())
    torch.amp.GradScaler("cuda", init_scale=2.0 ** 16).scale(loss).backward()
    for n, p in model.named_parameters():
        if not _unused(n):
            assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    model.zero_grad()
    model.cpu()


def test_small_train_step(hcir_built):
    from hcir.pretrain_engine import MAETrainStep
    model, sd0, _, images, _, _ = _setup("small")
    model = model.cuda()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    step = MAETrainStep(model, torch.optim.Adam(model.parameters(), lr=1e-3), torch.amp.GradScaler("cuda"))
    out = step({"anchor": images.cuda()})
    assert set(out) == {"loss"} and 0 < out["loss"] < 100
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]) == _unused(n), n
        assert p.grad is None or not p.grad.any(), n                       # zero_grad closes the step
    model.load_state_dict(sd0)
    model.cpu()


def test_vit_base_fused_loss_and_gradients(hcir_built):
    _fused("vit_base")


def test_train_from_files_cli_mae(hcir_built, tmp_path, monkeypatch, capsys):
    """tools/train_from_files.py --mode mae, the command itself: one epoch (two steps of four images) of
    MAE(vit_base_patch16_224()) on eight PNG files, one device view per image, torch's Adam and GradScaler."""
    import numpy as np
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(0)
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    rows = []
    for i in range(8):
        Image.fromarray(rng.integers(0, 255, (240, 250, 3), dtype=np.uint8)).save(img_dir / f"im_{i}.png")
        rows.append(f"im_{i}.png,{i % 3}")
    (tmp_path / "train.csv").write_text("id,class\n" + "\n".join(rows) + "\n")
    monkeypatch.syspath_prepend(os.path.join(root, "tools"))
    import train_from_files
    monkeypatch.setattr(sys, "argv", ["train_from_files.py", "--csv", str(tmp_path / "train.csv"), "--img-dir",
                                      str(img_dir), "--batch-size", "4", "--workers", "0", "--mode", "mae"])
    train_from_files.main()
    torch.cuda.synchronize()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert [ln.split(":")[0] for ln in lines] == ["step 0", "step 1"]
    for ln in lines:
        vals = dict(kv.split("=") for kv in ln.split(": ", 1)[1].split())
        assert set(vals) == {"loss"} and 0 < float(vals["loss"]) < 100
