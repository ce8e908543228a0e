"""hcir.backbone.SimMIM on an MI355X against the fp32 CPU restatement (tests/_mim_ref.py) and torch's autograd through
it: forward(images, idx_mask), the fused masked_loss, SimMIMTrainStep and extract_features.

Bars: every x_out row within cosine 1e-3 of the restatement (the project's embedding bar); every gradient within 1e-2
in relative norm and cosine >= 0.9999 (the bar of tests/test_vit_train_gpu.py), error norms taken against the
gradient's own norm plus a floor of 1e-3 of the largest per-element gradient RMS times sqrt(numel), and the cosine
only asked of tensors whose reference norm is above that floor (a gradient that is zero in exact arithmetic has only
rounding noise to compare).  The L1 gradient is discontinuous in x_out, so the oracle never re-decides a sign: the
fused gradients are compared with autograd of sum(x_out_ref * S) / N for S = sign(x_out_gpu - target).  The loss must
lie within mean|x_out_gpu - x_out_ref| (triangle inequality) plus the kernel's own bound of the restatement's loss.

The small model is the walk test's shape (dim 256, 4 heads, mlp 512, depth 3, 64 x 64, patch 16, batch 3, 13 masked
tokens per image); one case runs the whole ViT-B/16 at batch 2 (197 tokens, 148 masked)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mim_ref as mref

pytestmark = pytest.mark.gpu
_CACHE = {}


def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "heads.head" in n:
                continue
            if n.endswith(("ln_1.weight", "ln_2.weight", "ln.weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        for p in (model.backbone.vit.class_token, model.backbone.mask_token):
            p.copy_(0.02 * torch.randn(p.shape, generator=g))


def _setup(kind):
    """(model on the CPU, its reference state dict with autograd leaves, heads, images, idx_mask), built once."""
    if kind in _CACHE:
        return _CACHE[kind]
    from hcir import _tv_vit
    from hcir.backbone import SimMIM
    torch.manual_seed(5)
    if kind == "small":
        vit, heads, b, size = _tv_vit.TVVisionTransformer(image_size=64, patch_size=16, num_layers=3, num_heads=4,
                                                          hidden_dim=256, mlp_dim=512), 4, 3, 64
    else:
        vit, heads, b, size = _tv_vit.vit_b_16(), 12, 2, 224
    model = SimMIM(vit)
    _perturb(model, 9)
    g = torch.Generator().manual_seed(21)
    images = torch.randn(b, 3, size, size, generator=g)
    _, idx_mask = mref.random_token_mask(torch.rand(b, model.sequence_length, generator=g), 0.75)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _CACHE[kind] = (model, sd0, heads, images, idx_mask)
    return _CACHE[kind]


def _leaves(sd0):
    return {k: v.clone().requires_grad_(True) for k, v in sd0.items()}


def _check_grads(model, sd, what):
    named = dict(model.named_parameters())
    refs = {n: sd[n].grad for n in named if "heads.head" not in n}
    assert all(r is not None for r in refs.values())
    rms = max((r.norm() / r.numel() ** 0.5).item() for r in refs.values())
    worst = ("", 0.0)
    for n, p in named.items():
        if "heads.head" in n:
            assert p.grad is None, n                        # unused container: never given a gradient
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
    model, sd0, heads, images, idx_mask = _setup(kind)
    b, n = idx_mask.shape
    sd = _leaves(sd0)
    ref_out, ref_target = mref.simmim_forward(sd, images, idx_mask, heads)
    wgt = torch.randn(ref_out.shape, generator=torch.Generator().manual_seed(2))
    (ref_out * wgt).sum().backward()
    model = model.cuda().train()
    model.zero_grad()
    x_out, target = model(images.cuda(), idx_mask.cuda())
    assert x_out.requires_grad and not target.requires_grad and x_out.shape == target.shape == ref_out.shape
    assert target.dtype == torch.float32 and torch.equal(target.cpu().view(torch.int32), ref_target.view(torch.int32))
    cos = 1 - F.cosine_similarity(x_out.detach().cpu().double(), ref_out.detach().double(), dim=2)
    print(f"{kind}: worst x_out row cosine error {cos.max().item():.2e}")
    assert cos.max() <= 1e-3
    (x_out * wgt.cuda()).sum().backward()
    _check_grads(model, sd, f"{kind} forward")
    model.cpu()


def _fused(kind):
    model, sd0, heads, images, idx_mask = _setup(kind)
    model = model.cuda().train()
    with torch.no_grad():
        x_gpu, target = (t.cpu() for t in model(images.cuda(), idx_mask.cuda()))
    sgn = torch.sign(x_gpu.double() - target.double()).float()
    sd = _leaves(sd0)
    ref_out, ref_target = mref.simmim_forward(sd, images, idx_mask, heads)
    (ref_out * sgn).sum().div(sgn.numel()).backward()
    ref_loss = mref.l1_loss(ref_out.detach().double(), ref_target.double()).item()
    model.zero_grad()
    loss = model.masked_loss(images.cuda(), idx_mask.cuda())
    assert loss.dim() == 0 and loss.requires_grad and loss.dtype == torch.float32
    slack = (x_gpu.double() - ref_out.detach().double()).abs().mean().item()
    bound = mref.gamma(mref.l1_k(sgn.shape[0] * sgn.shape[1], sgn.shape[2])) * ref_loss
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


@pytest.mark.parametrize("scale", [None, 2.0 ** 16], ids=["no-scaler", "scale-2^16"])
def test_small_fused_gradients_survive_the_loss_scale(hcir_built, scale):
    model, _, _, images, idx_mask = _setup("small")
    model = model.cuda().train()
    model.zero_grad()
    loss = model.masked_loss(images.cuda(), idx_mask.cuda())
    if scale is None:
        loss.backward()
    else:
        torch.amp.GradScaler("cuda", init_scale=scale).scale(loss).backward()
    for n, p in model.named_parameters():
        if "heads.head" not in n:
            assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
    model.cpu()


def test_vit_b_16_fused_loss_and_gradients(hcir_built):
    _fused("vit_b_16")


def test_vit_b_16_train_step(hcir_built):
    from hcir.pretrain_engine import SimMIMTrainStep
    model, sd0, _, images, _ = _setup("vit_b_16")
    model = model.cuda()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    step = SimMIMTrainStep(model, torch.optim.Adam(model.parameters(), lr=1e-3), torch.amp.GradScaler("cuda"))
    out = step(images.cuda())
    assert set(out) == {"loss"} and 0 < out["loss"] < 10
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]) == ("heads.head" in n), n
        assert p.grad is None or not p.grad.any(), n                       # zero_grad closes the step
    model.load_state_dict(sd0)
    model.cpu()


def test_extract_features(hcir_built):
    from hcir.vit_engine import VitEngine
    model, sd0, heads, images, idx_mask = _setup("small")
    model = model.cuda().eval()
    x = images.cuda()
    with torch.no_grad():
        none = model.extract_features(x, torch.zeros((x.shape[0], 0), dtype=torch.int64, device=x.device))
        eng = VitEngine(model._spec(), x.device)
        plain = eng.cls_embedding(eng.forward_tokens(x, cls_only_last=True), final_norm=True, l2_normalize=False)
        assert torch.equal(none.view(torch.int32), plain.view(torch.int32))
        fixed = model.extract_features(x, idx_mask.cuda())
        ref = mref.encode(sd0, images, idx_mask, heads)[:, 0]
        cos = 1 - F.cosine_similarity(fixed.cpu().double(), ref.double(), dim=1)
        print(f"extract_features, fixed mask: worst cosine error {cos.max().item():.2e}")
        assert cos.max() <= 1e-3
        assert not torch.equal(fixed, none)
        a = model.extract_features(x, generator=torch.Generator().manual_seed(4))
        b = model.extract_features(x, generator=torch.Generator().manual_seed(4))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and a.shape == (x.shape[0], 256)
    with pytest.raises(NotImplementedError):
        model.extract_features(x)
    model.cpu()
