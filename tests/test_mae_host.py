"""MAE without a GPU: the wiring of the masked-encoder / decoder walk (hcir.vit_train.MaeTrainer) against torch's
autograd through the restatement (tests/_mae_ref.py), both in float64 over stand-in ops (tests/_mae_walk_ref.py); the
model's state-dict keys, index validation, MAETrainStep and the CLIs; and the kernels' derived bounds against fp32
emulations of their reductions, with mutations that must miss them.

The walk's case: encoder dim 256, 4 heads (head_dim 64), mlp 512, depth 2; decoder dim 512, 16 heads (head_dim 32), mlp
2048, depth 2; 64 x 64 images, patch 16 (17 tokens), batch 3, mask ratio 0.75: int(17 * 0.25) = 4 kept and 13 masked
tokens per image, compact heights 12 and 39 (both pad to 64), 51 stream rows (pad to 64).  Compared: pred and all
4 + 12*2 + 2 + 3 + 12*2 + 4 gradients for both keep_recomputable settings, by the error rule of test_mim_host.py, and the
fused MSE loss with its gradients.  Both sides are float64 and differ only in summation order.  Measured here: worst
error of the unmutated walk 2.2e-15; TOL is 100 x that, rounded up to a power of ten.  Three mutations must each miss
TOL by at least 10^6."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mae_ref as aref
import _mae_walk_ref as ref_ops

TOL = 1e-12
DIM, HEADS, MLP, DEPTH = 256, 4, 512, 2
DDIM, DHEADS, DMLP, DDEPTH = 512, 16, 2048, 2
PATCH, SIZE, B, RATIO = 16, 64, 3, 0.75
T = (SIZE // PATCH) ** 2 + 1
PDIM = 3 * PATCH * PATCH
_BLOCK_KEYS = (("ln1_w", "norm1.weight"), ("ln1_b", "norm1.bias"), ("qkv_w", "attn.qkv.weight"),
               ("qkv_b", "attn.qkv.bias"), ("proj_w", "attn.proj.weight"), ("proj_b", "attn.proj.bias"),
               ("ln2_w", "norm2.weight"), ("ln2_b", "norm2.bias"), ("fc1_w", "mlp.fc1.weight"),
               ("fc1_b", "mlp.fc1.bias"), ("fc2_w", "mlp.fc2.weight"), ("fc2_b", "mlp.fc2.bias"))
_CASE = []


def _case():
    """The two specs, the input, the index pair, and the restatement's pred, loss and gradients, computed once."""
    if _CASE:
        return _CASE[0]
    from hcir.vit_engine import VitLayer, VitSpec
    g = torch.Generator().manual_seed(53)
    r = lambda *s, scale=1.0: scale * torch.randn(*s, generator=g, dtype=torch.float64)
    w = lambda n, k: r(n, k, scale=k ** -0.5)

    def layer(d, mlp):
        gain, bias = lambda: 1.0 + r(d, scale=0.2), lambda n: r(n, scale=0.05)
        return VitLayer(ln1_w=gain(), ln1_b=bias(d), qkv_w=w(3 * d, d), qkv_b=bias(3 * d), proj_w=w(d, d),
                        proj_b=bias(d), ln2_w=gain(), ln2_b=bias(d), fc1_w=w(mlp, d), fc1_b=bias(mlp),
                        fc2_w=w(d, mlp), fc2_b=bias(d))
    enc_layers = [layer(DIM, MLP) for _ in range(DEPTH)]
    spec = VitSpec(patch=PATCH, dim=DIM, heads=HEADS, eps=1e-6, pos_mult=1.0,
                   conv_w=w(DIM, PDIM).view(DIM, 3, PATCH, PATCH), conv_b=r(DIM, scale=0.05),
                   cls=r(1, 1, DIM, scale=0.02), pos=r(1, T, DIM, scale=0.02), layers=enc_layers,
                   final_ln_w=1.0 + r(DIM, scale=0.2), final_ln_b=r(DIM, scale=0.05))
    dec = types.SimpleNamespace(embed_w=w(DDIM, DIM), embed_b=r(DDIM, scale=0.05), mask_token=r(1, 1, DDIM, scale=0.5),
                                pos=r(1, T, DDIM, scale=0.5), layers=[layer(DDIM, DMLP) for _ in range(DDEPTH)],
                                heads=DHEADS, eps=1e-6, norm_w=1.0 + r(DDIM, scale=0.2), norm_b=r(DDIM, scale=0.05),
                                pred_w=w(PDIM, DDIM), pred_b=r(PDIM, scale=0.05))
    x = r(B, 3, SIZE, SIZE)
    idx_keep, idx_mask = aref.random_token_mask(torch.rand(B, T, generator=g), RATIO)
    idx_keep = idx_keep.flip(1).contiguous()              # not sorted, the class token last
    idx_mask = idx_mask.contiguous()
    wgt = r(B * idx_mask.shape[1], PDIM)
    leaf = lambda t: t.clone().requires_grad_(True)
    p = "backbone.vit."
    sd = {p + "patch_embed.proj.weight": leaf(spec.conv_w), p + "patch_embed.proj.bias": leaf(spec.conv_b),
          p + "cls_token": leaf(spec.cls), p + "pos_embed": leaf(spec.pos)}
    for i, l in enumerate(enc_layers):
        for field, key in _BLOCK_KEYS:
            sd[f"{p}blocks.{i}.{key}"] = leaf(getattr(l, field))
    sd[p + "norm.weight"], sd[p + "norm.bias"] = leaf(spec.final_ln_w), leaf(spec.final_ln_b)
    sd["decoder.decoder_embed.weight"], sd["decoder.decoder_embed.bias"] = leaf(dec.embed_w), leaf(dec.embed_b)
    sd["decoder.mask_token"] = leaf(dec.mask_token)
    for i, l in enumerate(dec.layers):
        for field, key in _BLOCK_KEYS:
            sd[f"decoder.decoder_blocks.{i}.{key}"] = leaf(getattr(l, field))
    sd["decoder.decoder_norm.weight"], sd["decoder.decoder_norm.bias"] = leaf(dec.norm_w), leaf(dec.norm_b)
    sd["decoder.decoder_pred.weight"], sd["decoder.decoder_pred.bias"] = leaf(dec.pred_w), leaf(dec.pred_b)
    order = list(sd)                                      # the order of MaeTrainer.params()
    sd["decoder.decoder_pos_embed"] = dec.pos             # no gradient
    x_pred, target = aref.mae_forward(sd, x, idx_keep, idx_mask, HEADS, DHEADS)
    pred = x_pred.reshape(-1, PDIM)
    (pred * wgt).sum().backward(retain_graph=True)
    g_lin = [sd[k].grad.clone() for k in order]
    for k in order:
        sd[k].grad = None
    loss = aref.mse_loss(x_pred, target)
    loss.backward()
    g_mse = [sd[k].grad for k in order]
    _CASE.append((spec, dec, x, idx_keep, idx_mask, wgt, pred.detach(), g_lin, loss.detach(), g_mse))
    return _CASE[0]


def _errors(pred, pred0, grads, g0):
    rms = max((t.norm() / t.numel() ** 0.5).item() for t in g0)
    errs = [((pred - pred0).norm() / pred0.norm()).item()]
    errs += [((a - b).norm() / (b.norm() + 1e-3 * rms * b.numel() ** 0.5)).item() for a, b in zip(grads, g0)]
    return max(errs)


def _worst(keep, ops=ref_ops):
    """Largest error of the walk over `ops` against the restatement: pred and every gradient."""
    from hcir.vit_train import MaeTrainer
    spec, dec, x, idx_keep, idx_mask, wgt, pred0, g0, _, _ = _case()
    trainer = MaeTrainer(spec, dec, torch.device("cpu"), keep_recomputable=keep, ops=ops)
    pred, saved = trainer.forward(x, idx_keep, idx_mask)
    rows = B * idx_mask.shape[1]
    assert (rows, B * idx_keep.shape[1], tuple(pred.shape)) == (39, 12, (64, PDIM)) and not pred[rows:].any()
    grads = trainer.backward(saved, wgt)
    assert len(grads) == len(g0) == 4 + 12 * DEPTH + 2 + 3 + 12 * DDEPTH + 4
    assert all(a.shape == b.shape == p.shape for a, b, p in zip(grads, g0, trainer.params()))
    return _errors(pred[:rows], pred0, grads, g0)


@pytest.mark.parametrize("keep", [True, False], ids=["keep=1", "keep=0"])
def test_walk_is_mae(keep):
    worst = _worst(keep)
    print(f"keep={int(keep)}: MAE walk vs autograd, worst error over pred and gradients {worst:.3e}")
    assert worst <= TOL


def test_fused_mse_loss_and_its_gradients():
    """vit_mae_mse_with_grad: the loss, and 2 g / N (x_pred - target) through the same walk, with an upstream factor."""
    from hcir.vit_train import MaeTrainer, vit_mae_mse_with_grad, vit_mae_with_grad
    spec, dec, x, idx_keep, idx_mask, wgt, pred0, g_lin, loss0, g_mse = _case()
    trainer = MaeTrainer(spec, dec, torch.device("cpu"), ops=ref_ops)
    params = trainer.params()
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    loss = vit_mae_mse_with_grad(trainer, x, idx_keep, idx_mask)
    (3.0 * loss).backward()
    grads = [p.grad / 3.0 for p in params]
    worst = _errors(loss.reshape(1), loss0.reshape(1), grads, g_mse)
    for p in params:
        p.grad = None
    x_pred = vit_mae_with_grad(trainer, x, idx_keep, idx_mask)
    (x_pred.reshape(-1, PDIM) * wgt).sum().backward()
    worst = max(worst, _errors(x_pred.detach().reshape(-1, PDIM), pred0, [p.grad for p in params], g_lin))
    for p in params:
        p.grad = None
        p.requires_grad_(False)
    print(f"fused MSE and differentiable forward through autograd.Function: worst error {worst:.3e}")
    assert worst <= TOL


def _wrapped(name, wrapper):
    ops = types.SimpleNamespace(**{k: v for k, v in vars(ref_ops).items() if not k.startswith("__")})
    setattr(ops, name, wrapper(getattr(ref_ops, name)))
    return ops


def _scatter_lands_on_masked_rows(scatter):
    def f(comp, b, t, idx, dtok):                         # the encoder's scatter (4 kept tokens), not the decoder's (13)
        if idx.shape[1] == 4:
            idx = _case()[4][:, :4].contiguous()
        scatter(comp, b, t, idx, dtok)
    return f


def _mask_token_sums_kept_rows(bwd):
    def f(dres, b, t, idx_keep, d_embed, g_mask_token):
        bwd(dres, b, t, idx_keep, d_embed, g_mask_token)
        g_mask_token.copy_(d_embed[: b * idx_keep.shape[1]].sum(0))
    return f


def _position_by_compact_index(dec_in):
    def f(embed, b, t, idx_keep, mask_token, pos, x):
        dec_in(embed, b, t, idx_keep, mask_token, pos, x)
        k, d = idx_keep.shape[1], mask_token.numel()
        rows = x[: b * t].view(b, t, d)
        for i in range(b):
            for j in range(k):
                rows[i, idx_keep[i, j]] = embed[i * k + j] + pos[j]
    return f


MUTATIONS = {"scatter_on_masked_rows": ("mae_scatter_rows", _scatter_lands_on_masked_rows),
             "mask_token_sums_kept_rows": ("mae_decoder_input_bwd", _mask_token_sums_kept_rows),
             "position_by_compact_index": ("mae_decoder_input", _position_by_compact_index)}


@pytest.mark.parametrize("keep", [True, False], ids=["keep=1", "keep=0"])
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_wiring_error_is_seen(mutation, keep):
    worst = _worst(keep, _wrapped(*MUTATIONS[mutation]))
    print(f"{mutation}, keep={int(keep)}: worst error {worst:.3e}")
    assert worst >= 1e6 * TOL


# ---------------------------------------------------------------------------------------------------------------
# model: state dict, initialisation, index validation, the step, the CLIs
# ---------------------------------------------------------------------------------------------------------------
_MODEL = []


def _model():
    if not _MODEL:
        from hcir.backbone import MAE, vit_base_patch16_224
        torch.manual_seed(5)
        _MODEL.append(MAE(vit_base_patch16_224()))
    return _MODEL[0]


def test_state_dict_has_lightlys_decoder_keys():
    sd = {k: tuple(v.shape) for k, v in _model().state_dict().items()}
    want = {"decoder.decoder_embed.weight": (512, 768), "decoder.decoder_embed.bias": (512,),
            "decoder.mask_token": (1, 1, 512), "decoder.decoder_pos_embed": (1, 197, 512),
            "decoder.decoder_norm.weight": (512,), "decoder.decoder_norm.bias": (512,),
            "decoder.decoder_pred.weight": (768, 512), "decoder.decoder_pred.bias": (768,)}
    blk = {"norm1.weight": (512,), "norm1.bias": (512,), "attn.qkv.weight": (1536, 512), "attn.qkv.bias": (1536,),
           "attn.proj.weight": (512, 512), "attn.proj.bias": (512,), "norm2.weight": (512,), "norm2.bias": (512,),
           "mlp.fc1.weight": (2048, 512), "mlp.fc1.bias": (2048,), "mlp.fc2.weight": (512, 2048), "mlp.fc2.bias": (512,)}
    for i in range(8):
        want.update({f"decoder.decoder_blocks.{i}.{k}": v for k, v in blk.items()})
    assert {k: v for k, v in sd.items() if k.startswith("decoder.")} == want
    assert sd["backbone.mask_token"] == (1, 1, 768) and sd["backbone.vit.pos_embed"] == (1, 197, 768)
    assert sd["backbone.vit.norm.weight"] == (768,) and "backbone.vit.blocks.11.mlp.fc2.bias" in sd
    model = _model()
    assert (model.mask_ratio, model.patch_size, model.sequence_length) == (0.75, 16, 197)
    res = model.load_state_dict({k: torch.full(v, 0.5) for k, v in sd.items()}, strict=True)   # with the decoder: strict
    assert not res.missing_keys and not res.unexpected_keys
    _MODEL.clear()


def test_decoder_initialisation_is_lightlys():
    dec = _model().decoder
    assert not dec.decoder_pos_embed.requires_grad and dec.mask_token.requires_grad
    pos = dec.decoder_pos_embed[0].double()
    assert not pos[0].any()                                                 # the class token's row
    # patch (row 2, column 5) = token 1 + 2 * 14 + 5: first half codes the column, second half the row
    omega = 1.0 / 10000 ** (torch.arange(128, dtype=torch.float64) / 128)
    want = torch.cat([(5 * omega).sin(), (5 * omega).cos(), (2 * omega).sin(), (2 * omega).cos()])
    assert torch.allclose(pos[1 + 2 * 14 + 5], want, atol=1e-6)
    assert 0.015 < float(dec.mask_token.detach().std()) < 0.025
    lin = dec.decoder_blocks[3].mlp.fc1
    bound = (6.0 / (512 + 2048)) ** 0.5                                     # Xavier uniform
    wmax = float(lin.weight.detach().abs().max())
    assert 0.99 * bound < wmax <= bound
    assert not lin.bias.any() and not dec.decoder_pred.bias.any() and not dec.decoder_blocks[0].attn.qkv.bias.any()
    assert bool((dec.decoder_norm.weight == 1).all()) and not dec.decoder_blocks[7].norm2.bias.any()


def test_small_decoder_keywords():
    from hcir.backbone import MAE, _TimmViT
    from functools import partial
    vit = _TimmViT(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4, mlp_ratio=2, qkv_bias=True,
                   norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    m = MAE(vit, decoder_dim=512, decoder_depth=2, decoder_num_heads=16)
    assert len(m.decoder.decoder_blocks) == 2 and tuple(m.decoder.decoder_pos_embed.shape) == (1, 17, 512)
    assert m.sequence_length == 17 and tuple(m.decoder.decoder_embed.weight.shape) == (512, 256)


def test_bad_indices_raise_before_any_launch(monkeypatch):
    import hcir._lib as L
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("library call")))
    model = _model()
    x = torch.zeros(2, 3, 224, 224)
    perm = torch.stack([torch.arange(197), torch.arange(197)])
    keep, mask = perm[:, :49], perm[:, 49:]
    swapped = perm.clone()
    swapped[0, 0], swapped[0, 100] = 100, 0                                 # class token of image 0 masked
    dup = perm.clone()
    dup[1, 60] = 61                                                          # token 61 twice, 60 never
    bad = [(keep, None), (None, mask), (keep.int(), mask), (keep, mask.float()), (keep[:1], mask[:1]),
           (keep, mask[:, :-1]), (perm, perm[:, :0]), (swapped[:, :49], swapped[:, 49:]), (dup[:, :49], dup[:, 49:]),
           (keep, mask + 1), (keep.reshape(-1), mask)]
    for k, m in bad:
        with pytest.raises(ValueError):
            model.masked_loss(x, k, m)
        with pytest.raises(ValueError):
            model(x, k, m)
    with pytest.raises(NotImplementedError):
        model.extract_features(x)                         # grad enabled, trainable parameters


def test_train_step_runs_the_reference_sequence():
    from hcir.pretrain_engine import MAETrainStep
    calls = []

    class Model:
        def train(self):
            calls.append("train")

        def masked_loss(self, images):
            calls.append(("masked_loss", tuple(images.shape)))
            return w.sum() * 2.0

    class Scaler:
        def scale(self, loss):
            calls.append("scale")
            return loss * 8.0

        def step(self, opt):
            calls.append("step")
            assert float(w.grad) == 16.0                  # the scaled loss went backward before the step
            opt.step()

        def update(self):
            calls.append("update")

    w = torch.ones(1, requires_grad=True)
    opt = torch.optim.SGD([w], lr=0.0)
    out = MAETrainStep(Model(), opt, Scaler())({"anchor": torch.zeros(2, 3, 32, 32)}, epoch=1, batch_id=0)
    assert calls == ["train", ("masked_loss", (2, 3, 32, 32)), "scale", "step", "update"] and out == {"loss": 2.0}
    assert w.grad is None or not w.grad.any()             # zero_grad
    out = MAETrainStep(Model(), opt)(torch.zeros(1, 3, 32, 32))
    assert out == {"loss": 2.0}


def test_clis_know_mae():
    import knn_classification as cli
    from hcir.backbone import MAE
    model = cli.build_model(cli.parse_args(["--mode", "mae", "--model", "vit_b_16"]))
    assert isinstance(model, MAE) and len(model.decoder.decoder_blocks) == 8
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_from_files as tff
    a = tff.build_parser().parse_args(["--csv", "x.csv", "--img-dir", "d", "--mode", "mae"])
    assert a.mode == "mae" and a.model == "vit_b_16"


# ---------------------------------------------------------------------------------------------------------------
# bounds: the fp32 emulation of each reduction sits inside its bound, a mutation misses it tenfold
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,d", [(3, 17, 256), (2, 197, 512), (300, 5, 64)])
def test_g_mask_token_bound(b, t, d):
    rng = np.random.default_rng(7)
    dres = rng.standard_normal((b * t, d)).astype(np.float32) * np.float32(3e-3)
    kept = (rng.random((b, t)) < 0.25).astype(np.uint8)
    kept[:, 0] = 1
    kept = kept.reshape(-1)
    terms = dres.astype(np.float64)[kept == 0]
    k = aref.g_mask_token_k(b, t)
    exact, bound = terms.sum(0), aref.gamma(k) * np.abs(terms).sum(0)
    err = np.abs(aref.emulate_decoder_input_bwd(dres, kept, b, t).astype(np.float64) - exact)
    print(f"g_mask_token {b}x{t}x{d}: k {k}, worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    e16 = np.abs(aref.emulate_decoder_input_bwd(dres, kept, b, t, np.float16).astype(np.float64) - exact)
    eall = np.abs(aref.emulate_decoder_input_bwd(dres, np.zeros_like(kept), b, t).astype(np.float64) - exact)
    print(f"   fp16 lanes {np.max(e16 / bound):.1f} x bound, kept rows summed too {np.max(eall / bound):.1f} x bound")
    # fp16 lanes err by ~2^-12 sqrt(terms) where the bound is k 2^-24 terms: seen tenfold while k is small, i.e. few shares
    assert np.max(eall / bound) >= 10 and (np.max(e16 / bound) >= 10 or aref.bwd_plan(b)[0] > 8)


@pytest.mark.parametrize("rows,p", [(1, 192), (39, 768), (151, 192), (1100, 192)])
def test_mse_loss_bound(rows, p):
    rng = np.random.default_rng(rows)
    target = rng.standard_normal((rows, p)).astype(np.float32)
    pred = (target + rng.standard_normal((rows, p)).astype(np.float32) * np.float32(0.5)).astype(np.float16)
    terms = (pred.astype(np.float64) - target.astype(np.float64)) ** 2
    k = aref.mse_k(rows, p)
    exact, bound = terms.mean(), aref.gamma(k) * terms.mean()
    err = abs(float(aref.emulate_mse(pred, target)) - exact)
    print(f"mse {rows}x{p}: k {k}, err/bound {err / bound:.3f}")
    assert err <= bound
    # mutation: differences cut to fp16 towards zero lose up to 2^-10 of every term (rounding them to NEAREST, as the
    # kernel does for the matrix it hands the backward, is unbiased and hides inside the bound: measured 0.4 x)
    emut = abs(float(aref.emulate_mse(pred, target, diff_to_f16_towards_zero=True)) - exact)
    print(f"   fp16 differences towards zero: {emut / bound:.1f} x bound")
    assert emut >= 10 * bound


def test_decoder_input_and_diff_bound():
    rng = np.random.default_rng(2)
    emb = (rng.standard_normal((17, 512)) * 0.7).astype(np.float16)
    pos = rng.uniform(-1, 1, (17, 512)).astype(np.float32)
    exact = emb.astype(np.float64) + pos.astype(np.float64)
    got = (emb.astype(np.float32) + pos).astype(np.float16).astype(np.float64)     # the kernel's two roundings
    bound = aref.f16_of_f32_sum_bound(exact)
    assert (np.abs(got - exact) <= bound).all()
    wrong = (emb.astype(np.float32) + np.roll(pos, 1, axis=0)).astype(np.float16).astype(np.float64)
    assert np.max(np.abs(wrong - exact) / bound) >= 10    # mutation: the position of the neighbouring token
    trunc = np.where(np.abs(got) > np.abs(exact), np.nextafter(got.astype(np.float16), np.float16(0)).astype(np.float64),
                     got)                                  # mutation: fp16 rounding towards zero - up to a whole ulp
    assert np.max(np.abs(trunc - exact) / bound) > 1
