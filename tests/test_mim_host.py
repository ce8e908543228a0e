"""SimMIM without a GPU: the wiring of the masked walk (hcir.vit_train.VitTrainer.forward_mim / backward_mim) against
torch's autograd through the restatement (tests/_mim_ref.py), both in float64 over stand-in ops
(tests/_mim_walk_ref.py); random_token_mask; the reference's state-dict keys; the CLI; the argument checks; and the
kernels' derived bounds against fp32 emulations of their reductions, with mutations that must miss them.

The walk's case is test_vit_walk_host.py's: dim 256, 4 heads, mlp 512, depth 3, 64 x 64 images, patch 16 (17 tokens),
batch 3, mask ratio 0.75: 13 masked tokens per image, 39 compact rows padding to 64, 51 stream rows padding to 64, 48
patch rows padding to 64.  Compared: pred and all 4 + 12*3 + 2 + 3 gradients (mask_token, decoder.*, conv_proj.*
among them) for both keep_recomputable settings, by the error rule of that file.  Both sides are float64 and differ
only in summation order.  Measured here: worst error of the unmutated walk 1.6e-15; TOL is 100 x that, rounded up to
a power of ten.  Three mutations must each miss TOL by at least 10^6."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mim_ref as mref
import _mim_walk_ref as ref_ops

TOL = 1e-12
DIM, HEADS, MLP, DEPTH, PATCH, SIZE, B, RATIO = 256, 4, 512, 3, 16, 64, 3, 0.75
T = (SIZE // PATCH) ** 2 + 1
PDIM = 3 * PATCH * PATCH
_LAYER_KEYS = (("ln1_w", "ln_1.weight"), ("ln1_b", "ln_1.bias"), ("qkv_w", "self_attention.in_proj_weight"),
               ("qkv_b", "self_attention.in_proj_bias"), ("proj_w", "self_attention.out_proj.weight"),
               ("proj_b", "self_attention.out_proj.bias"), ("ln2_w", "ln_2.weight"), ("ln2_b", "ln_2.bias"),
               ("fc1_w", "mlp.0.weight"), ("fc1_b", "mlp.0.bias"), ("fc2_w", "mlp.3.weight"), ("fc2_b", "mlp.3.bias"))
_CASE = []


def _case():
    """The spec, the SimMIM extras, the input, the mask, and the restatement's pred and gradients, computed once."""
    if _CASE:
        return _CASE[0]
    from hcir.vit_engine import VitLayer, VitSpec
    g = torch.Generator().manual_seed(47)
    r = lambda *s, scale=1.0: scale * torch.randn(*s, generator=g, dtype=torch.float64)
    gain = lambda: 1.0 + r(DIM, scale=0.2)
    bias = lambda n: r(n, scale=0.05)
    w = lambda n, k: r(n, k, scale=k ** -0.5)
    layers = [VitLayer(ln1_w=gain(), ln1_b=bias(DIM), qkv_w=w(3 * DIM, DIM), qkv_b=bias(3 * DIM), proj_w=w(DIM, DIM),
                       proj_b=bias(DIM), ln2_w=gain(), ln2_b=bias(DIM), fc1_w=w(MLP, DIM), fc1_b=bias(MLP),
                       fc2_w=w(DIM, MLP), fc2_b=bias(DIM)) for _ in range(DEPTH)]
    spec = VitSpec(patch=PATCH, dim=DIM, heads=HEADS, eps=1e-6, pos_mult=1.0,
                   conv_w=w(DIM, PDIM).view(DIM, 3, PATCH, PATCH), conv_b=bias(DIM),
                   cls=r(1, 1, DIM, scale=0.02), pos=r(1, T, DIM, scale=0.02), layers=layers,
                   final_ln_w=gain(), final_ln_b=bias(DIM))
    mim = (r(1, 1, DIM, scale=0.02), w(PDIM, DIM), bias(PDIM))
    x = r(B, 3, SIZE, SIZE)
    idx_keep, idx_mask = mref.random_token_mask(torch.rand(B, T, generator=g), RATIO)
    wgt = r(B * idx_mask.shape[1], PDIM)
    leaf = lambda t: t.clone().requires_grad_(True)
    p = "backbone.vit."
    sd = {p + "conv_proj.weight": leaf(spec.conv_w), p + "conv_proj.bias": leaf(spec.conv_b),
          p + "class_token": leaf(spec.cls), p + "encoder.pos_embedding": leaf(spec.pos)}
    order = list(sd)
    for i, l in enumerate(layers):
        for field, key in _LAYER_KEYS:
            sd[f"{p}encoder.layers.encoder_layer_{i}.{key}"] = leaf(getattr(l, field))
            order.append(f"{p}encoder.layers.encoder_layer_{i}.{key}")
    sd[p + "encoder.ln.weight"], sd[p + "encoder.ln.bias"] = leaf(spec.final_ln_w), leaf(spec.final_ln_b)
    sd["backbone.mask_token"], sd["decoder.weight"], sd["decoder.bias"] = (leaf(t) for t in mim)
    order += [p + "encoder.ln.weight", p + "encoder.ln.bias", "backbone.mask_token", "decoder.weight", "decoder.bias"]
    x_out, _ = mref.simmim_forward(sd, x, idx_mask, num_heads=HEADS)
    pred = x_out.reshape(-1, PDIM)
    (pred * wgt).sum().backward()
    _CASE.append((spec, mim, x, idx_keep, idx_mask, wgt, pred.detach(), [sd[k].grad for k in order]))
    return _CASE[0]


def _worst(keep, ops=ref_ops, scatter_to_kept=False):
    """Largest error of the walk over `ops` against the restatement: pred and every gradient."""
    from hcir.vit_train import VitTrainer
    spec, mim, x, idx_keep, idx_mask, wgt, pred0, g0 = _case()
    trainer = VitTrainer(spec, torch.device("cpu"), ops=ops, keep_recomputable=keep, cls_only_last=False, mim=mim)
    pred, saved = trainer.forward_mim(x, idx_mask)
    rows = B * idx_mask.shape[1]
    assert (rows, tuple(pred.shape)) == (39, (64, PDIM)) and not pred[rows:].any()
    if scatter_to_kept:                                   # the mutation: the compact rows' gradient lands on kept rows
        kept = (torch.arange(B)[:, None] * T + idx_keep).reshape(-1)
        saved.mim.flat = kept.repeat(-(-rows // kept.numel()))[:rows]
    grads = trainer.backward_mim(saved, wgt)
    assert len(grads) == len(g0) == 4 + 12 * DEPTH + 2 + 3
    assert all(a.shape == b.shape == p.shape for a, b, p in zip(grads, g0, trainer.params() + trainer.mim_params()))
    rms = max((t.norm() / t.numel() ** 0.5).item() for t in g0)
    errs = [((pred[:rows] - pred0).norm() / pred0.norm()).item()]
    errs += [((a - b).norm() / (b.norm() + 1e-3 * rms * b.numel() ** 0.5)).item() for a, b in zip(grads, g0)]
    return max(errs)


@pytest.mark.parametrize("keep", [True, False], ids=["keep=1", "keep=0"])
def test_masked_walk_is_simmim(keep):
    worst = _worst(keep)
    print(f"keep={int(keep)}: masked walk vs autograd, worst error over pred and gradients {worst:.3e}")
    assert worst <= TOL


def _wrapped(name, wrapper):
    ops = types.SimpleNamespace(**{k: v for k, v in vars(ref_ops).items() if not k.startswith("__")})
    setattr(ops, name, wrapper(getattr(ref_ops, name)))
    return ops


def _mask_not_applied(mim_mask_tokens):
    return lambda *a, **k: None


def _dpatch_not_zeroed(mim_mask_bwd):
    def f(dtok, b, t, mask, g_mask_token, dpatch):
        mim_mask_bwd(dtok, b, t, mask, g_mask_token, dpatch)
        dpatch[: b * (t - 1)] = dtok[: b * t].view(b, t, -1)[:, 1:].reshape(b * (t - 1), -1)
    return f


@pytest.mark.parametrize("keep", [True, False], ids=["keep=1", "keep=0"])
@pytest.mark.parametrize("mutation", ["mask_not_applied", "dpatch_not_zeroed", "scatter_to_kept_rows"])
def test_a_wiring_error_is_seen(mutation, keep):
    if mutation == "mask_not_applied":
        worst = _worst(keep, _wrapped("mim_mask_tokens", _mask_not_applied))
    elif mutation == "dpatch_not_zeroed":
        worst = _worst(keep, _wrapped("mim_mask_bwd", _dpatch_not_zeroed))
    else:
        worst = _worst(keep, scatter_to_kept=True)
    print(f"{mutation}, keep={int(keep)}: worst error {worst:.3e}")
    assert worst >= 1e6 * TOL


def test_cls_exit_is_untouched_by_the_mim_extras():
    """forward / backward of a trainer that carries the SimMIM extras are those of one that does not."""
    from hcir.vit_train import VitTrainer
    spec, mim, x, *_ = _case()
    wgt = torch.randn(B, DIM, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    outs = []
    for extra in (None, mim):
        tr = VitTrainer(spec, torch.device("cpu"), ops=ref_ops, mim=extra)
        cls, sv = tr.forward(x)
        outs.append([cls] + tr.backward(sv, wgt))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---------------------------------------------------------------------------------------------------------------
# random_token_mask
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,num_keep", [(197, 49), (17, 4)])
def test_random_token_mask(seq, num_keep):
    from hcir.backbone import random_token_mask
    keep, mask = random_token_mask((5, seq), 0.75, generator=torch.Generator().manual_seed(11))
    assert keep.shape == (5, num_keep) and mask.shape == (5, seq - num_keep) and keep.dtype == torch.int64
    assert (keep[:, 0] == 0).all() and not (mask == 0).any()              # the class token is never masked
    both = torch.cat([keep, mask], 1).sort(1).values
    assert torch.equal(both, torch.arange(seq).expand(5, seq))             # together: a permutation of the tokens
    noise = torch.rand(5, seq, generator=torch.Generator().manual_seed(11))
    k0, m0 = mref.random_token_mask(noise, 0.75)
    assert torch.equal(keep, k0) and torch.equal(mask, m0)                 # argsort of the same noise
    kc, mc = random_token_mask((5, seq), 0.75, mask_class_token=True, generator=torch.Generator().manual_seed(11))
    assert kc.shape[1] == num_keep and (mc == 0).any()                     # class token maskable when asked


# ---------------------------------------------------------------------------------------------------------------
# state dict, CLI, argument checks
# ---------------------------------------------------------------------------------------------------------------
def _model():
    from hcir._tv_vit import vit_b_16
    from hcir.backbone import SimMIM
    return SimMIM(vit_b_16())


def test_state_dict_has_the_reference_keys(golden_dir):
    with open(os.path.join(golden_dir, "simmim_state_keys.json")) as f:
        keys = json.load(f)
    assert keys["decoder.weight"] == [768, 768] and keys["backbone.mask_token"] == [1, 1, 768]
    assert keys["backbone.vit.heads.head.weight"] == [1000, 768]
    model = _model()
    sd = {k: torch.full(shape, 0.5) for k, shape in keys.items()}
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == keys
    assert (model.mask_ratio, model.patch_size, model.sequence_length) == (0.75, 16, 197)
    assert (model.decoder.bias.detach() == 0.5).all() and (model.backbone.mask_token.detach() == 0.5).all()


def test_cli_builds_simmim():
    import knn_classification as cli
    from hcir.backbone import SimMIM
    model = cli.build_model(cli.parse_args(["--mode", "simMIM", "--model", "vit_b_16"]))
    assert isinstance(model, SimMIM) and tuple(model.decoder.weight.shape) == (768, 768)


def test_bad_idx_mask_raises_before_any_launch(monkeypatch):
    import hcir._lib as L
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("library call")))
    model = _model()
    x = torch.zeros(2, 3, 224, 224)
    for bad in (torch.tensor([[1, 197], [2, 3]]), torch.tensor([[1, 2], [-1, 3]]), torch.tensor([[0, 2], [1, 3]]),
                torch.tensor([[5, 5], [1, 3]]), torch.zeros((2, 0), dtype=torch.int64),
                torch.tensor([[1, 2]]), torch.tensor([[1.0, 2.0], [1.0, 3.0]])):
        with pytest.raises(ValueError):
            model.masked_loss(x, bad)
        with pytest.raises(ValueError):
            model(x, bad)
    with pytest.raises(NotImplementedError):
        model.extract_features(x)                         # grad enabled, trainable parameters


# ---------------------------------------------------------------------------------------------------------------
# bounds: the fp32 emulation of each reduction sits inside its bound, a mutation misses it tenfold
# ---------------------------------------------------------------------------------------------------------------
def _bwd_case(b, t, d, seed):
    rng = np.random.default_rng(seed)
    dtok = rng.standard_normal((b * t, d)).astype(np.float32) * np.float32(3e-3)
    mask = (rng.random((b, t)) < 0.75).astype(np.uint8)
    mask[:, 0] = 0
    return dtok, mask.reshape(-1)


@pytest.mark.parametrize("b,t,d", [(3, 17, 256), (2, 197, 768), (9, 17, 64)])
def test_g_mask_token_bound(b, t, d):
    dtok, mask = _bwd_case(b, t, d, 5)
    terms = dtok.astype(np.float64)[mask != 0]
    exact, bound = terms.sum(0), mref.gamma(mref.g_mask_token_k(b * t)) * np.abs(terms).sum(0)
    err = np.abs(mref.emulate_mask_bwd(dtok, mask).astype(np.float64) - exact)
    print(f"g_mask_token {b}x{t}x{d}: k {mref.g_mask_token_k(b * t)}, worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    # mutations: fp16 row lanes; every row summed
    e16 = np.abs(mref.emulate_mask_bwd(dtok, mask, np.float16).astype(np.float64) - exact)
    eall = np.abs(mref.emulate_mask_bwd(dtok, np.ones_like(mask)).astype(np.float64) - exact)
    print(f"   fp16 lanes {np.max(e16 / bound):.1f} x bound, all rows {np.max(eall / bound):.1f} x bound")
    assert np.max(e16 / bound) >= 10 and np.max(eall / bound) >= 10


@pytest.mark.parametrize("rows,p", [(1, 192), (39, 768), (151, 192), (1100, 192)])
def test_l1_loss_bound(rows, p):
    rng = np.random.default_rng(rows)
    target = rng.standard_normal((rows, p)).astype(np.float32)
    pred = (target + rng.standard_normal((rows, p)).astype(np.float32) * np.float32(0.5)).astype(np.float16)
    terms = np.abs(pred.astype(np.float64) - target.astype(np.float64))
    exact, bound = terms.mean(), mref.gamma(mref.l1_k(rows, p)) * terms.mean()
    err = abs(float(mref.emulate_l1(pred, target)) - exact)
    print(f"l1 {rows}x{p}: k {mref.l1_k(rows, p)}, err/bound {err / bound:.3f}")
    assert err <= bound
    if rows > 1:   # mutation: the last row of every share with more than one row is dropped (one share: rows <= 1024)
        emut = abs(float(mref.emulate_l1(pred, target, skip_last_row_of_share=True)) - exact)
        if mref.l1_plan(rows)[1] > 1:
            print(f"   last row of a share dropped: {emut / bound:.1f} x bound")
            assert emut >= 10 * bound
    # mutation: differences rounded to fp16 towards zero lose 2^-11 of every term
    t16 = np.abs(pred.astype(np.float32) - target).astype(np.float16).astype(np.float64)
    t16 = np.where(t16 > terms, np.nextafter(t16.astype(np.float16), np.float16(0)).astype(np.float64), t16)
    assert abs(t16.mean() - exact) >= 10 * bound


def test_masked_token_bound():
    rng = np.random.default_rng(2)
    mt, pos = (rng.standard_normal(s).astype(np.float32) * np.float32(0.02) for s in ((256,), (17, 256)))
    for pos_mult in (1.0, 2.0):
        exact = mt.astype(np.float64) + pos_mult * pos.astype(np.float64)
        v32 = (mt.astype(np.float64) + pos_mult * pos.astype(np.float64)).astype(np.float32)   # one rounding: the fma
        for f16 in (True, False):
            got = v32.astype(np.float16).astype(np.float64) if f16 else v32.astype(np.float64)
            bound = mref.mask_token_bound(exact, f16)
            assert (np.abs(got - exact) <= bound).all()
            wrong = np.roll(got, 1, axis=0)               # mutation: the position of the neighbouring token
            assert np.max(np.abs(wrong - exact) / bound) >= 10
