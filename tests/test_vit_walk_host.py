"""The wiring of the ViT training walk - hcir.vit_train.VitTrainer's forward and backward, one block body over two row
sets - against torch's autograd, on the CPU in float64 with stand-in ops (tests/_vit_walk_ref.py) and no library call.
Ground truth: autograd through the oracle's functional ViTWrapper (oracle/vit.py) of sum(cls * W), same tensors.
The case is the smallest that has everything: dim 256, 4 heads, mlp 512 (every % 256 refusal of the trainer holds
unchanged), depth 3 (a first block, a middle block with the dy16 / fc2-bias handoff on both sides, the last block),
17 tokens, batch 3: m = 51 and b = 3 both pad to 64, so pad rows are live in the full and in the compact row set.
Compared: the class token and all 4 + 12*3 + 2 gradients, for the four (keep_recomputable, cls_only_last) trainers.
Each gradient's error norm is taken against the reference's norm plus a floor of 1e-3 of the largest per-element
gradient RMS times sqrt(numel) (the rule of test_forward_views_equals_separate_calls): every block's key bias has a
gradient of zero in exact arithmetic.
Both sides are float64 and differ only in summation order, so the bound measures no kernel.  Measured here: worst error
of the unmutated walk 2.35e-15 over the four variants; TOL is 100 x that, rounded up to a power of ten.  Three
mutations, each one stand-in op wrapped, show that a wiring error is seen: each must miss the bound by at least 10^6."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vit_walk_ref as ref_ops
from oracle import vit as ovit

TOL = 1e-12
DIM, HEADS, MLP, DEPTH, PATCH, SIZE, B = 256, 4, 512, 3, 16, 64, 3
T = (SIZE // PATCH) ** 2 + 1
VARIANTS = [dict(keep_recomputable=k, cls_only_last=c) for k in (True, False) for c in (True, False)]
_LAYER_KEYS = (("ln1_w", "ln_1.weight"), ("ln1_b", "ln_1.bias"), ("qkv_w", "self_attention.in_proj_weight"),
               ("qkv_b", "self_attention.in_proj_bias"), ("proj_w", "self_attention.out_proj.weight"),
               ("proj_b", "self_attention.out_proj.bias"), ("ln2_w", "ln_2.weight"), ("ln2_b", "ln_2.bias"),
               ("fc1_w", "mlp.0.weight"), ("fc1_b", "mlp.0.bias"), ("fc2_w", "mlp.3.weight"), ("fc2_b", "mlp.3.bias"))
_CASE = []


def _case():
    """The spec, its input, and the oracle's class token and gradients (in params() order), computed once."""
    if _CASE:
        return _CASE[0]
    from hcir.vit_engine import VitLayer, VitSpec
    g = torch.Generator().manual_seed(31)
    r = lambda *s, scale=1.0: scale * torch.randn(*s, generator=g, dtype=torch.float64)
    gain = lambda: 1.0 + r(DIM, scale=0.2)             # LayerNorm gains away from 1, every bias away from 0
    bias = lambda n: r(n, scale=0.05)
    w = lambda n, k: r(n, k, scale=k ** -0.5)
    layers = [VitLayer(ln1_w=gain(), ln1_b=bias(DIM), qkv_w=w(3 * DIM, DIM), qkv_b=bias(3 * DIM), proj_w=w(DIM, DIM),
                       proj_b=bias(DIM), ln2_w=gain(), ln2_b=bias(DIM), fc1_w=w(MLP, DIM), fc1_b=bias(MLP),
                       fc2_w=w(DIM, MLP), fc2_b=bias(DIM)) for _ in range(DEPTH)]
    spec = VitSpec(patch=PATCH, dim=DIM, heads=HEADS, eps=1e-6, pos_mult=ovit.POS_EMBED_MULT,
                   conv_w=w(DIM, 3 * PATCH * PATCH).view(DIM, 3, PATCH, PATCH), conv_b=bias(DIM),
                   cls=r(1, 1, DIM, scale=0.02), pos=r(1, T, DIM, scale=0.02), layers=layers,
                   final_ln_w=gain(), final_ln_b=bias(DIM))
    x, wgt = r(B, 3, SIZE, SIZE), r(B, DIM)
    leaf = lambda t: t.clone().requires_grad_(True)
    sd = {"conv_proj.weight": leaf(spec.conv_w), "conv_proj.bias": leaf(spec.conv_b), "cls_token": leaf(spec.cls),
          "pos_embedding": leaf(spec.pos), "encoder.ln.weight": leaf(spec.final_ln_w),
          "encoder.ln.bias": leaf(spec.final_ln_b)}
    sd["encoder.pos_embedding"] = sd["pos_embedding"]                  # one Parameter, two names: added twice
    order = ["conv_proj.weight", "conv_proj.bias", "cls_token", "pos_embedding"]
    for i, l in enumerate(layers):
        for field, key in _LAYER_KEYS:
            sd[f"encoder.layers.encoder_layer_{i}.{key}"] = leaf(getattr(l, field))
            order.append(f"encoder.layers.encoder_layer_{i}.{key}")
    order += ["encoder.ln.weight", "encoder.ln.bias"]
    cls = ovit.vitwrapper_forward.__wrapped__(sd, x, "", num_heads=HEADS)[0]
    (cls * wgt).sum().backward()
    _CASE.append((spec, x, wgt, cls.detach(), [sd[k].grad for k in order]))
    return _CASE[0]


def _worst(variant, ops=ref_ops):
    """Largest error of the walk over `ops` against the oracle: the class token and every gradient."""
    from hcir.vit_train import VitTrainer
    spec, x, wgt, cls0, g0 = _case()
    trainer = VitTrainer(spec, torch.device("cpu"), ops=ops, **variant)
    cls, saved = trainer.forward(x)
    grads = trainer.backward(saved, wgt)
    assert len(grads) == len(g0) == 4 + 12 * DEPTH + 2
    assert all(a.shape == b.shape == p.shape for a, b, p in zip(grads, g0, trainer.params()))
    rms = max((t.norm() / t.numel() ** 0.5).item() for t in g0)
    errs = [((cls - cls0).norm() / cls0.norm()).item()]
    errs += [((a - b).norm() / (b.norm() + 1e-3 * rms * b.numel() ** 0.5)).item() for a, b in zip(grads, g0)]
    return max(errs)


def _ids(v):
    return f"keep={int(v['keep_recomputable'])}-cls_only={int(v['cls_only_last'])}"


@pytest.mark.parametrize("variant", VARIANTS, ids=_ids)
def test_walk_is_the_vit(variant):
    worst = _worst(variant)
    print(f"{_ids(variant)}: walk vs autograd, worst error over the class token and gradients {worst:.3e}")
    assert worst <= TOL


def _wrapped(name, wrapper):
    """The stand-in ops with `name` replaced by wrapper(the real one)."""
    ops = types.SimpleNamespace(**{k: v for k, v in vars(ref_ops).items() if not k.startswith("__")})
    setattr(ops, name, wrapper(getattr(ref_ops, name)))
    return ops


def _proj_without_resid(gemm):
    def f(a, w, bias, rows, out, resid=None):          # proj: the square GEMM with a residual (fc2's is [D, mlp])
        gemm(a, w, bias, rows, out, None if w.shape[0] == w.shape[1] else resid)
    return f


def _ln_bwd_without_colsum(layernorm_bwd):
    def f(*args, dres_colsum=None, **kw):               # the fc2-bias (and proj-bias) handoff is lost
        layernorm_bwd(*args, **kw)
        if dres_colsum is not None:
            dres_colsum.zero_()
    return f


def _cls_bwd_without_kv(attn_cls_bwd):
    def f(qkv, out, d_out, lse, b, t, heads, scale, d_qkv):
        attn_cls_bwd(qkv, out, d_out, lse, b, t, heads, scale, d_qkv)
        d_qkv[: b * t].view(b, t, 3, heads, 64)[:, :, 1:] = 0
    return f


_MUTATIONS = {"proj_gemm_ignores_resid": ("gemm", _proj_without_resid, VARIANTS),
              "ln_bwd_leaves_colsum_zero": ("layernorm_bwd", _ln_bwd_without_colsum, VARIANTS),
              "cls_attn_bwd_zero_k_v": ("attn_cls_bwd", _cls_bwd_without_kv,
                                        [v for v in VARIANTS if v["cls_only_last"]])}


@pytest.mark.parametrize("mutation,variant", [(m, v) for m, (_, _, vs) in _MUTATIONS.items() for v in vs],
                         ids=lambda p: p if isinstance(p, str) else _ids(p))
def test_a_wiring_error_is_seen(mutation, variant):
    name, wrapper, _ = _MUTATIONS[mutation]
    worst = _worst(variant, _wrapped(name, wrapper))
    print(f"{mutation}, {_ids(variant)}: worst error {worst:.3e}")
    assert worst >= 1e6 * TOL


def test_default_ops_refuse_the_cpu():
    from hcir._lib import HcirError
    from hcir.vit_train import VitTrainer
    with pytest.raises(HcirError):
        VitTrainer(_case()[0], torch.device("cpu"))
