"""MSN without a GPU: the float64 restatement of lightly's MSNLoss (tests/_msn_ref.py) pinned to torch's own ops and
to its closed-form backward, with six mutations that the device test's bounds must see on its own table of cases; the
wiring of the masked class-token walk (hcir.vit_train.VitTrainer.forward(x, keep=, interpolate_pos=)) against torch's
autograd through the restatement, both in float64 over stand-in ops (tests/_mae_walk_ref.py), with mutations; the
position interpolation and its gradient against F.interpolate under autograd; the model's state-dict keys (recorded
under tests/golden/), frozen and trainable sets and the mask quirk; MSNTrainStep; the refusals; the ABI; the CLIs.

The walk's case: dim 256, 4 heads (head_dim 64), mlp 512, depth 2, patch 16, a stored 3 x 3 position grid (48 x 48
images, 10 tokens, 7 kept) and 32 x 32 focal views (a 2 x 2 grid interpolated from the stored one, 5 tokens, 3 kept),
batch 4.  Both sides are float64 and differ only in summation order; TOL is that of tests/test_mae_host.py."""
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mae_walk_ref as ref_ops
import _msn_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


# ---------------------------------------------------------------------------------------------------------------
# the loss: restatement, closed forms, mutations
# ---------------------------------------------------------------------------------------------------------------
_TABLE = mr.table()
_IDS = ["-".join(str(x) for x in c) + f"-{f}-it{it}-w{w}" for c, f, it, w in _TABLE]
_REF = {}


def _ref(entry):
    """(inputs, restatement, autograd gradient, fp32 bounds) of one table entry, computed once and left unchanged."""
    if entry not in _REF:
        case, family, it, w = entry
        a, t, c = mr.make_inputs(case, family, torch.float32)
        ref = mr.msn_f64(a, t, c, iterations=it, weight=w)
        g = mr.grads_f64(a, t, c, iterations=it, weight=w)
        _REF[entry] = (a, t, c, ref, g, mr.bounds(ref, a, t, torch.float32, iterations=it, weight=w))
    return _REF[entry]


@pytest.mark.parametrize("entry", _TABLE, ids=_IDS)
def test_restatement_is_lightlys_formula_and_its_closed_forms(entry):
    """The loss equals the literal lightly formula, the closed-form gradient equals autograd, the single-softmax form
    of the sharpened targets equals softmax ** (1 / Ts) renormalised; every value is finite and no target degenerate."""
    case, family, it, w = entry
    a, t, c, ref, g, _ = _ref(entry)
    lit = mr.msn_literal_f64(a, t, c, iterations=it, weight=w)
    assert abs(float(ref.loss - lit)) <= 1e-13 * max(1.0, abs(float(lit)))   # weight 0: lightly skips the regulariser
    cf = mr.closed_form_grad(ref, a, weight=w)
    assert torch.isfinite(g).all() and torch.isfinite(ref.q).all()
    scale = g.abs().max()
    assert float((cf - g).abs().max() / scale) <= 1e-13
    sharp = torch.softmax(ref.st * mr.TS_DEFAULT, 1) ** (1.0 / mr.TS_DEFAULT)
    sharp = sharp / sharp.sum(1, keepdim=True)
    assert float(((sharp - ref.q0).abs() / ref.q0.clamp_min(1e-300)).max()) <= 1e-9
    assert float(ref.q.max()) < 1.0 and float(ref.pbar.min()) > 0.0 and float(ref.q.sum(1).sub(1).abs().max()) < 1e-12
    if it > 0:                                            # Sinkhorn as two scaling vectors, the kernel's form
        b, k = ref.q0.shape
        v = torch.ones(b, dtype=torch.float64)
        for _ in range(it):
            u = 1.0 / (k * (ref.q0 * v[:, None]).sum(0))
            v = 1.0 / (b * (ref.q0 * u[None, :]).sum(1))
        q = ref.q0 * u[None, :]
        q = q / q.sum(1, keepdim=True)
        assert float(((q - ref.q).abs() / ref.q.clamp_min(1e-300)).max()) <= 1e-9


def _applies(mutation, entry):
    (b, v, k, d), family, it, w = entry
    return {"prototype_unnormalised": family == "scaled",          # unit prototypes hide it
            "sinkhorn_step_dropped": it > 0,
            "wrong_pairing": b > 1 and v > 1}.get(mutation, True)


@pytest.mark.parametrize("mutation", mr.MUTATIONS)
def test_a_mutation_is_seen_on_the_device_tests_table(mutation):
    """Each mistake moves at least one compared quantity past the device test's own fp32 bound, on EVERY entry of the
    device test's table it can show on (an unnormalised prototype only where the prototypes are not unit rows, a
    dropped Sinkhorn step only with iterations, a wrong pairing only with more than one target and view)."""
    hit = 0
    for entry in _TABLE:
        if not _applies(mutation, entry):
            continue
        case, family, it, w = entry
        a, t, c, ref, g, bd = _ref(entry)
        bad = mr.msn_f64(a, t, c, iterations=it, weight=w, mutation=mutation)
        gbad = mr.grads_f64(a, t, c, iterations=it, weight=w, mutation=mutation)
        out = {"q": bad.q, "row_lse": bad.lse, "pbar": bad.pbar, "ce": bad.ce, "reg": bad.reg, "loss": bad.loss,
               "danchors": gbad}
        r = mr.verdicts(out, ref, bd, g, torch.float32)
        assert max(r.values()) > 1.0, (mutation, entry, r)
        hit += 1
    assert hit >= 4, (mutation, hit)


def test_bounds_are_ordered_by_format():
    """The bound of every quantity grows from fp32 to fp16 to bf16 and is positive."""
    entry = _TABLE[0]
    a, t, c, ref, g, b32 = _ref(entry)
    b16 = mr.bounds(ref, a, t, torch.float16, iterations=entry[2], weight=entry[3])
    bbf = mr.bounds(ref, a, t, torch.bfloat16, iterations=entry[2], weight=entry[3])
    for lo, hi in ((b32, b16), (b16, bbf)):
        for x, y in zip(lo, hi):
            assert bool((x > 0).all()) and bool((y >= x).all())


def test_refusals():
    from hcir.losses import MSNLoss
    with pytest.raises(NotImplementedError, match="never enabled by the reference"):
        MSNLoss(gather_distributed=True)
    with pytest.raises(ValueError):
        MSNLoss(temperature=0.0)
    with pytest.raises(ValueError):
        MSNLoss(sinkhorn_iterations=-1)
    crit = MSNLoss()
    assert (crit.temperature, crit.sinkhorn_iterations, crit.regularization_weight) == (0.1, 3, 1.0)
    a, t = torch.zeros(6, 8, requires_grad=True), torch.zeros(3, 8)
    with pytest.raises(NotImplementedError, match="never used by the reference"):
        crit(a, t, torch.nn.Parameter(torch.zeros(16, 8)))
    with pytest.raises(ValueError):
        crit(torch.zeros(7, 8), t, torch.zeros(16, 8))
    from hcir import HcirError
    with pytest.raises(HcirError, match="no CPU fallback"):
        crit(a, t, torch.zeros(16, 8))


def test_abi_entries_match_the_loader():
    """The four hcir_msn_* entries of include/hcir.h: as many ctypes arguments as C parameters, pointers as void
    pointers, sizes as size_t, the 64-bit counts as int64."""
    import re
    from hcir import _lib
    hdr = open(os.path.join(ROOT, "include", "hcir.h")).read()
    kinds = {"int64_t": _lib.c_i64, "int32_t": _lib.c_i32, "int": _lib.c_int, "float": _lib.c_f32, "size_t": _lib.c_sz}
    found = 0
    for ret, name, args in re.findall(r"^(size_t|int)\s+(hcir_msn_[a-z_]+)\(([^;]*)\);", hdr, re.M):
        res, argtypes = _lib.SIGNATURES[name]
        assert res is (_lib.c_sz if ret == "size_t" else _lib.c_int)
        params = [" ".join(p.split()) for p in args.split(",")]
        assert len(params) == len(argtypes), name
        for p, ct in zip(params, argtypes):
            want = _lib.c_vp if "*" in p else kinds[p.replace("const ", "").split(" ")[0]]
            assert ct is want, (name, p)
        found += 1
    assert found == 4


# ---------------------------------------------------------------------------------------------------------------
# the masked class-token walk and the position interpolation
# ---------------------------------------------------------------------------------------------------------------
DIM, HEADS, MLP, DEPTH, PATCH, GRID0, B = 256, 4, 512, 2, 16, 3, 4
_LAYER_KEYS = (("ln1_w", "ln_1.weight"), ("ln1_b", "ln_1.bias"), ("qkv_w", "self_attention.in_proj_weight"),
               ("qkv_b", "self_attention.in_proj_bias"), ("proj_w", "self_attention.out_proj.weight"),
               ("proj_b", "self_attention.out_proj.bias"), ("ln2_w", "ln_2.weight"), ("ln2_b", "ln_2.bias"),
               ("fc1_w", "mlp.0.weight"), ("fc1_b", "mlp.0.bias"), ("fc2_w", "mlp.3.weight"), ("fc2_b", "mlp.3.bias"))
_WALK = {}


def _walk_case(size):
    """The spec, images of side `size`, an idx_keep in lightly's form (token 0 first, the rest in random order) and the
    restatement's class tokens and gradients under a random cotangent, computed once."""
    if size in _WALK:
        return _WALK[size]
    from hcir.vit_engine import VitLayer, VitSpec
    g = torch.Generator().manual_seed(97)                 # the same parameters for both sizes
    r = lambda *s, scale=1.0: scale * torch.randn(*s, generator=g, dtype=torch.float64)
    w = lambda n, k: r(n, k, scale=k ** -0.5)

    def layer(d, mlp):
        gain, bias = lambda: 1.0 + r(d, scale=0.2), lambda n: r(n, scale=0.05)
        return VitLayer(ln1_w=gain(), ln1_b=bias(d), qkv_w=w(3 * d, d), qkv_b=bias(3 * d), proj_w=w(d, d),
                        proj_b=bias(d), ln2_w=gain(), ln2_b=bias(d), fc1_w=w(mlp, d), fc1_b=bias(mlp),
                        fc2_w=w(d, mlp), fc2_b=bias(d))
    layers = [layer(DIM, MLP) for _ in range(DEPTH)]
    pdim = 3 * PATCH * PATCH
    spec = VitSpec(patch=PATCH, dim=DIM, heads=HEADS, eps=1e-6, pos_mult=1.0,
                   conv_w=w(DIM, pdim).view(DIM, 3, PATCH, PATCH), conv_b=r(DIM, scale=0.05),
                   cls=r(1, 1, DIM, scale=0.02), pos=r(1, GRID0 * GRID0 + 1, DIM, scale=0.5), layers=layers,
                   final_ln_w=1.0 + r(DIM, scale=0.2), final_ln_b=r(DIM, scale=0.05))
    g2 = torch.Generator().manual_seed(size)
    x = torch.randn(B, 3, size, size, generator=g2, dtype=torch.float64)
    npatch = (size // PATCH) ** 2
    keep, _ = _random_keep(npatch, g2)
    wgt = torch.randn(B, DIM, generator=g2, dtype=torch.float64)
    leaf = lambda t: t.clone().requires_grad_(True)
    p = "anchor_backbone.vit."
    sd = {p + "conv_proj.weight": leaf(spec.conv_w), p + "conv_proj.bias": leaf(spec.conv_b),
          p + "class_token": leaf(spec.cls), p + "encoder.pos_embedding": leaf(spec.pos)}
    for i, l in enumerate(layers):
        for field, key in _LAYER_KEYS:
            sd[f"{p}encoder.layers.encoder_layer_{i}.{key}"] = leaf(getattr(l, field))
    sd[p + "encoder.ln.weight"], sd[p + "encoder.ln.bias"] = leaf(spec.final_ln_w), leaf(spec.final_ln_b)
    order = list(sd)                                      # the order of VitTrainer.params()
    out = {}
    for name, kp in (("keep", keep), ("full", None)):
        cls = mr.masked_vit_cls(sd, x, kp, HEADS)
        (cls * wgt).sum().backward()
        out[name] = (cls.detach(), [sd[k].grad.clone() for k in order])
        for k in order:
            sd[k].grad = None
    _WALK[size] = (spec, x, keep, wgt, out)
    return _WALK[size]


def _random_keep(npatch, g):
    """The reference's draw: lightly's random_token_mask over npatch positions (no slot for the class token)."""
    import _mim_ref as mim
    return mim.random_token_mask(torch.rand(B, npatch, generator=g), 0.15)


def _errors(cls, cls0, grads, g0):
    rms = max((t.norm() / t.numel() ** 0.5).item() for t in g0)
    errs = [((cls - cls0).norm() / cls0.norm()).item()]
    errs += [((a - b).norm() / (b.norm() + 1e-3 * rms * b.numel() ** 0.5)).item() for a, b in zip(grads, g0)]
    return max(errs)


def _walk_worst(size, which, cls_only_last, keep_recomputable=True, ops=ref_ops):
    from hcir.vit_train import VitTrainer
    spec, x, keep, wgt, out = _walk_case(size)
    cls0, g0 = out[which]
    tr = VitTrainer(spec, torch.device("cpu"), keep_recomputable=keep_recomputable, cls_only_last=cls_only_last, ops=ops)
    kp = keep.contiguous() if which == "keep" else None
    cls, saved = tr.forward(x, keep=kp, interpolate_pos=True)
    if which == "keep":
        assert saved.tb == keep.shape[1] and saved.t == (size // PATCH) ** 2 + 1
    grads = tr.backward(saved, wgt)
    assert len(grads) == len(g0) == 4 + 12 * DEPTH + 2
    assert all(a.shape == b.shape == p.shape for a, b, p in zip(grads, g0, tr.params()))
    return _errors(cls, cls0, grads, g0)


@pytest.mark.parametrize("keep_recomputable", [True, False], ids=["keep=1", "keep=0"])
@pytest.mark.parametrize("cls_only_last", [True, False], ids=["cls-rows", "all-rows"])
@pytest.mark.parametrize("size,which", [(48, "keep"), (32, "keep"), (32, "full")],
                         ids=["stored-grid-7-of-10", "focal-3-of-5", "focal-unmasked"])
def test_masked_class_token_walk(size, which, cls_only_last, keep_recomputable):
    """The class token and all 4 + 12 * depth + 2 gradients - pos_embedding through the interpolation included - on the
    kept rows of the stored grid (7 of 10 tokens) and of a focal view (3 of 5, the 3 x 3 table interpolated to 2 x 2),
    with the last block on all kept rows and on the class-token rows only (the class-token attention pair at t = 7
    and 3: `_row_set` holds for any stream length)."""
    worst = _walk_worst(size, which, cls_only_last, keep_recomputable)
    print(f"{size} {which} cls_only_last={cls_only_last} keep={keep_recomputable}: worst error {worst:.3e}")
    assert worst <= TOL


def test_kept_counts_of_the_walks_case():
    assert _walk_case(48)[2].shape == (B, 7) and _walk_case(32)[2].shape == (B, 3)
    for size in (48, 32):
        keep = _walk_case(size)[2]
        assert bool((keep[:, 0] == 0).all()) and int(keep.max()) < (size // PATCH) ** 2


def _wrapped(name, wrapper):
    ops = types.SimpleNamespace(**{k: v for k, v in vars(ref_ops).items() if not k.startswith("__")})
    setattr(ops, name, wrapper(getattr(ref_ops, name)))
    return ops


def _gather_rolled(gather):
    def f(tok, b, t, idx, out):                           # the class token is no longer the first kept row
        gather(tok, b, t, idx.roll(1, dims=1).contiguous(), out)
    return f


def _scatter_shifted(scatter):
    def f(comp, b, t, idx, dtok):                         # gradients land one token further
        scatter(comp, b, t, ((idx + 1) % t).contiguous(), dtok)
    return f


def _position_grid_transposed(embed):
    def f(x, ps, w16, bias, cls, pos, pos_mult, tok):     # rows and columns of the position grid swapped
        g = int(math.isqrt(pos.shape[0] - 1))
        grid = pos[1:].view(g, g, -1).transpose(0, 1).reshape(g * g, -1)
        embed(x, ps, w16, bias, cls, torch.cat((pos[:1], grid), 0).contiguous(), pos_mult, tok)
    return f


WALK_MUTATIONS = {"gather_rolled": ("mae_gather_rows", _gather_rolled),
                  "scatter_shifted": ("mae_scatter_rows", _scatter_shifted),
                  "position_grid_transposed": ("patch_embed", _position_grid_transposed)}


@pytest.mark.parametrize("size", [48, 32])
@pytest.mark.parametrize("mutation", sorted(WALK_MUTATIONS))
def test_a_walk_wiring_error_is_seen(mutation, size):
    worst = _walk_worst(size, "keep", True, ops=_wrapped(*WALK_MUTATIONS[mutation]))
    print(f"{mutation} at {size}: worst error {worst:.3e}")
    assert worst >= 1e6 * TOL


def test_without_interpolation_the_token_count_is_refused():
    from hcir import HcirError
    from hcir.vit_train import VitTrainer
    spec, x, keep, _, _ = _walk_case(32)
    tr = VitTrainer(spec, torch.device("cpu"), ops=ref_ops)
    with pytest.raises(HcirError, match="pos_embedding has 10"):
        tr.forward(x)
    with pytest.raises(HcirError, match="pos_embedding has 10"):
        tr.forward(x, keep=keep.contiguous())
    with pytest.raises(HcirError, match="square"):
        tr.forward(x[:, :, :, :16].contiguous(), interpolate_pos=True)


@pytest.mark.parametrize("g0,npatch", [(3, 4), (14, 36), (14, 9), (14, 196)])
def test_position_interpolation_and_its_gradient_are_f_interpolates(g0, npatch):
    """interpolate_pos_encoding and VitTrainer._pos_grad against F.interpolate under autograd, written out here."""
    from hcir.vit_train import interpolate_pos_encoding
    d = 8
    g = torch.Generator().manual_seed(g0 * 100 + npatch)
    pos = torch.randn(1, g0 * g0 + 1, d, generator=g, dtype=torch.float64, requires_grad=True)
    got = interpolate_pos_encoding(pos, npatch)
    if npatch == g0 * g0:
        assert got is pos
        return
    side = int(math.isqrt(npatch))
    grid = F.interpolate(pos[:, 1:].reshape(1, g0, g0, d).permute(0, 3, 1, 2), scale_factor=math.sqrt(npatch / g0 ** 2),
                         mode="bicubic")
    assert tuple(grid.shape) == (1, d, side, side)
    want = torch.cat((pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, npatch, d)), 1)
    assert torch.equal(got, want) and torch.equal(got[:, 0], pos[:, 0])
    assert torch.equal(mr.interpolate_pos_encoding(pos, npatch), want)
    cot = torch.randn(want.shape, generator=g, dtype=torch.float64)
    ref_grad, = torch.autograd.grad(want, pos, cot)
    stub = types.SimpleNamespace(spec=types.SimpleNamespace(pos=pos.detach()), ops=ref_ops, device=torch.device("cpu"))
    from hcir.vit_train import VitTrainer
    mine = VitTrainer._pos_grad(stub, cot.reshape(-1, d), npatch)
    assert mine.shape == pos.shape and float((mine - ref_grad).abs().max()) <= 1e-14
    assert float((mine[:, 0] - cot[:, 0]).abs().max()) == 0.0            # the class row passes through


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
_MODEL = []


def _model():
    if not _MODEL:
        from hcir._tv_vit import vit_b_16
        from hcir.backbone import MSN
        torch.manual_seed(5)
        _MODEL.append(MSN(vit_b_16()))
    return _MODEL[0]


def _recorded_keys():
    """tests/golden/msn_state_dict_keys.txt: `name shape` per line (2048x768; nothing for a 0-d tensor), written out
    by hand from the reference's class (HairPretraining/src/backbone.py:87-101 over torchvision's vit_b_16)."""
    out = {}
    with open(os.path.join(ROOT, "tests", "golden", "msn_state_dict_keys.txt")) as f:
        for line in f:
            parts = line.split()
            out[parts[0]] = tuple(int(s) for s in parts[1].split("x")) if len(parts) > 1 else ()
    return out


def _filled(want, value):
    """A state dict of the recorded shapes without their memory: every tensor is one expanded element."""
    return {k: torch.full((), value).expand(v) if v else torch.tensor(3) for k, v in want.items()}


def test_state_dict_keys_are_the_references():
    want = _recorded_keys()
    model = _model()
    have = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert len(want) == 335 and have == want, (set(have) ^ set(want))
    res = model.load_state_dict(_filled(want, 0.5), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(model.prototypes.detach()[3, 4]) == 0.5 and int(model.projection_head.layers[1].num_batches_tracked) == 3
    _MODEL.clear()


def test_frozen_and_trainable_sets():
    model = _model()
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert frozen and all(n.startswith(("backbone.", "projection_head.")) for n in frozen)
    assert trainable == {n for n, _ in model.named_parameters()
                         if n.startswith(("anchor_backbone.", "anchor_projection_head."))} | {"prototypes"}
    assert {"anchor_" + n for n in frozen} == trainable - {"prototypes"}
    assert model.mask_ratio == 0.15 and tuple(model.prototypes.shape) == (1024, 256)
    head = model.projection_head.layers
    assert [type(m).__name__ for m in head] == ["Linear", "BatchNorm1d", "GELU", "Linear", "BatchNorm1d", "GELU",
                                                "Linear"]
    assert head[0].bias is None and head[3].bias is None and head[6].bias is not None
    # the twins start as copies
    for (n, p), (m, q) in zip(model.backbone.named_parameters(), model.anchor_backbone.named_parameters()):
        assert n == m and torch.equal(p, q)


@pytest.mark.parametrize("size,tokens,kept", [(224, 197, 166), (96, 37, 30)])
def test_the_mask_quirk(size, tokens, kept):
    """The mask is drawn over (width // patch) ** 2 positions: index 0 always kept, the last token never, 166 of 197
    kept at 224 x 224 and 30 of 37 at 96 x 96."""
    model = _model()
    x = torch.zeros(16, 3, size, size)
    seen = set()
    for _ in range(4):
        keep = model._idx_keep(x, None)
        assert keep.shape == (16, kept) and keep.dtype == torch.int64 and bool((keep[:, 0] == 0).all())
        assert int(keep.max()) <= tokens - 2
        seen.update(keep.flatten().tolist())
    assert tokens - 1 not in seen and len(seen) == tokens - 1


def test_bad_idx_keep_raises_before_any_launch(monkeypatch):
    import hcir._lib as L
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("library call")))
    model = _model()
    x = torch.zeros(2, 3, 224, 224)
    ok = torch.stack([torch.arange(166), torch.arange(166)])
    dup = ok.clone()
    dup[1, 5] = 6
    for bad in (ok.int(), ok[:1], ok.reshape(-1), ok[:, :0], ok + 100, ok - 1, dup):
        with pytest.raises(ValueError):
            model.forward_masked(x, bad)


def test_train_step_runs_the_reference_sequence(monkeypatch):
    from hcir import pretrain_engine as pe
    calls = []
    monkeypatch.setattr(pe, "update_momentum", lambda src, dst, m: calls.append(("ema", src, dst, m)))
    w = torch.ones(1, requires_grad=True)

    class Model:
        anchor_backbone, backbone, anchor_projection_head, projection_head = "ab", "b", "ah", "h"
        prototypes = torch.nn.Parameter(torch.full((8, 4), 2.0))

        def train(self):
            calls.append("train")

        def __call__(self, x):
            calls.append(("target", tuple(x.shape), torch.is_autocast_enabled("cuda")))
            return torch.zeros(x.shape[0], 4)

        def forward_masked(self, x):
            calls.append(("masked", tuple(x.shape), torch.is_autocast_enabled("cuda")))
            return w * torch.ones(x.shape[0], 4)

    def criterion(anchors, targets, prototypes):
        calls.append(("loss", tuple(anchors.shape), tuple(targets.shape), prototypes.requires_grad,
                      anchors.dtype, torch.is_autocast_enabled("cuda")))
        return anchors.sum() / anchors.numel() * 2.0

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

    opt = torch.optim.SGD([w], lr=0.0)
    big, small = torch.zeros(2, 3, 48, 48), torch.zeros(2, 3, 32, 32)
    out = pe.MSNTrainStep(Model(), opt, Scaler(), criterion)([big, big + 1, small, small, small], epoch=1)
    amp = calls[3][2]
    assert calls == ["train", ("ema", "ab", "b", 0.996), ("ema", "ah", "h", 0.996), ("target", (2, 3, 48, 48), amp),
                     ("masked", (2, 3, 48, 48), amp), ("masked", (6, 3, 32, 32), amp),
                     ("loss", (8, 4), (2, 4), False, torch.float32, False), "scale", "step", "update"]
    assert out == {"loss": 2.0} and (w.grad is None or not w.grad.any())
    calls.clear()
    out = pe.MSNTrainStep(Model(), opt, None, criterion)({"anchor": big, "pos1": big})
    assert [c[0] if isinstance(c, tuple) else c for c in calls] == ["train", "ema", "ema", "target", "masked", "loss"]
    assert out == {"loss": 2.0}
    calls.clear()
    pe.MSNTrainStep(Model(), opt, None, criterion)({"anchor": big, "pos1": big, "focal": [small, small]})
    assert ("masked", (4, 3, 32, 32), amp) in calls
    with pytest.raises(ValueError):
        pe.MSNTrainStep(Model(), opt, None, criterion)([big])
    from hcir.losses import MSNLoss
    assert isinstance(pe.MSNTrainStep(Model(), opt).criterion, MSNLoss)


def test_clis_know_msn():
    import knn_classification as cli
    from hcir.backbone import MSN
    model = cli.build_model(cli.parse_args(["--mode", "MSN", "--model", "vit_b_16"]))
    assert isinstance(model, MSN)
    with pytest.raises(SystemExit) as e:
        cli.build_model(cli.parse_args(["--mode", "dinov2"]))
    assert "MSN" in str(e.value).split("built modes:")[1]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_from_files as tff
    a = tff.build_parser().parse_args(["--csv", "x.csv", "--img-dir", "d", "--mode", "msn"])
    assert a.mode == "msn" and a.model == "vit_b_16"
    assert "no focal views" in " ".join(tff.build_parser().format_help().split())


def test_cli_loads_a_reference_checkpoint(monkeypatch):
    """A trainer dict whose ['model_state_dict'] has the reference's keys (the recorded list) loads strictly."""
    import knn_classification as cli
    monkeypatch.setattr(torch, "load", lambda path, **kw: {"model_state_dict": _filled(_recorded_keys(), 0.25)})
    model = cli.build_model(cli.parse_args(["--mode", "MSN", "--model", "vit_b_16", "--checkpoint_path", "msn.pth"]))
    assert float(model.anchor_backbone.vit.encoder.ln.weight[0]) == 0.25
