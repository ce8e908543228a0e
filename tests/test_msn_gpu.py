"""hcir.backbone.MSN, hcir.losses.MSNLoss and MSNTrainStep on an MI355X against fp32 CPU autograd through the
restatement (tests/_msn_ref.py).

The model: a two-block torchvision-layout ViT with 4 heads of head dim 64 and patch 16, heads of hidden width 512 and
64 prototypes of width 256; 48 x 48 images (9 patches: the mask is drawn over 9 positions, 7 tokens kept) as target and
anchor views and two 32 x 32 focal views (a 3 -> 2 position grid, 3 tokens kept); batch 4.  The width is 256, not
the 128 first thought of: the training walk's weight-gradient GEMM (hcir_gemm_f16_tn) takes widths that are multiples
of 256, and a narrower model would test nothing of this path.

Ground truth G: fp32 CPU autograd through the restatement on the same inputs and masks.  e_ref: the restatement as
plain torch on the GPU under fp16 autocast (the reference's step).  e_hip: the path under test - the target branch on
the inference engine, the anchors through hcir.vit_train's class-token exit on the kept rows, the loss on
hcir_msn_targets / _fwd / _bwd.  The project's rule, per gradient tensor of the anchor branch (pos_embedding through
the interpolation, class_token, conv_proj and the anchor head among them) and for the loss:

    e_hip <= max(2 e_ref, 2^-11)          2^-11: one rounding of the fp16 operand format

Measured on an MI355X: backbone tensors e_ref 1.1e-2 .. 1.6e-2, e_hip 1.3e-2 .. 1.7e-2; head tensors e_ref 1.7e-3 ..
1.4e-2, e_hip 2.5e-3 .. 1.6e-2; loss e_ref 9.2e-5, e_hip 3.7e-6.  encoder.ln.bias is zero in exact arithmetic (the
head's first BatchNorm removes a constant added to every class token): both sides hold rounding noise only there.
"""
import copy

import numpy as np
import pytest
import torch

import _msn_ref as mr
from _fp64 import rel

pytestmark = pytest.mark.gpu

HEADS, DIM, HIDDEN, OUT, PROTOS, B, SCALE = 4, 256, 512, 256, 64, 4, 1024.0
ONE_ROUNDING = 2.0 ** -11


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _new_model(seed=3):
    from hcir import _tv_vit
    from hcir.backbone import MSN
    torch.manual_seed(seed)
    vit = _tv_vit.TVVisionTransformer(image_size=48, patch_size=16, num_layers=2, num_heads=HEADS, hidden_dim=DIM,
                                      mlp_dim=2 * DIM)
    m = MSN(vit, hidden_dim=HIDDEN, output_dim=OUT, num_prototypes=PROTOS)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for part in (m.anchor_backbone, m.anchor_projection_head):
            for n, p in part.named_parameters():
                if "heads.head" in n:
                    continue
                if n.endswith(("ln_1.weight", "ln_2.weight", "ln.weight")) or (p.dim() == 1 and n.endswith("weight")):
                    p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
                elif p.dim() == 1:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
        for p in (m.anchor_backbone.vit.class_token, m.anchor_backbone.vit.encoder.pos_embedding):
            p.copy_(0.3 * torch.randn(p.shape, generator=g))
        # the target pair lags the anchor pair, as after some steps
        for part, twin in ((m.anchor_backbone, m.backbone), (m.anchor_projection_head, m.projection_head)):
            for p, e in zip(part.parameters(), twin.parameters()):
                e.copy_(p + 0.01 * torch.randn(p.shape, generator=g) * p.abs().mean())
    return m.train()


def _inputs(seed=8):
    import _mim_ref as mim
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(B, 3, 48, 48, generator=g)
    views = [big + 0.2 * torch.randn(B, 3, 48, 48, generator=g), big + 0.2 * torch.randn(B, 3, 48, 48, generator=g)]
    views += [torch.randn(B, 3, 32, 32, generator=g), torch.randn(B, 3, 32, 32, generator=g)]
    keep_a, _ = mim.random_token_mask(torch.rand(B, 9, generator=g), 0.15)
    keep_f, _ = mim.random_token_mask(torch.rand(2 * B, 4, generator=g), 0.15)
    assert keep_a.shape == (B, 7) and keep_f.shape == (2 * B, 3)
    return views, (keep_a.contiguous(), keep_f.contiguous())


_ANCHOR = ("anchor_backbone.", "anchor_projection_head.")
# containers the reference's checkpoints carry and its forward never reads: torchvision's classification head, and the
# mask token (MSN drops masked tokens, it does not replace them)
_UNUSED = ("heads.head.weight", "heads.head.bias", "mask_token")
_RESULTS = {}


def _results():
    if _RESULTS:
        return _RESULTS
    from hcir.losses import MSNLoss
    m = _new_model()
    views, keeps = _inputs()
    names = [n for n, _ in m.named_parameters() if n.startswith(_ANCHOR) and not n.endswith(_UNUSED)]

    def leaves(device):
        sd = {k: v.detach().clone().to(device) for k, v in m.state_dict().items()}
        for n in names:
            sd[n].requires_grad_(True)
        return sd

    # G: fp32 CPU autograd through the restatement
    sd = leaves("cpu")
    loss, _, _ = mr.msn_step_loss(sd, views, keeps, HEADS)
    (loss * SCALE).backward()
    G = ({n: sd[n].grad.double() for n in names}, loss.detach().double().reshape(1))

    # e_ref: the same restatement as plain torch on the GPU under fp16 autocast
    sd = leaves("cuda")
    cv, ck = [v.cuda() for v in views], [k.cuda() for k in keeps]
    with torch.autocast("cuda", dtype=torch.float16):
        with torch.no_grad():
            tgt = mr.projection_head(sd, mr.masked_vit_cls(sd, cv[0], None, HEADS, "backbone.vit."), "projection_head.")
        a1 = mr.projection_head(sd, mr.masked_vit_cls(sd, cv[1], ck[0], HEADS))
        a2 = mr.projection_head(sd, mr.masked_vit_cls(sd, torch.cat(cv[2:], 0), ck[1], HEADS))
        loss = mr.msn_loss_torch(torch.cat([a1, a2], 0), tgt, sd["prototypes"].detach())
    (loss * SCALE).backward()
    REF = ({n: sd[n].grad.detach().cpu().double() for n in names}, loss.detach().cpu().double().reshape(1))

    # e_hip: the path under test, as MSNTrainStep composes it, with the same masks
    hip = copy.deepcopy(m).cuda().train()
    with torch.autocast("cuda", dtype=torch.float16):
        tgt = hip(cv[0])
        a1 = hip.forward_masked(cv[1], ck[0])
        a2 = hip.forward_masked(torch.cat(cv[2:], 0), ck[1])
    assert not tgt.requires_grad and a1.requires_grad and tuple(a2.shape) == (2 * B, OUT)
    loss = MSNLoss()(torch.cat([a1, a2], 0).float(), tgt.float(), hip.prototypes.data)
    (loss * SCALE).backward()
    HIP = ({n: p.grad.detach().cpu().double() for n, p in hip.named_parameters() if n in names},
           loss.detach().cpu().double().reshape(1))
    none = [n for n, p in hip.named_parameters() if n not in names and p.grad is not None]
    _RESULTS.update(G=G, REF=REF, HIP=HIP, names=names, none=none, model=m, hip=hip, views=cv, keeps=ck)
    return _RESULTS


def test_anchor_gradients_and_loss_vs_cpu_autograd():
    r = _results()
    (g64, l64), (g_ref, l_ref), (g_hip, l_hip) = r["G"], r["REF"], r["HIP"]
    assert set(g_hip) == set(g64) == set(r["names"]) and all(torch.isfinite(v).all() for v in g_hip.values())
    for must in ("anchor_backbone.vit.encoder.pos_embedding", "anchor_backbone.vit.class_token",
                 "anchor_backbone.vit.conv_proj.weight", "anchor_projection_head.layers.6.bias",
                 "anchor_projection_head.layers.0.weight"):
        assert must in g_hip and float(g64[must].norm()) > 0
    rows = [(n, rel(g_ref[n], g64[n]), rel(g_hip[n], g64[n])) for n in r["names"]]
    rows.append(("loss", rel(l_ref, l64), rel(l_hip, l64)))
    for n, e_ref, e_hip in rows:
        print(f"  {n}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    for n, e_ref, e_hip in rows:
        assert e_hip <= max(2.0 * e_ref, ONE_ROUNDING), f"{n}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}"


def test_target_branch_and_prototypes_have_no_gradient():
    r = _results()
    assert r["none"] == []
    hip = r["hip"]
    assert hip.prototypes.grad is None and hip.prototypes.requires_grad
    assert all(p.grad is None for part in (hip.backbone, hip.projection_head) for p in part.parameters())
    assert hip.anchor_backbone.vit.heads.head.weight.grad is None and hip.anchor_backbone.mask_token.grad is None


def test_class_token_exit_without_keep_is_the_bits_it_was():
    """At the stored grid, vit_cls_with_grad with its new arguments at their defaults, with idx_keep=None spelled out,
    and with interpolation allowed but not needed gives the same class tokens and the same gradients, bit for bit."""
    from hcir.vit_train import vit_cls_with_grad
    r = _results()
    hip, x = r["hip"], r["views"][1]
    tr = hip.trainer(x.device)
    outs = []
    for kw in ({}, dict(idx_keep=None), dict(idx_keep=None, interpolate_pos=True)):
        hip.zero_grad()
        cls = vit_cls_with_grad(tr, x, **kw)
        cls.square().sum().backward()
        outs.append((cls.detach().clone(), [p.grad.detach().clone() for p in tr.params()]))
    for cls, grads in outs[1:]:
        assert torch.equal(cls.view(torch.int32), outs[0][0].view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads, outs[0][1]))
    # every token kept, in order: the kept-rows stream is the whole stream
    hip.zero_grad()
    every = torch.arange(10, device=x.device).repeat(B, 1)
    cls = vit_cls_with_grad(tr, x, every)
    assert torch.equal(cls.detach().view(torch.int32), outs[0][0].view(torch.int32))
    hip.zero_grad()


def test_one_train_step():
    """One MSNTrainStep with a GradScaler: the anchor parameters move, the target parameters are exactly the EMA of
    the previous anchors, the prototypes stay bit-equal."""
    from hcir.pretrain_engine import MSNTrainStep
    model = _new_model(seed=5).cuda()
    views, _ = _inputs(seed=9)
    views = [v.cuda() for v in views]
    anchors = [p for part in (model.anchor_backbone, model.anchor_projection_head) for p in part.parameters()]
    pairs = [(model.anchor_backbone, model.backbone), (model.anchor_projection_head, model.projection_head)]
    mom = 0.996
    m32, o32 = float(np.float32(mom)), float(np.float32(1.0 - mom))
    want = [e.data * m32 + p.data * o32 for a, c in pairs for p, e in zip(a.parameters(), c.parameters())]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    protos = model.prototypes.detach().clone()
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
    step = MSNTrainStep(model, torch.optim.Adam(model.parameters(), lr=1e-3), scaler)
    out = step(views)
    assert set(out) == {"loss"} and np.isfinite(out["loss"]) and 0 < out["loss"] < 20
    assert scaler.get_scale() == 256.0                    # no overflow: the optimizer step was taken
    for n, p in model.named_parameters():
        if n.startswith(_ANCHOR) and not n.endswith(_UNUSED):
            assert not torch.equal(p.detach(), before[n]), n
        assert p.grad is None or not p.grad.any(), n     # zero_grad closes the step
    ema = [e for a, c in pairs for e in c.parameters()]
    for e, w in zip(ema, want):
        assert torch.equal(e.data, w)
    assert torch.equal(model.prototypes.detach(), protos)
    out2 = step({"anchor": views[0], "pos1": views[1]})     # no focal views: the second call is skipped
    assert np.isfinite(out2["loss"])


def test_knn_cli_model_extracts_the_target_class_token():
    """knn_classification.build_model --mode MSN: extract_features is the target branch's class token."""
    import knn_classification as cli
    from hcir.backbone import MSN, _tv_spec
    from hcir.vit_engine import VitEngine
    model = cli.build_model(cli.parse_args(["--mode", "MSN", "--model", "vit_b_16"]))
    assert isinstance(model, MSN)
    model = model.cuda().eval()
    with torch.no_grad():
        model.backbone.vit.class_token.add_(0.5)           # the target and the anchor branch now differ
    x = torch.randn(2, 3, 224, 224, device="cuda")
    feats = model.extract_features(x)
    assert feats.shape == (2, 768) and not feats.requires_grad
    eng = VitEngine(_tv_spec(model.backbone.vit), x.device)
    want = eng.cls_embedding(eng.forward_tokens(x, cls_only_last=True), final_norm=True, l2_normalize=False)
    assert torch.equal(feats.view(torch.int32), want.view(torch.int32))
    other = VitEngine(_tv_spec(model.anchor_backbone.vit), x.device)
    assert not torch.equal(feats, other.cls_embedding(other.forward_tokens(x, cls_only_last=True), final_norm=True,
                                                      l2_normalize=False))
    small = _results()
    ref = mr.masked_vit_cls({k: v.detach().cpu() for k, v in small["model"].state_dict().items()},
                            small["views"][0].cpu(), None, HEADS, "backbone.vit.")
    got = small["hip"].extract_features(small["views"][0])
    cos = 1 - torch.nn.functional.cosine_similarity(got.cpu().double(), ref.double(), dim=1)
    assert cos.max() <= 1e-3
