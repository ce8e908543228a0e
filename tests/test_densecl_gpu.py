"""DenseCL on the device: NTXentLoss with its memory bank and select_most_similar as modules, the DenseCL model on the
HIP trunk paths against a float64 ground truth, and one whole DenseCLTrainStep.

The model (frame of tests/_resnet_train_frame.py: B = 4 at 64 x 64 on a ResNet-18 trunk with feature_dim = 512, and one
ResNet-50 case at B = 2).  Ground truth G: a float64 CPU copy of the model with the restated losses of
tests/_densecl_ref.py.  e_ref: torch under fp16 autocast on the GPU with every switch off and the losses composed in
torch (F.normalize, matmul, cross_entropy).  e_hip: the path under test - hip_train, hip_train_norm and hip_train_stem
on, the losses on hcir_ntxent_bank_fwd / _bwd.  Both device runs gather the key's local rows with the match indices of
G, so that a near-tie cannot turn rounding into an order-1 difference; the kernel's own indices are held to the
dense-match rule on the maps it read.  Criterion, the project's own (tests/_resnet_train_frame.py):

    every query-side gradient tensor and each of the three losses     e_hip <= max(2 e_ref, 1e-2)
    the concatenated gradient                                         e_hip <= 2 e_ref

Measured on an MI355X (e_hip is the same from run to run, e_ref moves in its second digit): ResNet-18, B = 4:
concatenated gradient e_ref 1.8e-1, e_hip 1.26e-1; losses (total, global, local) e_ref 5e-4 / 1e-3 / 3e-4, e_hip
1.5e-4 / 1.2e-4 / 2.8e-4.  ResNet-50, B = 2: 1.2 / 0.96 - its last stage normalises over 8 values per channel, and
both paths are at order 1 there; losses e_ref 1.4e-2 / 2.1e-2 / 1.2e-2, e_hip 1.9e-5 / 1.7e-2 / 5.1e-3.  The model's
maps have 4 positions per image (16 and 8 rows per case): no row was left to the match rule's weaker condition.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _densecl_ref as dr
from _fp64 import rel

pytestmark = pytest.mark.gpu

T, LAM, BANK_K, SCALE = 0.2, 0.5, 64, 1024.0
SWITCHES = ("hip_train", "hip_train_norm", "hip_train_stem")


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


# --------------------------------------------------------------------------------------------- loss module and queue
def test_ntxent_loss_with_bank_three_calls_and_a_wrap():
    """Three consecutive calls on a (24, 16) bank with 8 rows each - fill, fill, wrap - against the float64
    restatement and the CPU queue: loss, both gradients, bank contents and pointer after every call."""
    from hcir.losses import NTXentLoss
    torch.manual_seed(11)
    crit = NTXentLoss(0.2, memory_bank_size=(24, 16)).cuda()
    assert crit.bank.is_cuda and list(crit.state_dict()) == []
    bank64, ptr = crit.bank.detach().cpu().double(), 0
    g = torch.Generator().manual_seed(12)
    dtype = torch.float32
    for call in range(3):
        z0 = torch.randn(8, 16, generator=g)
        z1 = z0 + 0.5 * torch.randn(8, 16, generator=g)
        a0, a1 = z0.cuda().requires_grad_(True), z1.cuda().requires_grad_(True)
        before = crit.bank.detach().cpu().clone()
        loss = crit(a0, a1)
        loss.backward()
        ref = dr.bank_loss_f64(z0, z1, before, 0.2, full=True)
        d0, d1 = dr.bank_grads_f64(z0, z1, before, 0.2)
        u_in = dr.U_ROUND[dtype]
        assert dr.err_over_bound(loss.detach().cpu(), ref.loss, dr.loss_bound(ref, 0.2, dtype, u_in)) <= 1.0
        b0, b1 = dr.grad_bounds(ref, z0, z1, d0, d1, 0.2, 1.0, dtype, u_in)
        assert dr.err_over_bound(a0.grad.cpu(), d0, b0, dtype) <= 1.0
        assert dr.err_over_bound(a1.grad.cpu(), d1, b1, dtype) <= 1.0
        want, ptr = dr.enqueue(before.double(), ptr, ref.k)
        assert crit.bank_ptr == ptr == (8, 16, 0)[call]
        got = crit.bank.detach().cpu()
        rows = slice(8 * call, 8 * call + 8)
        assert dr.err_over_bound(got[rows], want[rows], dr.k_unit_bound(ref)) <= 1.0
        keep = torch.ones(24, dtype=torch.bool)
        keep[rows] = False
        assert torch.equal(got[keep], before[keep])          # every other row bit for bit as it was
    # no gradient, no update; a key without gradient leaves the query's gradient as it is
    with torch.no_grad():
        crit(a0.detach(), a1.detach())
    assert crit.bank_ptr == 0 and torch.equal(crit.bank.detach().cpu(), got)
    q = a0.detach().clone().requires_grad_(True)
    crit2 = NTXentLoss(0.2, memory_bank_size=(24, 16)).cuda()
    crit2.bank.copy_(before.cuda())
    crit2(q, a1.detach()).backward()
    assert torch.equal(q.grad, a0.grad)
    # overflow rows are dropped: 8 rows at ptr = 20 of 24 -> 4 fit, ptr = 0
    crit2.bank_ptr = 20
    old = crit2.bank.detach().clone()
    crit2(q, a1.detach())
    assert crit2.bank_ptr == 0 and torch.equal(crit2.bank[:20], old[:20]) and not torch.equal(crit2.bank[20:], old[20:])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_select_most_similar_module(dtype):
    """fp16 and fp32 inputs (fp32 rounded to fp16 once), with and without a y_values gradient."""
    from hcir.dense import dense_match, select_most_similar
    case = (3, 49, 49, 72, 16)
    x, y, vals = dr.match_inputs("relu", case, torch.float32)
    xd, yd = x.to(dtype).cuda(), y.to(dtype).cuda()              # fp16-representable either way
    idx, none = dense_match(xd, yd)
    assert none is None and idx.dtype == torch.int32
    ratio, wrong, weak = dr.match_verdict(idx.cpu(), x, y)
    assert ratio <= 1.0 and wrong == 0 and weak <= 0.10
    index = idx.long().unsqueeze(-1).expand(-1, -1, vals.shape[2])
    for vdt in (torch.float16, torch.float32):
        v = vals.to(vdt).cuda()
        out = select_most_similar(xd, yd, v)
        assert out.dtype == vdt and not out.requires_grad and torch.equal(out, torch.gather(v, 1, index))
        vg = v.clone().requires_grad_(True)
        outg = select_most_similar(xd.clone().requires_grad_(True), yd, vg)
        assert outg.requires_grad and torch.equal(outg.detach(), out)
        outg.sum().backward()
        counts = torch.zeros(v.shape[:2], device="cuda").scatter_add_(1, idx.long(), torch.ones(idx.shape, device="cuda"))
        assert torch.equal(vg.grad.float(), counts.unsqueeze(-1).expand_as(v).contiguous())


# ------------------------------------------------------------------------------------------------------- the model
def _new_model(name, seed=21):
    from hcir import _tv_resnet
    from hcir.backbone import DenseCL
    torch.manual_seed(seed)
    trunk = nn.Sequential(*list(getattr(_tv_resnet, name)(weights=None).children())[:-2])
    m = DenseCL(trunk, feature_dim=512 if name == "resnet18" else 2048)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in list(m.backbone.modules()) + list(m.backbone_momentum.modules()):
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
        for p, e in zip(m.projection_head_local.parameters(), m.projection_head_local_momentum.parameters()):
            e.add_(0.01 * torch.randn(e.shape, generator=g))
    return m.train()


def _query_grads(m):
    out = {}
    for part in ("backbone", "projection_head_global", "projection_head_local"):
        for n, p in getattr(m, part).named_parameters():
            out[f"{part}.{n}"] = p.grad.detach().cpu().double()
    return out


def _torch_bank_loss(q, k, bank, t):
    q, k = F.normalize(q, dim=1), F.normalize(k, dim=1)
    logits = torch.cat([(q * k).sum(1, keepdim=True), q @ bank.to(q.dtype).t()], 1) / t
    return F.cross_entropy(logits, torch.zeros(q.shape[0], dtype=torch.long, device=q.device))


_RESULTS = {}


def _results(name, b):
    if name in _RESULTS:
        return _RESULTS[name]
    from hcir import conv_train
    from hcir.dense import dense_match
    from hcir.losses import bank_criterion
    m = _new_model(name)
    gen = torch.Generator().manual_seed(5)
    xq = torch.randn(b, 3, 64, 64, generator=gen)
    xk = xq + 0.3 * torch.randn(b, 3, 64, 64, generator=gen)
    bank_g, bank_l = dr.make_bank(BANK_K, 512, seed=1), dr.make_bank(BANK_K, 512, seed=2)

    def finish(model, loss, lg, ll):
        for p in model.parameters():
            p.grad = None
        (loss * SCALE).backward()
        assert all(p.grad is None for part in (model.backbone_momentum, model.projection_head_global_momentum,
                                               model.projection_head_local_momentum) for p in part.parameters())
        losses = {k: v.detach().cpu().double().reshape(1) for k, v in (("loss", loss), ("global", lg), ("local", ll))}
        return _query_grads(model), losses

    # G: float64 on the CPU, the restated losses, its own match
    m64 = copy.deepcopy(m).double().train()
    qf, qg, ql = m64(xq.double())
    kf, kg, kl = m64.forward_momentum(xk.double())
    idx, kl_sel = dr.select_most_similar_f64(qf.detach(), kf, kl)
    lg = dr.bank_loss_f64(qg, kg, bank_g, T)
    ll = dr.bank_loss_f64(ql.flatten(end_dim=1), kl_sel.flatten(end_dim=1), bank_l, T)
    G = finish(m64, (1 - LAM) * lg + LAM * ll, lg, ll)
    index = idx.cuda().unsqueeze(-1).expand(-1, -1, 512)

    # e_ref: autocast, every switch off, torch losses; train_trunk_map must never be entered
    ref_m = copy.deepcopy(m).cuda().train()
    assert not any(getattr(ref_m, s) for s in SWITCHES)

    def forbidden(*a, **k):
        raise AssertionError("train_trunk_map entered with the switches off")

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(conv_train, "train_trunk_map", forbidden)
        with torch.autocast("cuda", dtype=torch.float16):
            qf, qg, ql = ref_m(xq.cuda())
            kf, kg, kl = ref_m.forward_momentum(xk.cuda())
            kl_sel = torch.gather(kl, 1, index)
            lg = _torch_bank_loss(qg, kg, bank_g.cuda(), T)
            ll = _torch_bank_loss(ql.flatten(end_dim=1), kl_sel.flatten(end_dim=1), bank_l.cuda(), T)
            loss = (1 - LAM) * lg + LAM * ll
        REF = finish(ref_m, loss, lg, ll)

    # e_hip: the three switches, our losses; the walk is entered once per trunk
    hip_m = copy.deepcopy(m).cuda().train()
    for s in SWITCHES:
        setattr(hip_m, s, True)
    entered, real = [], conv_train.train_trunk_map

    def spy(trunk, x, **kw):
        entered.append((len(list(trunk.children())), kw, torch.is_grad_enabled()))
        return real(trunk, x, **kw)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(conv_train, "train_trunk_map", spy)
        with torch.autocast("cuda", dtype=torch.float16):
            qf, qg, ql = hip_m(xq.cuda())
            kf, kg, kl = hip_m.forward_momentum(xk.cuda())
    assert entered == [(9, dict(fused_norm=True, fused_stem=True), True),
                       (9, dict(fused_norm=True, fused_stem=True), False)]
    assert qf.dtype == torch.float16 and qf.shape == (b, 4, 512 if name == "resnet18" else 2048) and qf.is_contiguous()
    hip_idx, _ = dense_match(qf, kf)
    verdict = dr.match_verdict(hip_idx.cpu(), qf.detach().cpu(), kf.cpu())
    kl_sel = torch.gather(kl, 1, index)
    lg, _ = bank_criterion(qg, kg, bank_g.cuda(), T)
    ll, _ = bank_criterion(ql.flatten(end_dim=1), kl_sel.flatten(end_dim=1), bank_l.cuda(), T)
    HIP = finish(hip_m, (1 - LAM) * lg + LAM * ll, lg, ll)
    nbt = [int(v) for part in (hip_m.backbone, hip_m.backbone_momentum) for n, v in part.named_buffers()
           if n.endswith("num_batches_tracked")]
    _RESULTS[name] = dict(G=G, REF=REF, HIP=HIP, verdict=verdict, nbt=nbt)
    return _RESULTS[name]


def _cat(d):
    return torch.cat([d[k].flatten() for k in sorted(d)])


@pytest.mark.parametrize("name,b", [("resnet18", 4), ("resnet50", 2)], ids=["resnet18-b4", "resnet50-b2"])
def test_model_gradients_and_losses_vs_f64(name, b):
    r = _results(name, b)
    (g64, l64), (g_ref, l_ref), (g_hip, l_hip) = r["G"], r["REF"], r["HIP"]
    assert set(g_hip) == set(g64) and all(torch.isfinite(v).all() for v in g_hip.values())
    e_ref_all, e_hip_all = rel(_cat(g_ref), _cat(g64)), rel(_cat(g_hip), _cat(g64))
    print(f"\n{name}: concatenated query-side gradient e_ref {e_ref_all:.3e} e_hip {e_hip_all:.3e}")
    rows = [(n, rel(g_ref[n], g64[n]), rel(g_hip[n], g64[n])) for n in g64] \
        + [(f"loss {n}", rel(l_ref[n], l64[n]), rel(l_hip[n], l64[n])) for n in l64]
    for n, e_ref, e_hip in rows:
        print(f"  {n}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip_all <= 2.0 * e_ref_all
    for n, e_ref, e_hip in rows:
        assert e_hip <= max(2.0 * e_ref, 1e-2), f"{n}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}"


@pytest.mark.parametrize("name,b", [("resnet18", 4), ("resnet50", 2)], ids=["resnet18-b4", "resnet50-b2"])
def test_model_match_indices_and_statistics(name, b):
    """The kernel's indices on the model's own fp16 maps obey the dense-match rule; every BatchNorm of the query and
    of the momentum trunk saw exactly one batch."""
    r = _results(name, b)
    ratio, wrong, weak = r["verdict"]
    print(f"\n{name}: match (max - chosen) / bound {ratio:.3f}, strict rows wrong {wrong}, weak rows {100 * weak:.1f} %")
    assert ratio <= 1.0 and wrong == 0 and weak <= 0.10
    assert r["nbt"] and all(v == 1 for v in r["nbt"])


def test_extract_features_on_the_engine():
    """hip_trunk: the eval-mode extract_features runs hcir.resnet_engine on the 8-child trunk's view."""
    m = _new_model("resnet18").cuda().eval()
    x = torch.randn(2, 3, 64, 64, device="cuda")
    with torch.no_grad():
        want = m.extract_features(x)
        m.hip_trunk = True
        got = m.extract_features(x)
    assert got.shape == (2, 512) and rel(got, want) <= 1e-2 and not torch.equal(got, want)
    assert list(m.state_dict()) == list(_new_model("resnet18").state_dict())


# ----------------------------------------------------------------------------------------------------- one whole step
def test_one_train_step():
    """DenseCLTrainStep with a GradScaler at B = 8, 64 x 64, ResNet-18, every switch on."""
    from hcir.pretrain_engine import DenseCLTrainStep
    model = _new_model("resnet18", seed=9).cuda()
    for s in SWITCHES:
        setattr(model, s, True)
    query = [p for part in (model.backbone, model.projection_head_global, model.projection_head_local)
             for p in part.parameters()]
    opt = torch.optim.Adam(query, lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
    gen = torch.Generator().manual_seed(1)
    xq = torch.randn(8, 3, 64, 64, generator=gen)
    batch = {"x_query": xq.cuda(), "x_key": (xq + 0.3 * torch.randn(8, 3, 64, 64, generator=gen)).cuda()}
    pairs = [(model.backbone, model.backbone_momentum),
             (model.projection_head_global, model.projection_head_global_momentum),
             (model.projection_head_local, model.projection_head_local_momentum)]
    mom = 0.99
    want = [e.data * mom + p.data * (1.0 - mom) for a, c in pairs for p, e in zip(a.parameters(), c.parameters())]
    before = [p.detach().clone() for p in query]
    step = DenseCLTrainStep(model, opt, scaler)
    assert step.criterion_global.bank.shape == (4096, 512)
    out = step(batch, momentum=mom, epoch=0, batch_id=0)
    assert set(out) == {"loss", "loss_global", "loss_local"} and all(np.isfinite(v) for v in out.values())
    assert abs(out["loss"] - 0.5 * (out["loss_global"] + out["loss_local"])) <= 1e-5 * abs(out["loss"])
    assert scaler.get_scale() == 256.0                    # no overflow: the optimizer step was taken
    for p, old in zip(query, before):
        assert not torch.equal(p.detach(), old)
    ema = [e for a, c in pairs for e in c.parameters()]
    for e, w in zip(ema, want):
        assert torch.equal(e.data, w) and e.grad is None   # the EMA expression bit for bit, and never a gradient
    assert step.criterion_global.bank_ptr == 8 and step.criterion_local.bank_ptr == 8 * 4
    assert step.criterion_global.bank.is_cuda
    out2 = step(batch, momentum=mom)
    assert np.isfinite(out2["loss"]) and step.criterion_global.bank_ptr == 16 and step.criterion_local.bank_ptr == 64


def test_train_from_files_cli_densecl(tmp_path, monkeypatch, capsys):
    """tools/train_from_files.py --mode densecl --hip-train-stem --hip-train-norm, the command itself: three steps
    of a ResNet-18 trunk on sixteen PNG files, hcir.optim.Adam's plain step under torch's GradScaler."""
    import os
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(0)
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    rows = []
    for i in range(16):
        Image.fromarray(rng.integers(0, 255, (240, 250, 3), dtype=np.uint8)).save(img_dir / f"im_{i}.png")
        rows.append(f"im_{i}.png,{i % 3}")
    (tmp_path / "train.csv").write_text("id,class\n" + "\n".join(rows) + "\n")
    monkeypatch.syspath_prepend(os.path.join(root, "tools"))
    import train_from_files
    monkeypatch.setattr(sys, "argv", ["train_from_files.py", "--csv", str(tmp_path / "train.csv"), "--img-dir",
                                      str(img_dir), "--batch-size", "4", "--workers", "0", "--mode", "densecl",
                                      "--model", "resnet18", "--hip-train-stem", "--hip-train-norm", "--max-steps", "3"])
    train_from_files.main()
    torch.cuda.synchronize()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert [ln.split(":")[0] for ln in lines] == ["step 0", "step 1", "step 2"]
    for ln in lines:
        vals = dict(kv.split("=") for kv in ln.split(": ", 1)[1].split())
        assert set(vals) == {"loss", "loss_global", "loss_local"} and all(np.isfinite(float(v)) for v in vals.values())
