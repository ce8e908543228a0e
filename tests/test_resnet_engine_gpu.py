"""hcir.resnet_engine on the device: the ResNet-18 / ResNet-50 trunk on the HIP convolution kernels against the CPU
oracle (oracle.vit.resnet_trunk_forward), the opt-in `hip_trunk` switch of SHAM2 / SimCLR, cache invalidation, the
C1 shape and the CLI flag.  Embedding bar: 1 - cos <= 1e-3, the project's bar for every embedding path."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import knn as oknn
from oracle import transform as otf
from oracle import vit as ovit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _cos_err(a, b):
    return (1.0 - F.cosine_similarity(a.double(), b.double(), dim=-1)).abs().max().item()


def _randomize(model, seed):
    """As tests/test_paths_gpu.py::_randomize: random running statistics and affine parameters, so that a folded
    BatchNorm that drops a term cannot pass."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in list(model.named_parameters()) + list(model.named_buffers()):
            if not p.dtype.is_floating_point:
                continue
            if "running_var" in name:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() <= 1:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))


_MODELS = {}


def _model(name):
    """One randomised SHAM2 per trunk for the whole module (CPU state dict kept for the oracle)."""
    if name not in _MODELS:
        from hcir.main_backbone import SHAM2
        torch.manual_seed(42)
        m = SHAM2(name).eval()
        _randomize(m, 12)
        _randomize(m.backbone_momentum, 13)          # the twins differ
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        _MODELS[name] = (m.cuda(), sd)
    m, sd = _MODELS[name]
    m.eval()
    m.hip_trunk = True
    return m, sd


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
@pytest.mark.parametrize("b,size", [(2, 224), (3, 64)])
def test_hip_trunk_vs_oracle(name, b, size):
    m, sd = _model(name)
    x = torch.randn(b, 3, size, size, generator=torch.Generator().manual_seed(size))
    ref = ovit.sham2_extract_features(sd, x, name)
    with torch.no_grad():
        out = m.extract_features(x.cuda())
        ema = m.extract_features_ema(x.cuda())
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape)
    assert torch.isfinite(out).all()
    err = _cos_err(out.cpu(), ref)
    print(f"{name} B={b} {size}x{size}: 1 - cos = {err:.2e}")
    assert err <= 1e-3
    # the momentum twin has its own weights
    ref_ema = ovit.sham2_extract_features(sd, x, name, prefix="backbone_momentum.")
    assert _cos_err(ema.cpu(), ref_ema) <= 1e-3
    assert _cos_err(ref, ref_ema) > 1e-2, "the test's twins must differ"


def test_switch_off_is_inert_and_train_mode_bypasses():
    m, _ = _model("resnet18")
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    # both sides of every torch.equal below are the torch / MIOpen path: pin its algorithm choice (the first call of a
    # shape may pick another kernel than the later ones) so that the comparison is about the switch alone
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for _ in range(2):
            m.backbone(x), m.backbone_momentum(x)
        hip = m.extract_features(x)
        m.hip_trunk = False
        off = m.extract_features(x)
        assert torch.equal(off, m.backbone(x).flatten(1))
        assert torch.equal(m.extract_features_ema(x), m.backbone_momentum(x).flatten(1))
        assert torch.equal(m(x), m.projection_head(m.backbone(x).flatten(1)))
        assert not torch.equal(hip, off)          # fp16 NHWC kernels against fp32 MIOpen: close, never identical
        m.hip_trunk = True
        # CPU input: not on a HIP device, the torch path
        mc_in = x[:1].cpu()
        with pytest.raises(Exception):
            m.extract_features(mc_in)             # torch's own device-mismatch error: the engine was not entered
    # autograd on: torch path, differentiable
    g = m.extract_features(x)
    assert g.requires_grad
    # train mode: batch statistics, torch path even with the switch on
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    try:
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            m.backbone(x)
            m.load_state_dict(sd)
            a = m.extract_features(x)
            m.load_state_dict(sd)                 # undo the running-stat update, then the plain torch path again
            b = m.backbone(x).flatten(1)
        assert torch.equal(a, b)
    finally:
        m.load_state_dict(sd)
        m.eval()


@pytest.mark.parametrize("name,dim", [("resnet18", 128), ("resnet50", 1024)])
def test_forward_uses_trunk_and_hip_head(name, dim, monkeypatch):
    from hcir import resnet_engine
    from hcir.main_backbone import SimCLRProjectionHead
    m, sd = _model(name)
    used = []
    real_e, real_h = resnet_engine.ResNetEngine.forward, SimCLRProjectionHead.forward_hip
    monkeypatch.setattr(resnet_engine.ResNetEngine, "forward",
                        lambda self, x, l2_normalize=False: used.append("trunk") or real_e(self, x, l2_normalize))
    monkeypatch.setattr(SimCLRProjectionHead, "forward_hip", lambda self, x16: used.append("head") or real_h(self, x16))
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        z = m(x.cuda())
        zm = m.forward_momentum(x.cuda())
    assert used == ["trunk", "head", "trunk", "head"]
    ref = ovit.projection_head_forward(sd, ovit.sham2_extract_features(sd, x, name))
    refm = ovit.projection_head_forward(sd, ovit.sham2_extract_features(sd, x, name, "backbone_momentum."),
                                        prefix="projection_head_momentum.")
    assert tuple(z.shape) == (2, dim)
    e, em = _cos_err(z.cpu(), ref), _cos_err(zm.cpu(), refm)
    print(f"{name} forward / forward_momentum: 1 - cos = {e:.2e} / {em:.2e}")
    assert e <= 1e-3 and em <= 1e-3


def test_simclr_forward_with_hip_trunk():
    from hcir.backbone import SimCLR
    torch.manual_seed(7)
    m = SimCLR("resnet18").eval()
    _randomize(m, 4)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(8))
    ref = ovit.projection_head_forward(sd, ovit.sham2_extract_features(sd, x, "resnet18"))
    with torch.no_grad():
        off = m(x.cuda())
        m.hip_trunk = True
        on = m(x.cuda())
        feats = m.extract_features(x.cuda())
    assert tuple(on.shape) == (3, 128) and not torch.equal(on, off)
    assert _cos_err(on.cpu(), ref) <= 1e-3 and _cos_err(off.cpu(), ref) <= 1e-3
    assert _cos_err(feats.cpu(), ovit.sham2_extract_features(sd, x, "resnet18")) <= 1e-3


def test_inputs_the_kernels_do_not_take_keep_the_torch_path():
    """fp16 input on an fp16 model, and a 6 x 6 image: the switch is on, the call must not reach the engine."""
    from hcir import resnet_engine
    m, _ = _model("resnet18")

    def boom(self, x, l2_normalize=False):
        raise AssertionError("engine entered")

    x = torch.randn(2, 3, 6, 6, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setattr(resnet_engine.ResNetEngine, "forward", boom)
        a = m.extract_features(x)
        assert tuple(a.shape) == (2, 512)
        with torch.autocast("cuda", dtype=torch.float16):
            b = m.extract_features(torch.randn(2, 3, 32, 32, device="cuda"))
        assert tuple(b.shape) == (2, 512)


def test_load_state_dict_invalidates_the_cache():
    from hcir.backbone import SimCLR
    torch.manual_seed(5)
    m = SimCLR("resnet18").eval()
    _randomize(m, 1)
    sd1 = {k: v.clone() for k, v in m.state_dict().items()}
    torch.manual_seed(6)
    other = SimCLR("resnet18").eval()
    _randomize(other, 2)
    sd2 = {k: v.clone() for k, v in other.state_dict().items()}
    m = m.cuda()
    m.hip_trunk = True
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        a = m.extract_features(x.cuda())
        eng = m.trunk_engine("backbone", x.cuda().device)
        assert m.trunk_engine("backbone", x.cuda().device) is eng          # unchanged weights: no repack
        m.load_state_dict(sd2)
        b = m.extract_features(x.cuda())
    assert _cos_err(a.cpu(), ovit.sham2_extract_features(sd1, x, "resnet18")) <= 1e-3
    assert _cos_err(b.cpu(), ovit.sham2_extract_features(sd2, x, "resnet18")) <= 1e-3
    assert _cos_err(a.cpu(), b.cpu()) > 1e-2


def test_config_c1_resnet50_top5_hip_trunk(golden_dir):
    """The C1 shape of test_config_c1_resnet50_top5 with the engine on: 64 crops, ResNet-50 on the HIP trunk with the
    L2 normalisation in the avgpool kernel, top-5 over the seed-0 1000 x 2048 gallery."""
    from hcir import ops
    from hcir.resnet_engine import ResNetEngineCache
    m, sd = _model("resnet50")
    win = np.load(os.path.join(golden_dir, "asset_windows.npz"))["windows"]
    rng = np.random.default_rng(0)
    crops = [otf.window_to_tensor(w) for w in win]
    while len(crops) < 64:
        w = win[len(crops) % 4]
        dy, dx = rng.integers(0, 32, 2)
        crops.append(otf.window_to_tensor(np.roll(w, (dy, dx), (0, 1))[:, ::(-1) ** len(crops)]))
    x = torch.from_numpy(np.stack(crops))
    ref = ovit.classifier_embed(sd, x, "resnet50")
    g = F.normalize(torch.randn(1000, 2048, generator=torch.Generator().manual_seed(0)), dim=1)
    with torch.no_grad():
        eng = ResNetEngineCache().get(m.backbone, torch.device("cuda", torch.cuda.current_device()))
        emb = eng.forward(x.cuda(), l2_normalize=True)
        val, idx = ops.sim_topk(emb, g.cuda(), 5)
    assert ((emb.double().norm(dim=1) - 1).abs() <= 1e-6).all()
    err = _cos_err(emb.cpu(), ref)
    print(f"C1 resnet50 hip trunk: 1 - cos = {err:.2e}")
    assert err <= 1e-3
    rv, ri = oknn.cosine_topk(emb.cpu().numpy(), g.numpy(), 5)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(val.cpu().numpy(), rv)


def test_knn_cli_resnet_engine_flag(tmp_path, monkeypatch):
    """--resnet_engine hip on the synthetic folder of test_knn_cli_end_to_end: same output file, and the trunk really
    ran on the engine.  Without the flag the namespace is the one the reference flags give, plus the default."""
    import importlib.util
    from PIL import Image
    from hcir import resnet_engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "knn_cli_resnet_engine", os.path.join(root, "hair-centric-image-retrieval_amd", "knn_classification.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(0)
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    rows = {"train": [], "test": []}
    for split, n in (("train", 48), ("test", 12)):
        for i in range(n):
            cls = i % 3
            arr = rng.integers(0, 255, (240, 250, 3), dtype=np.uint8)
            arr[..., cls] = 255 - arr[..., cls] // 4
            name = f"{split}_{i}.png"
            Image.fromarray(arr).save(img_dir / name)
            rows[split].append(f"{name},{cls}")
    for split in rows:
        (tmp_path / f"{split}.csv").write_text("id,class\n" + "\n".join(rows[split]) + "\n")
    argv = ["--mode", "SHAM", "--model", "resnet18", "--eval_type", "knn", "--batch_size", "16",
            "--num_workers", "0", "--device", "cuda", "--save_path", str(tmp_path / "out"),
            "--train_annotation", str(tmp_path / "train.csv"),
            "--test_annotation", str(tmp_path / "test.csv"), "--img_dir", str(img_dir)]
    plain = vars(cli.parse_args(argv))
    args = cli.parse_args(argv + ["--resnet_engine", "hip"])
    assert plain.pop("resnet_engine") == "torch"
    with_flag = dict(vars(args))
    assert with_flag.pop("resnet_engine") == "hip" and with_flag == plain
    assert cli.build_model(cli.parse_args(argv)).hip_trunk is False

    calls = []
    real = resnet_engine.ResNetEngine.forward

    def counted(self, x, l2_normalize=False):
        calls.append(tuple(x.shape))
        return real(self, x, l2_normalize)

    monkeypatch.setattr(resnet_engine.ResNetEngine, "forward", counted)
    cli.set_seed(args.seed)
    with pytest.raises(ValueError, match="n_neighbors"):
        cli.main(args)
    assert len(calls) >= 3 + 1 and calls[0] == (16, 3, 224, 224)      # 48 train + 12 test images in batches of 16
    txt = (tmp_path / "out" / "SHAM_resnet18_embedding" / "knn_evaluation_results.txt").read_text()
    for k in (5, 10, 20, 27, 30, 40):
        assert f"Results for k={k}\n" in txt
    assert "Results for k=642" not in txt and "Confusion Matrix:" in txt
