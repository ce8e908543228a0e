"""GPU tests of the SimCLR training views (hcir.views, hcir.dataloader.collate_train_views): every comparison is
torch.equal on the fp32 output against live Pillow composed as torchvision / lightly compose it (tests/_simclr_ref.py)
under the same boxes and parameters."""
import io
import itertools
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _simclr_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMAS = [0.1, 0.15, 0.3, 0.45, 0.6, 0.8, 1.0, 1.25, 1.5, 1.75, 1.9, 2.0]
FACTOR_ENDS = [0.2, 1.8, 1.0, 0.999, 1.001]


@pytest.fixture(scope="module")
def views(hcir_built):
    if not torch.cuda.is_available():
        pytest.fail("needs a HIP device")
    from hcir import views as v
    return v


@pytest.fixture(scope="module")
def crops():
    rng = np.random.default_rng(21)
    return [rng.integers(0, 256, (224, 224, 3)).astype(np.uint8), ref.hair_like(rng, 224, 224)]


def plain(views, n=1, **kw):
    """n records that do nothing, with fields overridden."""
    base = dict(flip=0, jitter=0, order=[[0, 1, 2, 3]], brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, gray=0,
                blur=0, sigma=1.0)
    base.update(kw)
    p = views.make_view_params(**base)
    return np.repeat(p, n) if len(p) == 1 and n > 1 else p


def check_params(views, crops_u8, params):
    """crops_u8: list of [224, 224, 3] arrays, one per record."""
    dev = torch.from_numpy(np.stack(crops_u8)).cuda()
    got = views.apply_view_params(dev, params).cpu()
    for k, (a, p) in enumerate(zip(crops_u8, params)):
        want = torch.from_numpy(ref.to_tensor_normalize(ref.apply_u8(Image.fromarray(a), p)))
        assert torch.equal(got[k], want), f"record {k}: {p}: {(got[k] != want).sum().item()} values differ"


def test_identity_is_to_tensor_normalize(views, crops):
    check_params(views, crops, plain(views, 2))


def test_flip_and_gray(views, crops):
    check_params(views, crops * 3, np.concatenate([plain(views, 2, flip=1), plain(views, 2, gray=1),
                                                   plain(views, 2, flip=1, gray=1)]))


@pytest.mark.parametrize("op,field", [(0, "brightness"), (1, "contrast"), (2, "saturation"), (3, "hue")])
def test_each_jitter_op_alone_and_factor_extremes(views, crops, op, field):
    """One op with a factor, the other three at their neutral factor (blend with 1.0 and a hue shift of 0 are run, as
    torchvision runs them)."""
    rng = np.random.default_rng(op)
    if field == "hue":
        grid = [0.2, -0.2, 0.0, 0.5, -0.5, 1 / 255, -1 / 255] + list(rng.uniform(-0.2, 0.2, 5))
    else:
        grid = FACTOR_ENDS + [0.0, 3.0] + list(rng.uniform(0.2, 1.8, 5))
    order = [op] + [k for k in range(4) if k != op]
    params = np.concatenate([plain(views, 2, jitter=1, order=[order], **{field: np.float32(f)}) for f in grid])
    check_params(views, crops * len(grid), params)


def test_all_24_jitter_orders(views, crops):
    orders = np.array(list(itertools.permutations(range(4))), dtype=np.int32)
    g = torch.Generator().manual_seed(3)
    params = views.draw_view_params(24, g, cj_prob=1.0, hf_prob=0.0, random_gray_scale=0.0, gaussian_blur=0.0)
    params["order"] = orders
    extremes = plain(views, 24, jitter=1, order=orders, brightness=1.8, contrast=1.8, saturation=0.2, hue=-0.2)
    check_params(views, (crops * 24)[:48], np.concatenate([params, extremes]))


def test_blur_over_sigma_grid(views, crops):
    rng = np.random.default_rng(8)
    grid = SIGMAS + [float(v) for v in rng.uniform(0.1, 2.0, 8).astype(np.float32)]
    params = np.concatenate([plain(views, 2, blur=1, sigma=np.float32(s)) for s in grid])
    assert set(params["blur_r"]) == {0, 1}
    check_params(views, crops * len(grid), params)


def test_batch_of_256_mixed_views(views, crops):
    rng = np.random.default_rng(5)
    params = views.draw_view_params(256, torch.Generator().manual_seed(17))
    assert params["jitter"].any() and params["blur"].any() and params["gray"].any() and params["flip"].any()
    imgs = [crops[0], crops[1]] + [ref.hair_like(rng, 224, 224) if k % 2 else
                                   rng.integers(0, 256, (224, 224, 3)).astype(np.uint8) for k in range(6)]
    check_params(views, [imgs[k % 8] for k in range(256)], params)


def _check_views(views, arrays, boxes, params):
    """simclr_views over images of any sizes against the Pillow composition; boxes [2, B, 4], params [2, B]."""
    out = views.simclr_views([torch.from_numpy(a).cuda() for a in arrays], boxes=boxes, params=params)
    assert out["anchor"].shape == out["pos1"].shape == (len(arrays), 3, 224, 224)
    assert out["anchor"].dtype == torch.float32
    for v, key in enumerate(("anchor", "pos1")):
        got = out[key].cpu()
        for k, a in enumerate(arrays):
            want = torch.from_numpy(ref.view(Image.fromarray(a), boxes[v][k], params[v][k]))
            assert torch.equal(got[k], want), f"{key}[{k}] box {boxes[v][k]}: {(got[k] != want).sum().item()} differ"


def test_boxes_from_8_percent_to_full_non_square_sources(views):
    rng = np.random.default_rng(13)
    arrays = [rng.integers(0, 256, (301, 415, 3)).astype(np.uint8), ref.hair_like(rng, 640, 480),
              rng.integers(0, 256, (224, 224, 3)).astype(np.uint8), ref.hair_like(rng, 97, 350),
              rng.integers(0, 256, (1024, 1024, 3)).astype(np.uint8)]
    # anchor: the smallest box torchvision can draw (8 % of the area: upscaling for the small sources) in a corner;
    # pos1: the whole image
    small, full = [], []
    for k, a in enumerate(arrays):
        h, w = a.shape[:2]
        bh, bw = max(int(round(np.sqrt(0.08) * h)), 1), max(int(round(np.sqrt(0.08) * w)), 1)
        small.append(((h - bh) if k % 2 else 0, 0 if k % 2 else (w - bw), bh, bw))
        full.append((0, 0, h, w))
    boxes = np.array([small, full])
    g = torch.Generator().manual_seed(2)
    params = views.draw_view_params(2 * len(arrays), g).reshape(2, len(arrays))
    _check_views(views, arrays, boxes, params)
    # drawn boxes, one axis already 224 wide, odd sizes
    drawn = views.random_resized_crop_boxes([a.shape[:2] for a in arrays] * 2, g).reshape(2, len(arrays), 4)
    drawn[0][0] = (10, 100, 150, 224)
    drawn[1][0] = (3, 5, 224, 77)
    _check_views(views, arrays, drawn, params)


@pytest.fixture(scope="module")
def asset_files(golden_dir):
    z = np.load(os.path.join(golden_dir, "png_streams.npz"))
    names = [str(n) for n in z["names"]]
    return {n: z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes() for i, n in enumerate(names)
            if n.startswith("asset_")}


def test_the_four_asset_pngs(views, asset_files):
    assert len(asset_files) == 4
    arrays = [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in asset_files.values()]
    assert all(a.shape == (1024, 1024, 3) for a in arrays)
    g = torch.Generator().manual_seed(4)
    boxes = views.random_resized_crop_boxes([(1024, 1024)] * 8, g).reshape(2, 4, 4)
    params = views.draw_view_params(8, g, cj_prob=1.0, gaussian_blur=1.0).reshape(2, 4)
    _check_views(views, arrays, boxes, params)


def test_same_seed_same_views_and_anchor_differs_from_pos1(views):
    rng = np.random.default_rng(1)
    imgs = [torch.from_numpy(ref.hair_like(rng, 300, 260)).cuda() for _ in range(6)]
    a = views.simclr_views(imgs, torch.Generator().manual_seed(77))
    b = views.simclr_views(imgs, torch.Generator().manual_seed(77))
    c = views.simclr_views(imgs, torch.Generator().manual_seed(78))
    assert torch.equal(a["anchor"], b["anchor"]) and torch.equal(a["pos1"], b["pos1"])
    assert not torch.equal(a["anchor"], c["anchor"])
    assert not torch.equal(a["anchor"], a["pos1"])
    assert all(not torch.equal(a["anchor"][k], a["pos1"][k]) for k in range(6))
    t = views.SimCLRTransform(input_size=224, min_scale=0.5, generator=torch.Generator().manual_seed(77))
    d = t(imgs)
    assert d["anchor"].shape == (6, 3, 224, 224) and torch.isfinite(d["pos1"]).all()


def test_errors(views):
    from hcir import HcirError
    img = torch.zeros((64, 64, 3), dtype=torch.uint8)
    with pytest.raises(HcirError):
        views.simclr_views([img])                                   # a CPU tensor: no fallback
    with pytest.raises(HcirError):
        views.apply_view_params(torch.zeros((1, 224, 224, 3), dtype=torch.uint8), plain(views))
    with pytest.raises(ValueError):
        plain(views, brightness=-0.1)
    with pytest.raises(ValueError):
        plain(views, jitter=1, hue=0.7)
    bad = plain(views, 2)
    bad["contrast"][1] = -1.0                                        # a table edited behind make_view_params' back
    with pytest.raises(ValueError):
        views.apply_view_params(torch.zeros((2, 224, 224, 3), dtype=torch.uint8).cuda(), bad)
    with pytest.raises(ValueError):
        views.simclr_views([img.cuda()], boxes=np.array([[[0, 0, 65, 64]], [[0, 0, 64, 64]]]), params=plain(views, 2))


# ---- from files ----
def _write_dataset(tmp_path, files):
    with open(tmp_path / "ann.csv", "w") as f:
        f.write("id,class\n")
        for k, (name, data) in enumerate(files):
            (tmp_path / name).write_bytes(data)
            f.write(f"{name},{k % 3}\n")
    return str(tmp_path / "ann.csv"), str(tmp_path)


def _encode(a, fmt, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, fmt, **kw)
    return b.getvalue()


def _palette_png(a):
    b = io.BytesIO()
    Image.fromarray(a).quantize(64).save(b, "PNG")
    return b.getvalue()


def _decoded(data):
    """The reference's decode of a file: Image.open(path).convert('RGB')."""
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


def test_collate_train_views_from_files(views, asset_files, tmp_path):
    from hcir.dataloader import EncodedDataset, collate_train_views
    rng = np.random.default_rng(31)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from corrupt_streams import synth_jpeg_image
    files = [("a_hair.png", _encode(ref.hair_like(rng, 300, 260), "PNG")),
             ("b_hair.png", _encode(ref.hair_like(rng, 300, 260), "PNG")),
             ("c_face.jpg", _encode(np.asarray(synth_jpeg_image(rng, 256, 320)), "JPEG", quality=90, subsampling=2)),
             ("d_asset.png", next(iter(asset_files.values()))),
             ("e_palette.png", _palette_png(ref.hair_like(rng, 128, 160))),
             ("f_face444.jpg", _encode(np.asarray(synth_jpeg_image(rng, 231, 199)), "JPEG", quality=80, subsampling=0))]
    # a 16-bit PNG is outside the device decoder's subset: PIL decodes it on the host
    b16 = io.BytesIO()
    Image.fromarray(rng.integers(0, 65535, (240, 250)).astype(np.uint16)).save(b16, "PNG")
    files.append(("g_16bit.png", b16.getvalue()))
    ann, root = _write_dataset(tmp_path, files)
    ds = EncodedDataset(ann, root, return_names=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=len(files), shuffle=False, num_workers=0,
                                         collate_fn=collate_train_views)
    batch = next(iter(loader))
    assert batch.n == len(files) and batch.names == [n for n, _ in files]
    assert 6 in batch.host_images and torch.equal(batch.labels, torch.tensor([0, 1, 2, 0, 1, 2, 0]))
    arrays = [_decoded(d) for _, d in files]
    g = torch.Generator().manual_seed(9)
    boxes = views.random_resized_crop_boxes([a.shape[:2] for a in arrays] * 2, g).reshape(2, len(files), 4)
    params = views.draw_view_params(2 * len(files), g).reshape(2, len(files))
    out = batch.views("cuda", boxes=boxes, params=params)
    for v, key in enumerate(("anchor", "pos1")):
        got = out[key].cpu()
        for k, a in enumerate(arrays):
            want = torch.from_numpy(ref.view(Image.fromarray(a), boxes[v][k], params[v][k]))
            assert torch.equal(got[k], want), f"{key}[{k}] ({files[k][0]})"
    # drawn inside: the same generator state gives the same batch
    o1 = batch.views("cuda", generator=torch.Generator().manual_seed(3))
    o2 = batch.views("cuda", generator=torch.Generator().manual_seed(3))
    assert torch.equal(o1["anchor"], o2["anchor"]) and torch.equal(o1["pos1"], o2["pos1"])


def test_corrupt_files_raise_with_their_names(views, tmp_path):
    from hcir import HcirError
    from hcir.dataloader import EncodedDataset, collate_train_views
    from corrupt_streams import png_corrupt_cases
    rng = np.random.default_rng(41)
    good = _encode(ref.hair_like(rng, 200, 180), "PNG")
    # cut in the middle of the file: the chunk structure is broken
    ann, root = _write_dataset(tmp_path, [("good.png", good), ("cut.png", good[:len(good) // 2])])
    ds = EncodedDataset(ann, root, return_names=True)
    with pytest.raises(HcirError, match="cut.png"):
        collate_train_views([ds[0], ds[1]]).views("cuda")
    # a truncated zlib stream inside valid chunks (CRCs right): only the device decoder can notice
    z = np.load(os.path.join(ROOT, "tests", "golden", "png_streams.npz"))
    i = [str(n) for n in z["names"]].index("filter4_rgb")
    base = z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes()
    cases = png_corrupt_cases(base, rng)
    name, bad = next(iter(cases.items()))
    sub = tmp_path / "zlib"
    sub.mkdir()
    ann, root = _write_dataset(sub, [("fine.png", base), ("broken_stream.png", bad)])
    ds = EncodedDataset(ann, root, return_names=True)
    with pytest.raises(HcirError, match="broken_stream.png") as e:
        collate_train_views([ds[0], ds[1]]).views("cuda")
    assert "fine.png" not in str(e.value), name
    # without names the batch position is reported
    ds2 = EncodedDataset(ann, root)
    with pytest.raises(HcirError, match="batch position 1"):
        collate_train_views([ds2[0], ds2[1]]).views("cuda")


def test_one_train_step_on_views_from_files(views, tmp_path):
    """Plumbing only: a batch produced from files goes through SHAMTrainStep (online and momentum paths read the same
    tensors) and gives finite losses."""
    from hcir.dataloader import EncodedDataset, collate_train_views
    from hcir.main_backbone import SHAM2
    from hcir.pretrain_engine import SHAMTrainStep
    rng = np.random.default_rng(51)
    files = [(f"{k}_hair.png", _encode(ref.hair_like(rng, 256, 256), "PNG")) for k in range(8)]
    ann, root = _write_dataset(tmp_path, files)
    ds = EncodedDataset(ann, root, return_names=True)
    batch = collate_train_views([ds[k] for k in range(len(ds))]).views("cuda", torch.Generator().manual_seed(1))
    assert batch["anchor"].shape == batch["pos1"].shape == (8, 3, 224, 224)
    before = {k: v.clone() for k, v in batch.items()}
    torch.manual_seed(9)
    model = SHAM2("vit_b_16").cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    step = SHAMTrainStep(model, opt, torch.amp.GradScaler("cuda", init_scale=256.0), warm_up_epochs=2)
    out = step(batch, epoch=0, batch_id=0)
    assert all(np.isfinite(v) for v in out.values() if isinstance(v, float)) and np.isfinite(out["total"])
    assert all(torch.equal(batch[k], before[k]) for k in batch)     # the step does not write into its input
    # the runnable example's epoch loop: the next batch is produced on a side stream under the current step
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from train_from_files import train_epoch
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0,
                                         collate_fn=collate_train_views)
    seen = []
    outs = train_epoch(step, loader, "cuda", torch.Generator().manual_seed(2), epoch=0,
                       on_step=lambda i, o: seen.append(i))
    assert seen == [0, 1] and len(outs) == 2 and all(np.isfinite(o["total"]) for o in outs)
    torch.cuda.synchronize()
