"""CPU tests of the SimCLR training views: csrc/view_core.h compiled for the host (tests/view_emul.cpp) and the new
host entries of libhcir against live Pillow, byte for byte (the composition is tests/_simclr_ref.py), and the draws of
hcir.views (boxes, parameter table) against torchvision's / lightly's published distributions."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _simclr_ref as ref  # noqa: E402

BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)
FACTORS = [0.2, 0.35, 0.5, 0.77, 0.999, 1.0, 1.001, 1.13, 1.5, 1.8]     # both sides of 1, the range's ends
SIGMAS = [0.1, 0.15, 0.3, 0.45, 0.6, 0.8, 1.0, 1.25, 1.5, 1.75, 1.9, 2.0]


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libview_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                           "-ffp-contract=off", os.path.join(ROOT, "tests", "view_emul.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.emul_params_bytes.restype = ctypes.c_size_t
    L.emul_jitter_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float]
    L.emul_gray.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    L.emul_rgb2hsv.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.emul_blur.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float]
    L.emul_view.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_void_p]
    return L


def all_colours() -> np.ndarray:
    """Every RGB triple once, as a 4096 x 4096 image."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v >> 16, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)


def test_params_struct_matches_numpy_mirror(emul):
    from hcir import views
    assert emul.emul_params_bytes() == views.PARAMS_DTYPE.itemsize == 64


def test_hue_round_trip_all_colours(emul):
    a = all_colours()
    img = Image.fromarray(a)
    hsv = np.empty_like(a)
    emul.emul_rgb2hsv(a.ctypes.data, a.shape[0] * a.shape[1], hsv.ctypes.data)
    assert np.array_equal(hsv, np.asarray(img.convert("HSV")))
    for hue in (0.0, 0.2, -0.2, 0.07, -0.13, 0.5, -0.5):
        f = float(np.float32(hue))
        got = a.copy()
        emul.emul_jitter_op(HUE, got.ctypes.data, a.shape[0] * a.shape[1], f)
        want = np.asarray(ref.adjust_hue(img, f))
        assert np.array_equal(got, want), f"hue {hue}: {(got != want).any(axis=2).sum()} colours differ"


def test_luma_all_colours(emul):
    a = all_colours()
    got = a.copy()
    emul.emul_gray(got.ctypes.data, a.shape[0] * a.shape[1])
    assert np.array_equal(got, np.asarray(ref.grayscale(Image.fromarray(a))))


@pytest.mark.parametrize("op,pil", [(BRIGHTNESS, ref.adjust_brightness), (CONTRAST, ref.adjust_contrast),
                                    (SATURATION, ref.adjust_saturation)])
def test_blends_over_factor_grid(emul, op, pil):
    rng = np.random.default_rng(op)
    images = [rng.integers(0, 256, (97, 131, 3)).astype(np.uint8), ref.hair_like(rng, 224, 224),
              rng.integers(100, 140, (64, 64, 3)).astype(np.uint8)]
    grid = FACTORS + [float(v) for v in rng.uniform(0.2, 1.8, 12).astype(np.float32)]
    for a in images:
        for f in grid:
            f = float(np.float32(f))
            got = a.copy()
            emul.emul_jitter_op(op, got.ctypes.data, a.shape[0] * a.shape[1], f)
            want = np.asarray(pil(Image.fromarray(a), f))
            assert np.array_equal(got, want), f"op {op} factor {f}: {(got != want).sum()} bytes differ"


def test_blur_over_sigma_grid(emul, hcir_built):
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, (224, 224, 3)).astype(np.uint8), ref.hair_like(rng, 224, 224),
              rng.integers(0, 256, (53, 90, 3)).astype(np.uint8)]
    grid = SIGMAS + [float(v) for v in rng.uniform(0.1, 2.0, 12).astype(np.float32)]
    seen_r = set()
    for a in images:
        for sigma in grid:
            sigma = float(np.float32(sigma))
            got = a.copy()
            r = emul.emul_blur(got.ctypes.data, a.shape[0], a.shape[1], sigma)
            assert r in (0, 1)
            seen_r.add(r)
            want = np.asarray(ref.gaussian_blur(Image.fromarray(a), sigma))
            assert np.array_equal(got, want), f"sigma {sigma}: {(got != want).sum()} bytes differ"
            # the library's host entry hands out the same weights
            rr, ww, fw = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
            assert hcir_built.hcir_view_blur_weights(sigma, ctypes.byref(rr), ctypes.byref(ww), ctypes.byref(fw)) == 0
            assert rr.value == r and (2 * r + 1) * ww.value + 2 * fw.value <= 1 << 24
    assert seen_r == {0, 1}
    bad = ctypes.c_int32()
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert hcir_built.hcir_view_blur_weights(sigma, ctypes.byref(bad), ctypes.byref(bad), ctypes.byref(bad)) == -1
    assert hcir_built.hcir_view_blur_weights(5.0, ctypes.byref(bad), ctypes.byref(bad), ctypes.byref(bad)) == -2


def _tables(L, flt, i, o):
    ks = L.hcir_resize_ksize(flt, i, o)
    assert ks > 0
    bounds, kk = np.zeros(2 * o, np.int32), np.zeros(o * ks, np.int32)
    assert L.hcir_resize_coeffs(flt, i, o, bounds.ctypes.data, kk.ctypes.data) == 0
    return ks, bounds, kk


def _resample_axis(a: np.ndarray, ks, bounds, kk) -> np.ndarray:
    """Pillow's 8bpc pass along axis 1 of a [rows, in, 3] array with integer tables."""
    o = len(bounds) // 2
    out = np.empty((a.shape[0], o, 3), np.uint8)
    for x in range(o):
        x0, n = int(bounds[2 * x]), int(bounds[2 * x + 1])
        ss = (1 << 21) + (a[:, x0:x0 + n, :].astype(np.int64) * kk[x * ks:x * ks + n].astype(np.int64)[None, :, None]
                          ).sum(axis=1)
        out[:, x] = np.clip(ss >> 22, 0, 255)
    return out


def test_bilinear_tables_match_pillow_resize(hcir_built):
    L = hcir_built
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (301, 415, 3)).astype(np.uint8)
    pil = Image.fromarray(img)
    # (top, left, h, w): up- and down-scales, odd sizes, boxes touching every border, one axis left alone
    boxes = [(0, 0, 301, 415), (0, 0, 85, 113), (216, 302, 85, 113), (10, 20, 31, 47), (0, 100, 301, 224),
             (77, 0, 224, 415), (5, 7, 224, 224), (150, 200, 7, 9), (0, 0, 1, 1), (300, 414, 1, 1)]
    for top, left, h, w in boxes:
        src = img[top:top + h, left:left + w]
        got = src
        if w != 224:
            got = _resample_axis(got, *_tables(L, 2, w, 224))
        if h != 224:
            got = _resample_axis(got.transpose(1, 0, 2), *_tables(L, 2, h, 224)).transpose(1, 0, 2)
        want = np.asarray(ref.crop_resize(pil, (top, left, h, w)))
        assert np.array_equal(got, want), (top, left, h, w)
    # the named entry's bicubic tables are the old entries', bit for bit
    for i, o in [(1024, 224), (224, 1024), (300, 224), (7, 224), (224, 3), (225, 224), (1, 1)]:
        ks, bounds, kk = _tables(L, 3, i, o)
        assert ks == L.hcir_resize_bicubic_ksize(i, o)
        b2, k2 = np.zeros_like(bounds), np.zeros_like(kk)
        assert L.hcir_resize_bicubic_coeffs(i, o, b2.ctypes.data, k2.ctypes.data) == 0
        assert np.array_equal(bounds, b2) and np.array_equal(kk, k2)
    assert L.hcir_resize_ksize(1, 10, 10) == 0 and L.hcir_resize_ksize(2, 0, 10) == 0
    assert L.hcir_resize_coeffs(5, 10, 10, b2.ctypes.data, k2.ctypes.data) == -2
    assert L.hcir_resize_coeffs(2, 10, 10, None, None) == -1


def test_whole_view_on_the_host_matches_pillow(emul, hcir_built):
    """The kernel's sequence of phases (emul_view) over drawn parameter records, incl. all 24 jitter orders."""
    import itertools
    from hcir import views
    rng = np.random.default_rng(11)
    g = torch.Generator().manual_seed(5)
    crops = [rng.integers(0, 256, (224, 224, 3)).astype(np.uint8), ref.hair_like(rng, 224, 224)]
    params = views.draw_view_params(40, g)
    orders = np.array(list(itertools.permutations(range(4))), dtype=np.int32)
    forced = views.draw_view_params(24, g, cj_prob=1.0)
    forced["order"] = orders
    out = np.empty((3, 224, 224), np.float32)
    for k, p in enumerate(np.concatenate([params, forced])):
        a = crops[k % 2]
        rec = np.array([p], dtype=views.PARAMS_DTYPE)
        emul.emul_view(a.ctypes.data, 224, rec.ctypes.data, ref.MEAN.ctypes.data, ref.STD.ctypes.data, out.ctypes.data)
        want = ref.to_tensor_normalize(ref.apply_u8(Image.fromarray(a), p))
        assert np.array_equal(out, want), f"record {k}: {p}"


def test_argument_validation_without_gpu(hcir_built):
    from hcir import views
    L = hcir_built
    p = views.draw_view_params(2, torch.Generator().manual_seed(1))
    m, s = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    assert L.hcir_simclr_view_f32(None, None, p.ctypes.data, 2, m, s, None, None) == -1
    bad = p.copy()
    bad["order"][1] = (0, 1, 1, 3)
    # rejected on the host table before any launch (the device pointers are never touched)
    assert L.hcir_simclr_view_f32(4096, 4096, bad.ctypes.data, 2, m, s, 4096, None) == -1
    for field, value in (("flip", 2), ("brightness", -0.1), ("contrast", float("nan")), ("hue", 0.6), ("gray", -1)):
        bad = p.copy()
        bad[field][0] = value
        assert L.hcir_simclr_view_f32(4096, 4096, bad.ctypes.data, 2, m, s, 4096, None) == -1, field
    bad = p.copy()
    bad["blur"][0], bad["blur_r"][0], bad["blur_ww"][0], bad["blur_fw"][0] = 1, 1, 1 << 24, 0
    assert L.hcir_simclr_view_f32(4096, 4096, bad.ctypes.data, 2, m, s, 4096, None) == -1


def test_python_errors_without_gpu(hcir_built):
    from hcir import HcirError, views
    img = torch.zeros((64, 64, 3), dtype=torch.uint8)
    with pytest.raises(HcirError):
        views.simclr_views([img])
    with pytest.raises(HcirError):
        views.apply_view_params(torch.zeros((1, 224, 224, 3), dtype=torch.uint8), views.draw_view_params(1))
    ok = dict(flip=0, jitter=1, order=[[0, 1, 2, 3]], brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, gray=0,
              blur=1, sigma=1.0)
    views.make_view_params(**ok)
    for key, value in (("brightness", -0.5), ("contrast", float("inf")), ("saturation", -1e-3), ("hue", 0.51),
                       ("hue", -0.7), ("sigma", 0.0), ("sigma", 3.0), ("order", [[0, 0, 2, 3]]), ("flip", 2)):
        with pytest.raises(ValueError):
            views.make_view_params(**{**ok, key: value})
    with pytest.raises(ValueError):
        views.draw_view_params(4, cj_hue=0.7)
    with pytest.raises(ValueError):
        views.SimCLRTransform(rr_prob=0.5)
    with pytest.raises(ValueError):
        views.SimCLRTransform(gaussian_blur=1.5)
    with pytest.raises(ValueError):
        views.random_resized_crop_boxes([(10, 10)], min_scale=0.0)


def test_boxes_lie_inside_and_follow_get_params():
    from hcir import views
    g = torch.Generator().manual_seed(0)
    sizes = [(1024, 1024)] * 2000 + [(300, 200)] * 2000 + [(37, 501)] * 2000 + [(1, 1)] * 10 + [(224, 224)] * 500
    boxes = views.random_resized_crop_boxes(sizes, g)
    hw = np.array(sizes)
    top, left, h, w = boxes.T
    assert (h > 0).all() and (w > 0).all() and (top >= 0).all() and (left >= 0).all()
    assert (top + h <= hw[:, 0]).all() and (left + w <= hw[:, 1]).all()
    sq = slice(0, 2000)   # 1024^2: every first try of scale <= 0.75 fits, so the area and ratio ranges show
    frac = (h[sq] * w[sq]) / float(1024 * 1024)
    assert frac.min() >= 0.08 * 0.98 and frac.max() <= 1.0
    assert (frac < 0.15).any() and (frac > 0.8).any()      # both ends of the scale range are drawn
    r = w[sq] / h[sq]
    assert r.min() >= 0.75 * 0.99 and r.max() <= (4 / 3) * 1.01
    assert (top[sq] > 0).any() and (left[sq] > 0).any()
    # same seed, same table; another seed, another table
    again = views.random_resized_crop_boxes(sizes, torch.Generator().manual_seed(0))
    assert np.array_equal(boxes, again)
    assert not np.array_equal(boxes, views.random_resized_crop_boxes(sizes, torch.Generator().manual_seed(1)))


def test_box_fallback_after_ten_failed_tries():
    from hcir import views
    g = torch.Generator().manual_seed(2)
    # area >= 0.9 of a 5:1 (1:5) image with a ratio inside [3/4, 4/3] never fits: every try fails
    wide = views.random_resized_crop_boxes([(100, 500)] * 50, g, min_scale=0.9)
    h, w = 100, int(round(100 * (4 / 3)))
    assert (wide == np.array([0, (500 - w) // 2, h, w])).all()
    tall = views.random_resized_crop_boxes([(500, 100)] * 50, g, min_scale=0.9)
    w, h = 100, int(round(100 / (3 / 4)))
    assert (tall == np.array([(500 - h) // 2, 0, h, w])).all()
    # an image whose ratio is inside the range but which no try fits (min_scale > 1 is refused; use a 1 x 1 image:
    # round(sqrt(U(0.08, 1) * r)) is 0 or 1, and 1 x 1 is the whole image either way)
    one = views.random_resized_crop_boxes([(1, 1)] * 50, g)
    assert (one == np.array([0, 0, 1, 1])).all()
    # in-range ratio with every try failing: ratio pinned to 2 on a square image, area >= 0.9 -> w > W always
    sq = views.random_resized_crop_boxes([(64, 64)] * 50, g, min_scale=0.9, ratio=(2.0, 2.0))
    assert (sq == np.array([(64 - 32) // 2, 0, 32, 64])).all()   # in_ratio 1 < 2: w = W, h = round(W / 2)


def test_param_table_ranges_and_probabilities():
    from hcir import views
    n = 100_000
    p = views.draw_view_params(n, torch.Generator().manual_seed(1234))
    assert np.array_equal(p, views.draw_view_params(n, torch.Generator().manual_seed(1234)))
    for name in ("brightness", "contrast", "saturation"):
        assert p[name].min() >= np.float32(0.2) and p[name].max() <= np.float32(1.8)
        assert abs(float(p[name].mean()) - 1.0) < 0.01
    assert p["hue"].min() >= np.float32(-0.2) and p["hue"].max() <= np.float32(0.2)
    blurred = p["blur"] == 1
    assert p["sigma"][blurred].min() >= np.float32(0.1) and p["sigma"][blurred].max() <= np.float32(2.0)
    assert (p["sigma"][~blurred] == 0).all() and set(np.unique(p["blur_r"])) <= {0, 1}
    assert (np.sort(p["order"], axis=1) == np.arange(4)).all()
    for name, prob in (("flip", 0.5), ("jitter", 0.8), ("gray", 0.2), ("blur", 0.5)):
        assert set(np.unique(p[name])) <= {0, 1}
        sd = math.sqrt(prob * (1 - prob) / n)
        assert abs(float(p[name].mean()) - prob) <= 5 * sd, (name, float(p[name].mean()))
    # each of the 24 orders has probability 1/24
    codes = (p["order"] * np.array([64, 16, 4, 1])).sum(axis=1)
    counts = np.unique(codes, return_counts=True)[1]
    assert len(counts) == 24
    sd = math.sqrt((1 / 24) * (23 / 24) / n)
    assert (np.abs(counts / n - 1 / 24) <= 5 * sd).all()
    # keywords reach the draws
    q = views.draw_view_params(1000, torch.Generator().manual_seed(1), hf_prob=0.0, cj_prob=1.0, gaussian_blur=1.0,
                               random_gray_scale=0.0, cj_strength=0.5, sigmas=(0.5, 0.6))
    assert not q["flip"].any() and q["jitter"].all() and q["blur"].all() and not q["gray"].any()
    assert q["brightness"].min() >= np.float32(0.6) and q["brightness"].max() <= np.float32(1.4)
    assert np.abs(q["hue"]).max() <= np.float32(0.1) and q["sigma"].min() >= np.float32(0.5)
