"""hcir.views — the two SimCLR views of the pretrain step on the HIP device (include/hcir.h, csrc/view.hip).

Stands where the reference's loader workers run `SimCLRTransform(input_size=224)` on every decoded hair-region image
(HP/mainpretrain.py:130; HP/utils/dataloader.py:36-38: `{"anchor": images[0], "pos1": images[1]}`), i.e. lightly's
transform over torchvision's PIL-mode ops, all of which Pillow executes:

    RandomResizedCrop(224, scale=(0.08, 1), ratio=(3/4, 4/3), bilinear) -> RandomHorizontalFlip(0.5)
    -> RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], p=0.8) -> RandomGrayscale(0.2)
    -> GaussianBlur(sigmas=(0.1, 2), prob=0.5) -> ToTensor -> Normalize(ImageNet)

The host draws the parameters of every view (`random_resized_crop_boxes`, `draw_view_params`); the device does the
work: the crop + bilinear resize is a job of the Pillow-exact resampler (`hcir.resize.resize_boxes`), everything after
it one workgroup of `hcir_simclr_view_f32` with the 224 x 224 image resident in LDS.  The bytes equal Pillow's after
every op.  Deviation: the random stream is this module's (a `torch.Generator` fills the tables below with the
distributions above), not the sequence torch's / Python's global generators would have produced inside torchvision.
There is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, resize
from ._lib import HcirError, check
from .transform import _MEAN, _STD

SIZE = 224
BRIGHTNESS, CONTRAST, SATURATION, HUE = range(4)   # HCIR_VIEW_*: entries of "order"
# mirror of hcir_view_params (include/hcir.h)
PARAMS_DTYPE = np.dtype([("flip", "<i4"), ("jitter", "<i4"), ("order", "<i4", (4,)), ("brightness", "<f4"),
                         ("contrast", "<f4"), ("saturation", "<f4"), ("hue", "<f4"), ("gray", "<i4"), ("blur", "<i4"),
                         ("blur_r", "<i4"), ("blur_ww", "<u4"), ("blur_fw", "<u4"), ("sigma", "<f4")])
assert PARAMS_DTYPE.itemsize == 64
RESIZE_CHUNK = 512   # views per resampler call: its 8-bit intermediate is up to source rows x 224 x 3 bytes per view


def _uniform(gen: Optional[torch.Generator], shape, lo: float, hi: float) -> np.ndarray:
    """U(lo, hi) in float64 from the caller's generator (host)."""
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo).numpy()


def _randint(gen: Optional[torch.Generator], high: np.ndarray) -> np.ndarray:
    """Uniform integers in [0, high) per element."""
    u = torch.rand(high.shape, generator=gen, dtype=torch.float64).numpy()
    return np.minimum((u * high).astype(np.int64), high - 1)


def random_resized_crop_boxes(sizes: Sequence[Tuple[int, int]], generator: Optional[torch.Generator] = None,
                              min_scale: float = 0.08, max_scale: float = 1.0,
                              ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0), tries: int = 10) -> np.ndarray:
    """torchvision RandomResizedCrop.get_params for every (height, width) of `sizes` -> int64 [n, 4] of
    (top, left, h, w): up to `tries` draws of area * U(scale) and exp(U(log ratio)), the first whose rounded box fits
    the image; after that the centre crop with the image's ratio clamped to `ratio`."""
    if not 0 < min_scale <= max_scale or not 0 < ratio[0] <= ratio[1]:
        raise ValueError("scale and ratio must be positive, increasing ranges")
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if (hw <= 0).any():
        raise ValueError("image sizes must be positive")
    n = len(hw)
    H, W = hw[:, 0], hw[:, 1]
    area = (H * W).astype(np.float64)[:, None]
    target = area * _uniform(generator, (n, tries), min_scale, max_scale)
    aspect = np.exp(_uniform(generator, (n, tries), math.log(ratio[0]), math.log(ratio[1])))
    w = np.rint(np.sqrt(target * aspect)).astype(np.int64)   # Python's round(): half to even
    h = np.rint(np.sqrt(target / aspect)).astype(np.int64)
    ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    first = np.argmax(ok, axis=1)
    rows = np.arange(n)
    bw, bh = w[rows, first], h[rows, first]
    top = _randint(generator, np.maximum(H - bh, 0) + 1)
    left = _randint(generator, np.maximum(W - bw, 0) + 1)
    boxes = np.stack([top, left, bh, bw], axis=1)
    for i in np.nonzero(~ok.any(axis=1))[0]:
        height, width = int(H[i]), int(W[i])
        in_ratio = float(width) / float(height)
        if in_ratio < ratio[0]:
            fw, fh = width, int(round(width / ratio[0]))
        elif in_ratio > ratio[1]:
            fh, fw = height, int(round(height * ratio[1]))
        else:
            fw, fh = width, height
        boxes[i] = ((height - fh) // 2, (width - fw) // 2, fh, fw)
    return boxes


def _blur_weights(sigma: float) -> Tuple[int, int, int]:
    r, ww, fw = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = _lib.lib().hcir_view_blur_weights(float(sigma), ctypes.byref(r), ctypes.byref(ww), ctypes.byref(fw))
    if rc != 0:
        raise ValueError(f"blur sigma {sigma} is outside (0, 2.3] (hcir_view_blur_weights: status {rc})")
    return r.value, ww.value, fw.value


def make_view_params(flip, jitter, order, brightness, contrast, saturation, hue, gray, blur, sigma) -> np.ndarray:
    """A parameter table (PARAMS_DTYPE, [n]) from per-view arrays (scalars broadcast).  order: [n, 4] permutations of
    (BRIGHTNESS, CONTRAST, SATURATION, HUE).  Raises ValueError for anything torchvision / lightly would refuse:
    a negative factor, |hue| > 0.5, an order that is no permutation, sigma outside (0, 2.3] on a blurred view."""
    order = np.asarray(order, dtype=np.int32).reshape(-1, 4)
    n = max([len(order)] + [np.size(v) for v in (flip, jitter, brightness, contrast, saturation, hue, gray, blur,
                                                  sigma)])
    p = np.zeros(n, PARAMS_DTYPE)
    for name, v in (("flip", flip), ("jitter", jitter), ("gray", gray), ("blur", blur)):
        v = np.broadcast_to(np.asarray(v), (n,))
        if not np.isin(v, (0, 1)).all():
            raise ValueError(f"{name} must be 0 or 1")
        p[name] = v
    p["order"] = np.broadcast_to(order, (n, 4))
    if not (np.sort(p["order"], axis=1) == np.arange(4)).all():
        raise ValueError("order must be a permutation of (0, 1, 2, 3) per view")
    for name, v in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        v = np.broadcast_to(np.asarray(v, dtype=np.float32), (n,))
        if not (np.isfinite(v) & (v >= 0)).all():
            raise ValueError(f"{name} factors must be finite and non-negative")
        p[name] = v
    hue = np.broadcast_to(np.asarray(hue, dtype=np.float32), (n,))
    if not (np.abs(hue) <= 0.5).all():
        raise ValueError("hue factors must lie in [-0.5, 0.5]")
    p["hue"] = hue
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (n,))
    p["sigma"] = np.where(p["blur"] != 0, sigma, 0)
    for i in np.nonzero(p["blur"])[0]:
        p["blur_r"][i], p["blur_ww"][i], p["blur_fw"][i] = _blur_weights(sigma[i])
    return p


def _check_transform(hf_prob, cj_prob, cj_strength, cj_bright, cj_contrast, cj_sat, cj_hue, random_gray_scale,
                     gaussian_blur, sigmas):
    """Range checks of the transform's keywords -> the four jitter strengths."""
    for name, v in (("hf_prob", hf_prob), ("cj_prob", cj_prob), ("random_gray_scale", random_gray_scale),
                    ("gaussian_blur", gaussian_blur)):
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"{name} must be a probability")
    strengths = tuple(cj_strength * v for v in (cj_bright, cj_contrast, cj_sat, cj_hue))
    if min(strengths) < 0 or strengths[3] > 0.5:
        raise ValueError("colour jitter strengths must be non-negative and the hue strength at most 0.5")
    if not 0 < sigmas[0] <= sigmas[1] <= 2.3:
        raise ValueError("sigmas must be a positive, increasing range inside (0, 2.3]")
    return strengths


def draw_view_params(n: int, generator: Optional[torch.Generator] = None, hf_prob: float = 0.5,
                     cj_prob: float = 0.8, cj_strength: float = 1.0, cj_bright: float = 0.8,
                     cj_contrast: float = 0.8, cj_sat: float = 0.8, cj_hue: float = 0.2,
                     random_gray_scale: float = 0.2, gaussian_blur: float = 0.5,
                     sigmas: Tuple[float, float] = (0.1, 2.0)) -> np.ndarray:
    """Parameters of n views with lightly's SimCLRTransform keywords and defaults: flags Bernoulli(hf_prob, cj_prob,
    random_gray_scale, gaussian_blur); brightness / contrast / saturation ~ U(max(0, 1 - s), 1 + s) with
    s = cj_strength * cj_*, hue ~ U(-s, s); a uniform permutation of the four ops; sigma ~ U(sigmas)."""
    s_b, s_c, s_s, s_h = _check_transform(hf_prob, cj_prob, cj_strength, cj_bright, cj_contrast, cj_sat, cj_hue,
                                          random_gray_scale, gaussian_blur, sigmas)
    flags = _uniform(generator, (4, n), 0.0, 1.0)
    f = _uniform(generator, (5, n), 0.0, 1.0)
    order = np.argsort(_uniform(generator, (n, 4), 0.0, 1.0), axis=1)

    def between(u, lo, hi):
        return (lo + u * (hi - lo)).astype(np.float32)

    return make_view_params(flip=flags[0] < hf_prob, jitter=flags[1] < cj_prob, order=order,
                            brightness=between(f[0], max(0.0, 1 - s_b), 1 + s_b),
                            contrast=between(f[1], max(0.0, 1 - s_c), 1 + s_c),
                            saturation=between(f[2], max(0.0, 1 - s_s), 1 + s_s), hue=between(f[3], -s_h, s_h),
                            gray=flags[2] < random_gray_scale, blur=flags[3] < gaussian_blur,
                            sigma=between(f[4], sigmas[0], sigmas[1]))


def apply_view_params(crops: torch.Tensor, params: np.ndarray) -> torch.Tensor:
    """hcir_simclr_view_f32: uint8 [n, 224, 224, 3] device crops + a parameter table -> fp32 [n, 3, 224, 224].
    Asynchronous on the current stream."""
    if not isinstance(crops, torch.Tensor) or not crops.is_cuda:
        raise HcirError("hcir_simclr_view_f32 runs on a HIP device only (no CPU fallback)")
    if crops.dtype != torch.uint8 or crops.dim() != 4 or tuple(crops.shape[1:]) != (SIZE, SIZE, 3) or \
            not crops.is_contiguous():
        raise HcirError(f"crops must be a contiguous uint8 [n, {SIZE}, {SIZE}, 3] tensor")
    params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE)
    n = crops.size(0)
    if params.shape != (n,):
        raise ValueError(f"{n} crops but a parameter table of shape {params.shape}")
    dev = crops.device
    host = torch.empty(n * PARAMS_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
    ctypes.memmove(host.data_ptr(), params.ctypes.data, params.nbytes)
    table = host.to(dev, non_blocking=True)
    out = torch.empty((n, 3, SIZE, SIZE), dtype=torch.float32, device=dev)
    mean = (ctypes.c_float * 3)(*_MEAN.tolist())
    std = (ctypes.c_float * 3)(*_STD.tolist())
    rc = _lib.lib().hcir_simclr_view_f32(crops.data_ptr(), table.data_ptr(), params.ctypes.data, n, mean, std,
                                         out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc == -1:
        raise ValueError("hcir_simclr_view_f32 refused the parameter table (flag, order, factor or blur weights out "
                         "of range; build it with make_view_params / draw_view_params)")
    check(rc, "hcir_simclr_view_f32")
    out._hcir_keepalive = (table, host, crops)
    return out


def simclr_views(images: Sequence[torch.Tensor], generator: Optional[torch.Generator] = None,
                 boxes: Optional[np.ndarray] = None, params: Optional[np.ndarray] = None,
                 **transform_kwargs) -> Dict[str, torch.Tensor]:
    """Two independent views of every image: a list of B RGB8 [h, w, 3] device tensors of any sizes ->
    {"anchor", "pos1"} fp32 [B, 3, 224, 224].  boxes int [2, B, 4] (top, left, h, w) and params (PARAMS_DTYPE [2, B])
    replace the draws (index 0: anchor, 1: pos1).  transform_kwargs: lightly's SimCLRTransform keywords
    (min_scale, hf_prob, cj_*, random_gray_scale, gaussian_blur, sigmas)."""
    imgs = list(images.unbind(0)) if isinstance(images, torch.Tensor) else list(images)
    if not imgs or any(not isinstance(t, torch.Tensor) or not t.is_cuda for t in imgs):
        raise HcirError("simclr_views takes RGB8 [h, w, 3] tensors on a HIP device (no CPU fallback)")
    b = len(imgs)
    box_kw = {k: transform_kwargs.pop(k) for k in ("min_scale",) if k in transform_kwargs}
    if boxes is None:
        boxes = random_resized_crop_boxes([(int(t.size(0)), int(t.size(1))) for t in imgs] * 2, generator, **box_kw)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(2 * b, 4)
    if params is None:
        params = draw_view_params(2 * b, generator, **transform_kwargs)
    elif transform_kwargs:
        raise TypeError(f"unexpected keywords next to an explicit parameter table: {sorted(transform_kwargs)}")
    params = np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(2 * b)
    index = list(range(b)) * 2
    parts = [resize.resize_boxes(imgs, boxes[s:s + RESIZE_CHUNK], SIZE, "bilinear", index[s:s + RESIZE_CHUNK])
             for s in range(0, 2 * b, RESIZE_CHUNK)]
    crops = parts[0] if len(parts) == 1 else torch.cat(parts)
    out = apply_view_params(crops, params)
    return {"anchor": out[:b], "pos1": out[b:]}


class SimCLRTransform:
    """lightly's SimCLRTransform with the constructor keywords that matter on this path; called with a list of RGB8
    device images it returns {"anchor", "pos1"} (HP/utils/dataloader.py:38).  rr_prob / vf_prob are zero in the
    reference's configuration and are not implemented: a non-zero value raises."""

    def __init__(self, input_size: int = 224, cj_prob: float = 0.8, cj_strength: float = 1.0, cj_bright: float = 0.8,
                 cj_contrast: float = 0.8, cj_sat: float = 0.8, cj_hue: float = 0.2, min_scale: float = 0.08,
                 random_gray_scale: float = 0.2, gaussian_blur: float = 0.5, sigmas: Tuple[float, float] = (0.1, 2),
                 vf_prob: float = 0.0, hf_prob: float = 0.5, rr_prob: float = 0.0, generator=None):
        if input_size != SIZE:
            raise ValueError(f"the device view is built for input_size={SIZE}")
        if vf_prob or rr_prob:
            raise ValueError("vf_prob / rr_prob are not implemented (zero in the reference's configuration)")
        self.kwargs = dict(cj_prob=cj_prob, cj_strength=cj_strength, cj_bright=cj_bright, cj_contrast=cj_contrast,
                           cj_sat=cj_sat, cj_hue=cj_hue, min_scale=min_scale, random_gray_scale=random_gray_scale,
                           gaussian_blur=gaussian_blur, sigmas=tuple(sigmas), hf_prob=hf_prob)
        _check_transform(hf_prob, cj_prob, cj_strength, cj_bright, cj_contrast, cj_sat, cj_hue, random_gray_scale,
                         gaussian_blur, tuple(sigmas))
        if not 0 < min_scale <= 1:
            raise ValueError("min_scale must lie in (0, 1]")
        self.generator = generator

    def __call__(self, images: Sequence[torch.Tensor]) -> Dict[str, torch.Tensor]:
        return simclr_views(images, self.generator, **self.kwargs)
