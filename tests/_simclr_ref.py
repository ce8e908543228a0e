"""The reference of every SimCLR-view comparison: live Pillow, composed the way torchvision's PIL-mode ops and
lightly's GaussianBlur compose it (lightly SimCLRTransform(input_size=224), HP/mainpretrain.py:130).  Nothing here
calls the code under test; a parameter record is read only for its drawn values (flags, order, factors, sigma)."""
import numpy as np
from PIL import Image, ImageEnhance, ImageFilter

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
SIZE = 224


def crop_resize(img: Image.Image, box, size: int = SIZE) -> Image.Image:
    """torchvision F.resized_crop on a PIL image: crop(top, left, h, w) then resize((size, size), BILINEAR)."""
    top, left, h, w = (int(v) for v in box)
    return img.crop((left, top, left + w, top + h)).resize((size, size), Image.BILINEAR)


def adjust_brightness(img, f):
    return ImageEnhance.Brightness(img).enhance(f)


def adjust_contrast(img, f):
    return ImageEnhance.Contrast(img).enhance(f)


def adjust_saturation(img, f):
    return ImageEnhance.Color(img).enhance(f)


def adjust_hue(img, f):
    """torchvision _functional_pil.adjust_hue: H += uint8(hue_factor * 255) modulo 256."""
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h = (np_h.astype(np.int32) + (int(f * 255) & 255)).astype(np.uint8)   # wraps modulo 256
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


JITTER = (adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue)   # torchvision ColorJitter's fn ids


def grayscale(img):
    """torchvision rgb_to_grayscale(num_output_channels=3)."""
    l = np.array(img.convert("L"), dtype=np.uint8)
    return Image.fromarray(np.dstack([l, l, l]), "RGB")


def gaussian_blur(img, sigma):
    """lightly GaussianBlur: img.filter(ImageFilter.GaussianBlur(radius=sigma))."""
    return img.filter(ImageFilter.GaussianBlur(radius=sigma))


def to_tensor_normalize(img) -> np.ndarray:
    """ToTensor + Normalize(ImageNet) in fp32 -> [3, h, w]."""
    a = np.asarray(img, dtype=np.uint8).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((a - MEAN) / STD).transpose(2, 0, 1))


def apply_u8(img: Image.Image, p) -> Image.Image:
    """Everything behind the crop + resize, on a PIL image; p: one parameter record."""
    if int(p["flip"]):
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if int(p["jitter"]):
        factors = (p["brightness"], p["contrast"], p["saturation"], p["hue"])
        for op in p["order"]:
            img = JITTER[int(op)](img, float(factors[int(op)]))   # the fp32 factor as a Python float
    if int(p["gray"]):
        img = grayscale(img)
    if int(p["blur"]):
        img = gaussian_blur(img, float(p["sigma"]))
    return img


def view(img: Image.Image, box, p) -> np.ndarray:
    """One view of an RGB PIL image -> fp32 [3, 224, 224]."""
    return to_tensor_normalize(apply_u8(crop_resize(img, box), p))


def hair_like(rng, h: int, w: int) -> np.ndarray:
    """An image like the reference's hair-region crops: smooth colour inside a blob, black background."""
    small = rng.integers(0, 256, (max(h // 16, 2), max(w // 16, 2), 3)).astype(np.uint8)
    a = np.asarray(Image.fromarray(small).resize((w, h), Image.BICUBIC)).copy()
    yy, xx = np.mgrid[0:h, 0:w]
    inside = ((yy - h * 0.45) / (h * 0.4)) ** 2 + ((xx - w * 0.5) / (w * 0.33)) ** 2 <= 1.0
    a[~inside] = 0
    return a
