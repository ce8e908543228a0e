"""Damaged PNG and JPEG files for the decoder tests.  Test infrastructure (no pytest, no GPU).

Each builder is seeded by the caller's generator, so a test that calls it with the same seed gets the same files.
Chunk CRCs are re-made on every damaged PNG: only the decoder can notice the damage, not the chunk walk.
"""
from __future__ import annotations

import io
import struct
import zlib
from typing import Dict, List, Sequence

import numpy as np
from PIL import Image

from png_writer import chunk, filter_rows, synth_image


def rebuild_png(data: bytes, new_idat: bytes) -> bytes:
    """the same file with another IDAT payload (CRCs valid, so only the decoder can notice)"""
    i = data.index(b"IDAT") - 4
    return data[:i] + chunk(b"IDAT", new_idat) + chunk(b"IEND", b"")


def png_corrupt_cases(good: bytes, rng: np.random.Generator) -> Dict[str, bytes]:
    """Six classes of broken zlib stream inside `good` (the golden "filter4_rgb": 297 x 261 RGB, whose scanlines
    are 892 bytes), in a fixed order: truncated, bad block type, a distance before the start, bad zlib header,
    a filter type > 4, garbage."""
    img = synth_image(rng, 261, 297, 3)
    raw = filter_rows(img, [4] * 261)
    z = zlib.compress(raw, 6)
    return {
        "truncated": rebuild_png(good, z[:len(z) // 3]),
        "bad block type": rebuild_png(good, b"\x78\x9c\x07" + bytes(40)),
        "distance before start": rebuild_png(good, b"\x78\x9c\x03\x02\x00" + bytes(40)),
        "bad zlib header": rebuild_png(good, b"\x79\x9c" + z[2:]),
        "filter type 7": rebuild_png(good, zlib.compress(raw[:200 * 892] + b"\x07" + raw[200 * 892 + 1:], 6)),
        "garbage": rebuild_png(good, b"\x78\x9c" + bytes(rng.integers(0, 256, 5000).astype(np.uint8))),
    }


def png_mutants(bases: Sequence[bytes], rng: np.random.Generator, count: int = 384) -> List[bytes]:
    """`count` files whose zlib streams carry random damage: one flipped bit, one replaced byte, an 8-byte burst or
    lost bytes (everything behind shifts), 1-3 times each, cycling through `bases` and the four kinds."""
    muts = []
    for k in range(count):
        f = bases[k % len(bases)]
        i = f.index(b"IDAT")
        n = struct.unpack(">I", f[i - 4:i])[0]
        z = bytearray(f[i + 4:i + 4 + n])
        kind = k % 4
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(2, len(z)))
            if kind == 0:
                z[at] ^= 1 << int(rng.integers(0, 8))          # one bit
            elif kind == 1:
                z[at] = int(rng.integers(0, 256))               # one byte
            elif kind == 2:
                z[at:at + 8] = bytes(rng.integers(0, 256, 8).astype(np.uint8))[:len(z) - at]   # a burst
            else:
                del z[at:at + int(rng.integers(1, 40))]         # bytes lost: everything behind shifts
        muts.append(f[:i - 4] + chunk(b"IDAT", bytes(z)) + chunk(b"IEND", b""))
    return muts


def synth_jpeg_image(rng: np.random.Generator, h: int, w: int) -> Image.Image:
    """smooth colour field plus noise: what a photo's blocks look like to the entropy coder"""
    base = rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 3)).astype(np.uint8)
    a = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC)).astype(np.int16)
    a += rng.integers(-20, 20, a.shape, dtype=np.int16)
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))


def encode_jpeg(im: Image.Image, **kw) -> bytes:
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def jpeg_corrupt_pair(rng: np.random.Generator):
    """(good, bad): a 128 x 128 4:2:0 baseline JPEG and the same file whose entropy-coded data from the middle on is
    random bytes (no 0xFF, so no marker appears), closed by EOI."""
    good = encode_jpeg(synth_jpeg_image(rng, 128, 128), quality=90, subsampling=2)
    bad = bytearray(good)
    cut = len(bad) // 2
    bad[cut:-2] = bytes(rng.integers(0, 255, len(bad) - 2 - cut, dtype=np.uint8))
    bad = bytes(bad).replace(b"\xff", b"\x7f", -1)
    bad = good[:cut] + bad[cut:-2] + b"\xff\xd9"
    return good, bad
