"""HairEncoder.device_windows on files the device decoders flag as corrupt: such a file goes where the reference
sends every file, PIL's Image.open(...).convert("RGB") - which raises for it, or whose pixels the window must then
hold byte for byte.  No zero-filled window may reach the resize, and no embedding of one may be stored."""
import io
import os
import struct
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from corrupt_streams import jpeg_corrupt_pair, png_corrupt_cases, png_mutants  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def png_streams(golden_dir):
    z = np.load(os.path.join(golden_dir, "png_streams.npz"))
    files = [z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes() for i in range(len(z["names"]))]
    return {str(n): f for n, f in zip(z["names"], files)}


@pytest.fixture(scope="module")
def jpeg_streams(golden_dir):
    z = np.load(os.path.join(golden_dir, "jpeg_streams.npz"))
    return [z["data"][z["offsets"][i]:z["offsets"][i + 1]].tobytes() for i in range(len(z["names"]))]


@pytest.fixture(scope="module")
def enc(hcir_built):
    from hcir.hair_encoder import HairEncoder
    torch.manual_seed(0)
    return HairEncoder(None, "vit_base_patch16", device="cuda")


def _pil_window(enc, data):
    """the reference's window of a file, or None where PIL raises for it"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with Image.open(io.BytesIO(data)) as im:
                return enc._window_u8(im.convert("RGB")).numpy()
    except Exception:  # noqa: BLE001 - PIL rejects the file (zlib error, truncated data, broken entropy stream ...)
        return None


def _check_batch(enc, batch, what):
    """device_windows(batch) raises where PIL raises for one of the files; otherwise equals PIL's windows byte for
    byte, every file of the batch."""
    ref = [_pil_window(enc, f) for f in batch]
    if any(r is None for r in ref):
        with pytest.raises(Exception):
            enc.device_windows(batch)
        return False
    got = enc.device_windows(batch).cpu().numpy()
    for k, r in enumerate(ref):
        np.testing.assert_array_equal(got[k], r, err_msg=f"{what}: file {k}")
    return True


def test_corrupt_file_in_a_mixed_batch_goes_to_pil(enc, png_streams, jpeg_streams):
    """One device_windows batch of good PNG and JPEG files (two PNG sizes, so two PNG groups) with a single corrupt
    file: each of the six corrupt-PNG classes of the decoder test, and its corrupt JPEG."""
    good_png = [png_streams[n] for n in ("filter4_rgb", "asset_20519_hair.png", "filter4_rgb", "palette")]
    good_jpeg = jpeg_streams[:3]
    cases = png_corrupt_cases(png_streams["filter4_rgb"], np.random.default_rng(4))
    jgood, jbad = jpeg_corrupt_pair(np.random.default_rng(3))
    cases["jpeg: broken entropy stream"] = jbad
    raised = []
    for name, bad in cases.items():
        batch = good_png[:2] + good_jpeg[:2] + [bad] + good_png[2:] + [jgood] + good_jpeg[2:]
        if not _check_batch(enc, batch, name):
            raised.append(name)
    # the damaged streams Pillow rejects outright; the mixed batch must not come back with a window for them
    assert [n for n in raised if not n.startswith("jpeg")] == [n for n in cases if not n.startswith("jpeg")]


def _only_the_checksum_is_wrong(data):
    """True when the file's zlib stream inflates whole as raw deflate to the full scanline size with valid filter
    types, and only its Adler-32 disagrees: PIL raises for it, the device does not verify the Adler-32."""
    i = data.index(b"IDAT")
    w, h = struct.unpack(">II", data[16:24])
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[data[25]]
    z = data[i + 4:i + 4 + struct.unpack(">I", data[i - 4:i])[0]]
    try:
        d = zlib.decompressobj(-15)
        raw = d.decompress(z[2:])
        zlib.decompress(z)
        return False
    except zlib.error:
        if not d.eof or len(raw) < h * (1 + w * bpp):
            return False
    rows = np.frombuffer(raw[:h * (1 + w * bpp)], np.uint8).reshape(h, 1 + w * bpp)
    return bool(rows[:, 0].max() <= 4)


def _mutants(png_streams):
    bases = [png_streams[n] for n in ("filter4_rgb", "mixed_blocks", "grey_l1", "palette", "mixed_filters_rgba_l9",
                                      "fixed_blocks")]
    return png_mutants(bases, np.random.default_rng(77))


def test_mutated_png_streams_through_device_windows(enc, png_streams):
    """The 384 mutants of the decoder test, whole-image decode: per file, PIL's window byte for byte where PIL
    decodes it, a raise where PIL rejects it.  Chunks of 48, a chunk that raises is re-run file by file so that one
    raise hides no other file.  Left out of the raise requirement: files whose only fault is the Adler-32 of the
    stream (test_png_adler32_damage_reaches_pil below)."""
    muts = _mutants(png_streams)
    decoded = rejected = tail = 0
    for c in range(0, len(muts), 48):
        chunk = muts[c:c + 48]
        try:
            got = enc.device_windows(chunk).cpu().numpy()
        except Exception:  # noqa: BLE001 - at least one file of the chunk is rejected: each file alone
            got = None
        for k, f in enumerate(chunk):
            ref = _pil_window(enc, f)
            if ref is None and _only_the_checksum_is_wrong(f):
                tail += 1
            elif got is not None:
                assert ref is not None, f"mutant {c + k}: PIL rejects it, device_windows returned a window"
                np.testing.assert_array_equal(got[k], ref, err_msg=f"mutant {c + k}")
            elif ref is None:
                with pytest.raises(Exception):
                    enc.device_windows([f])
            else:
                np.testing.assert_array_equal(enc.device_windows([f]).cpu().numpy()[0], ref, err_msg=f"mutant {c + k}")
            decoded += ref is not None
            rejected += ref is None
    assert rejected - tail > 250 and decoded >= 1
    print(f"{decoded} of {len(muts)} mutants decoded by PIL, {rejected} rejected ({tail} with only the Adler-32 wrong)")


@pytest.mark.xfail(strict=True, reason="the device inflate does not verify the zlib stream's Adler-32, which PIL "
                                       "does: a file whose data decode and whose checksum is wrong is not flagged")
def test_png_adler32_damage_reaches_pil(enc, png_streams):
    """Mutants whose stream decodes to valid scanlines but whose Adler-32 is wrong: PIL raises for every one of them,
    so device_windows must raise too.  Known gap of the device inflate, kept visible by this strict xfail."""
    bad = [f for f in _mutants(png_streams) if _only_the_checksum_is_wrong(f) and _pil_window(enc, f) is None]
    assert len(bad) > 50
    for f in bad:
        with pytest.raises(Exception):
            enc.device_windows([f])


def test_corrupt_file_on_disk_stops_the_embedding_pass(enc, png_streams, jpeg_streams, tmp_path):
    """extract_dataset_features over an ImageFolder with one corrupt file raises, as the reference's loader does,
    and stores no embeddings; encode_single_image on that file raises too, and a good file next to it embeds."""
    root = tmp_path / "data"
    for c in ("a", "b"):
        (root / c).mkdir(parents=True)
    (root / "a" / "0.png").write_bytes(png_streams["filter4_rgb"])
    (root / "a" / "1.jpg").write_bytes(jpeg_streams[0])
    bad = png_corrupt_cases(png_streams["filter4_rgb"], np.random.default_rng(4))["truncated"]
    assert _pil_window(enc, bad) is None
    (root / "b" / "2.png").write_bytes(bad)
    (root / "b" / "3.png").write_bytes(png_streams["palette"])
    out = tmp_path / "emb"
    with pytest.raises(Exception):
        enc.extract_dataset_features(str(root), batch_size=4, num_workers=0, save_dir=str(out))
    assert not (out / "embeddings.npy").exists()
    with pytest.raises(Exception):
        enc.encode_single_image(str(root / "b" / "2.png"))
    e = enc.encode_single_image(str(root / "b" / "3.png"))
    assert e.shape == (768,) and np.isfinite(e).all()
