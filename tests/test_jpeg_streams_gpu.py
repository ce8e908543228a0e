"""GPU tests of the device JPEG decoder on hand-built streams (tests/jpeg_writer.py, tests/_jpeg_cases.py) and on every
kernel instantiation: the four jpeg_huffman_kernel<threads, fast> variants and both jpeg_color_kernel variants, each
asserted through hcir_jpeg_plan before the decode that takes it.  Bar: BYTE-EXACT against live Pillow (libjpeg-turbo),
or against oracle/jpeg.py alone for the extreme-magnitude cases (the reference rule of tests/_jpeg_cases.py).  Every
stream here has been through the host-compiled emulation and the sanitised stand-alone program on the CPU
(tests/test_jpeg_host.py) - truncated and corrupt streams stay there."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpeg_cases as jc  # noqa: E402
from corrupt_streams import encode_jpeg, synth_jpeg_image  # noqa: E402

pytestmark = pytest.mark.gpu

GEOM_WORDS, GEOM_ROUNDS = 45, 38   # JGeom of csrc/jpeg.hip: int32 words per record, index of `rounds` (first in the workspace)


def _stage(files):
    from hcir import jpeg
    return jpeg.stage_batch(files)


def _decode(files, size, want_plan, allow_rejected=False):
    """Stage, assert the plan (threads, fast, colour pixels per thread), decode with the status checked."""
    from hcir import jpeg
    staged = _stage(files)
    plan = jpeg.plan(staged, size)
    print(f"hcir_jpeg_plan: b={len(files)} window={size} -> jpeg_huffman_kernel<{plan[0]}, {str(plan[1]).lower()}>, "
          f"jpeg_color_kernel<{plan[2]}>")
    assert plan == want_plan, (plan, want_plan)
    out = jpeg.decode_windows(staged.to("cuda"), size, check_status=True, _skip_rejected_check=allow_rejected)
    return out, staged


def _decode_raw(files, wh, ww, canary_rows=1):
    """The C entry point with buffers of the test's own: a canary behind the output, the workspace readable."""
    from hcir import _lib, jpeg
    L = _lib.lib()
    staged = _stage(files)
    b = staged.b
    dev_blob = staged.blob.to("cuda")
    n = b * wh * ww * 3
    out = torch.full((n + canary_rows * ww * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    hdrs = staged._host_headers.data_ptr()
    wsb = L.hcir_jpeg_workspace_bytes(hdrs, b, wh, ww)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    status = torch.full((b,), -77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.hcir_jpeg_decode_window_u8(dev_blob.data_ptr(), hdrs, b, wh, ww, out.data_ptr(), status.data_ptr(),
                                      ws.data_ptr(), ws.numel(), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * b
    o = out.cpu().numpy()
    assert (o[n:] == 0xA5).all(), "the colour kernel wrote behind the output buffer"
    off = (-ws.data_ptr()) % 256
    geom = ws[off:off + b * GEOM_WORDS * 4].cpu().numpy().view(np.int32).reshape(b, GEOM_WORDS)
    return o[:n].reshape(b, wh, ww, 3), staged, geom


def _check(got, cs, wh, ww, tag):
    for i, c in enumerate(cs):
        np.testing.assert_array_equal(got[i], c.window(wh, ww), err_msg=f"{tag}: {c.name} window {wh}x{ww}")


# ---- all four Huffman kernels on the edge sizes -----------------------------------------------------------------
@pytest.mark.parametrize("threads,fast", [(1024, True), (1024, False), (512, True), (512, False)])
def test_every_huffman_instantiation_on_edge_sizes(threads, fast, hcir_built):
    """48 distinct small streams (1 x 1, 3 x 5, 17 x 3 ... 50 x 70; grey, 4:4:4, 4:2:2, 4:2:0; restart intervals 0, 1, 3).
    The 40 with use2 == 1 alone take the fast loop; one use2 == 0 file appended sends the whole batch to the generic
    loop; repeated to >= 384 images they take the 512-thread kernels.  Window 80 x 72 > every image."""
    small = jc.small_cases()
    cs = [c for c in small if c.expect["fast"]] if fast else small + [jc.cases()["tab_dc_one"]]
    assert len(cs) == (40 if fast else 49)
    reps = 1 if threads == 1024 else -(-384 // len(cs))
    wh, ww = 80, 72
    out, _ = _decode([c.data for c in cs] * reps, (wh, ww), (threads, fast, 4))
    assert out.shape[0] >= (384 if threads == 512 else 1)
    got = out[:len(cs)].cpu().numpy()
    _check(got, cs, wh, ww, f"<{threads},{fast}>")
    for r in range(1, reps):   # every copy of a repeated file is identical
        assert torch.equal(out[r * len(cs):(r + 1) * len(cs)], out[:len(cs)]), f"copy {r}"


def _sweep_files():
    """The files of test_jpeg_gpu.py::test_live_pillow_sweep (the same seed and order)."""
    rng = np.random.default_rng(17)
    files = []
    for (h, w) in [(64, 64), (50, 70), (33, 17), (8, 8), (1, 1), (17, 3), (256, 240), (3, 5), (225, 223), (500, 333)]:
        for ss in (0, 1, 2):
            for ri in (0, 1, 5):
                kw = dict(quality=int(rng.choice([30, 75, 90, 95, 100])), subsampling=ss,
                          optimize=bool(rng.integers(0, 2)))
                if ri:
                    kw["restart_marker_blocks"] = ri
                    kw.pop("optimize", None)
                files.append(encode_jpeg(synth_jpeg_image(rng, h, w), **kw))
        files.append(encode_jpeg(synth_jpeg_image(rng, h, w).convert("L"), quality=85))
    return files


def test_live_pillow_sweep_split_by_loop(hcir_built):
    """Pillow's optimize=True writes incomplete tables (use2 == 0) for small images, and one such file sends a batch
    to the generic loop: the fast-table files of the sweep in a batch of their own run the production loop on the
    1 x 1 ... 17 x 3 images, restart interval 1 and the small grey images; all 100 together run the generic loop."""
    files = _sweep_files()
    assert len(files) == 100
    staged = _stage(files)      # kept alive: headers() is a view of its blob
    hdrs = staged.headers()

    def is_fast(h):
        return all(h.huff[t].lut.use2 for k in range(h.ncomp) for t in (h.dc_tab[k], h.ac_tab[k]))

    fast = [f for f, h in zip(files, hdrs) if is_fast(h)]
    print(f"live Pillow sweep: {len(fast)} fast-table files, {len(files) - len(fast)} with use2 == 0")
    assert 50 <= len(fast) < 100
    full = {id(f): np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files}
    for batch, is_f in ((fast, True), (files, False)):
        for size in ((224, 224), (32, 48)):
            out, _ = _decode(batch, size, (1024, is_f, 4))
            got = out.cpu().numpy()
            for i, f in enumerate(batch):
                np.testing.assert_array_equal(got[i], jc.center_window(full[id(f)], *size),
                                              err_msg=f"file {i} {full[id(f)].shape} window {size} fast {is_f}")


# ---- the one-pixel-per-thread colour kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("window", [(31, 45), (7, 1), (224, 222)])
def test_color_kernel_one_pixel_per_thread(window, hcir_built):
    """win_w % 4 != 0 takes jpeg_color_kernel<1> (byte stores).  A mixed batch with images smaller and larger than
    the window; a canary row behind the output buffer stays untouched."""
    from hcir import jpeg
    named = jc.cases()
    cs = jc.small_cases()[::3] + [named[n] for n in ("tab_four", "sym_zrl_noeob", "dc_ri7", "fmt_sof1_q16",
                                                     "fmt_fill_rst", "sym_extreme", "tab_look2")]
    wh, ww = window
    assert ww % 4 and any(c.expected().shape[0] < wh for c in cs) and any(c.expected().shape[1] > ww for c in cs)
    files = [c.data for c in cs]
    plan = jpeg.plan(_stage(files), window)
    print(f"hcir_jpeg_plan: b={len(files)} window={window} -> {plan}")
    assert plan[0] == 1024 and plan[2] == 1
    got, _, _ = _decode_raw(files, wh, ww)
    _check(got, cs, wh, ww, "color<1>")


# ---- every named case at 1024 and 512 threads ---------------------------------------------------------------------------
@pytest.mark.parametrize("threads,fast", [(1024, True), (1024, False), (512, True), (512, False)])
def test_every_named_case_byte_exact(threads, fast, hcir_built):
    """The case table (tables, symbols, synchronisation, DC scan, geometry, format) split by the loop its tables take,
    as a small batch (1024 threads) and padded to 384 images with copies of a tiny file (512 threads).  Window
    264 x 264 shows every MCU (1089 MCUs of the dc_* cases: chunk 2 and 3 in the DC scan); window 31 x 45 leaves
    last_mcu short of the last MCU.  The never-resynchronising stream has a test of its own."""
    named = jc.cases()
    cs = [c for c in named.values() if bool(c.expect["fast"]) == fast and c.name != "sync_never"]
    assert len(cs) >= 5
    pad = [] if threads == 1024 else [named["geo_nact1" if fast else "tab_dc_one"]] * (384 - len(cs))
    for (wh, ww) in (jc.BIG_WINDOW, jc.SMALL_WINDOW):
        out, _ = _decode([c.data for c in cs + pad], (wh, ww), (threads, fast, 4 if ww % 4 == 0 else 1))
        _check(out[:len(cs)].cpu().numpy(), cs, wh, ww, f"<{threads},{fast}>")
        if pad:
            assert torch.equal(out[len(cs):], out[len(cs):len(cs) + 1].expand(len(pad), -1, -1, -1))
            np.testing.assert_array_equal(out[len(cs)].cpu().numpy(), pad[0].window(wh, ww))


@pytest.mark.parametrize("threads", [1024, 512])
def test_never_resynchronising_stream(threads, hcir_built):
    """Fixed-length codes: no chain ever merges, thread 0's chain decodes the whole stream, the round loop runs to
    about nact (the worst case the kernel's comment describes; bounded by nact rounds).  More than kT / 4 chains
    survive round 1 (the in-place branch), the queue takes over when they thin out at the stream's end."""
    named = jc.cases()
    c = named["sync_never"]
    cs = [c] + ([] if threads == 1024 else [named["tab_dc_one"]] * 383)
    from hcir import jpeg
    wh, ww = 192, 192
    staged = _stage([x.data for x in cs])
    plan = jpeg.plan(staged, (wh, ww))
    print(f"hcir_jpeg_plan: b={len(cs)} -> {plan}")
    assert plan == (threads, False, 4)
    got, staged, geom = _decode_raw([x.data for x in cs], wh, ww)
    np.testing.assert_array_equal(got[0], c.window(wh, ww))
    bits = staged.headers()[0].stream_bits
    S = max(128, (-(-bits // threads) + 31) // 32 * 32)
    nact, rounds = -(-bits // S), int(geom[0, GEOM_ROUNDS])
    print(f"sync_never at {threads} threads: nact {nact}, device rounds {rounds}")
    assert geom[0, 38 - 3:38].tolist() == [3, 192, 192]          # ncomp, width, height: the record is where we read it
    assert nact / 2 <= rounds <= nact and nact > threads // 4
    for i in range(1, len(cs)):
        np.testing.assert_array_equal(got[i], got[1])


# ---- batch behaviour ----------------------------------------------------------------------------------------------------
def test_mixed_batch_equals_single_decodes(hcir_built):
    """Hand-built and Pillow streams, grey and colour, fast and generic tables, a rejected placeholder in the middle:
    every window equals the reference and the window the same file gives when decoded alone."""
    named = jc.cases()
    rng = np.random.default_rng(23)
    pil = [encode_jpeg(synth_jpeg_image(rng, 90, 70), quality=85, subsampling=2),
           encode_jpeg(synth_jpeg_image(rng, 40, 120).convert("L"), quality=70),
           encode_jpeg(synth_jpeg_image(rng, 130, 130), quality=95, subsampling=0, restart_marker_blocks=2)]
    cs = [named[n] for n in ("tab_four", "tab_range16", "sym_extreme", "geo_nact1", "sync_ri3", "dc_ri100",
                             "fmt_fill_rst", "sym_stuffed")] + jc.small_cases()[:4]
    files = [c.data for c in cs[:5]] + pil[:2] + [jc.rejected_cases()[0][1]] + [c.data for c in cs[5:]] + pil[2:]
    hole = 7
    wh, ww = 100, 96
    out, staged = _decode(files, (wh, ww), (1024, False, 4), allow_rejected=True)
    assert staged.rejected == [hole]
    got = out.cpu().numpy()
    assert not got[hole].any()
    refs = {c.data: c.window(wh, ww) for c in cs}
    for f in pil:
        refs[f] = jc.center_window(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), wh, ww)
    from hcir import jpeg
    for i, f in enumerate(files):
        if i == hole:
            continue
        np.testing.assert_array_equal(got[i], refs[f], err_msg=f"file {i} in the batch")
        alone = jpeg.decode_windows(_stage([f]).to("cuda"), (wh, ww), check_status=True)[0].cpu().numpy()
        np.testing.assert_array_equal(got[i], alone, err_msg=f"file {i} alone")
