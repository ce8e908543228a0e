"""GPU tests of the device PNG decoder (csrc/png.hip) on the hand-built deflate cases (tests/_deflate_cases.py): forms
of RFC 1951 that zlib's encoder never writes - long codes on every alphabet, one or no distance code, repeat codes
across the table boundary, runs of one-bit codes, distances at 32768 across the ring wrap, stored blocks at every bit
offset, blocks of end-of-block only - and the malformed headers and symbols a decoder must refuse.  Bar: byte-equal to
Pillow (test_png_deflate_host.py holds zlib, the C oracle and Pillow to one another on the same files), status 0 for
every valid case and -1 for every invalid one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _deflate_cases as cases  # noqa: E402
from png_writer import write_png  # noqa: E402
from test_png_gpu import _pil, _window, streams  # noqa: E402,F401 - the golden fixture and the CenterCrop reference

pytestmark = pytest.mark.gpu

GOLDEN_NEIGHBOURS = ("filter4_rgb", "mixed_blocks", "grey_l1", "palette", "far_matches", "small_100x80")


def _decode(files, size=224):
    """(windows, status, staged): status is read, not checked, so that a test can say which file was flagged."""
    from hcir import png
    staged = png.stage_batch(files)
    out, st = png.decode_windows(staged.to("cuda"), size, return_status=True)
    return out.cpu().numpy(), st.cpu().tolist(), staged


def _launch(L, files, wh=224, ww=224):
    """The C ABI, as a caller that looks at the status vector itself."""
    from hcir import png
    staged = png.stage_batch(files)
    assert staged.rejected == []
    st = torch.zeros(len(files), dtype=torch.int32, device="cuda")
    out = torch.empty((len(files), wh, ww, 3), dtype=torch.uint8, device="cuda")
    dev = staged.to("cuda")
    ws = torch.empty(L.hcir_png_workspace_bytes(staged._host_headers.data_ptr(), staged.b, wh, ww), dtype=torch.uint8,
                     device="cuda")
    rc = L.hcir_png_decode_window_u8(dev.blob.data_ptr(), staged._host_headers.data_ptr(), staged.b, wh, ww,
                                     out.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, st.cpu().tolist(), out.cpu().numpy(), dev


@pytest.mark.parametrize("name", list(cases.VALID))
def test_valid_case_alone(name, hcir_built):
    file = cases.build(name)[0]
    ref = _pil(file)
    got, st, staged = _decode([file], ref.shape[:2])  # window = image: the whole stream is decoded
    assert staged.rejected == [] and st == [0]
    np.testing.assert_array_equal(got[0], ref)
    got, st, _ = _decode([file], 224)
    assert st == [0]
    np.testing.assert_array_equal(got[0], _window(ref, 224, 224))


def test_all_valid_cases_in_one_batch_with_golden_neighbours(streams, hcir_built):
    names, files, wins = streams
    batch, want = [], []
    gold = [names.index(n) for n in GOLDEN_NEIGHBOURS]
    for k, name in enumerate(cases.VALID):
        file = cases.build(name)[0]
        batch.append(file)
        want.append((name, _window(_pil(file), 224, 224)))
        if k % 4 == 0:
            g = gold[(k // 4) % len(gold)]
            batch.append(files[g])
            want.append((names[g], wins[g]))
    a, st, staged = _decode(batch)
    b, st2, _ = _decode(batch)
    assert staged.rejected == [] and st == [0] * len(batch) and st2 == st
    np.testing.assert_array_equal(a, b)
    for k, (name, w) in enumerate(want):
        np.testing.assert_array_equal(a[k], w, err_msg=f"{k}: {name}")


def test_invalid_cases_are_flagged_not_fatal(streams, hcir_built):
    from hcir import png
    names, files, wins = streams
    g0, g1 = names.index("filter4_rgb"), names.index("grey_l1")
    bad = [cases.build(name)[0] for name in cases.INVALID]
    rc, st, out, dev = _launch(hcir_built, [files[g0]] + bad + [files[g1]])
    assert rc == 0
    assert st[0] == 0 and st[-1] == 0
    wrong = [(name, st[1 + k]) for k, name in enumerate(cases.INVALID) if st[1 + k] != -1]
    assert not wrong, wrong
    np.testing.assert_array_equal(out[0], wins[g0])
    np.testing.assert_array_equal(out[-1], wins[g1])
    with pytest.raises(png.HcirError, match="corrupt"):
        png.decode_windows(dev, 224, check_status=True)


def test_small_window_stops_early(hcir_built):
    """An 8 x 8 window of the 600-row case needs rows 0..303.  The file's stream is cut off at three quarters of its
    length: the decoder must stop once it has the rows it needs (status 0, window byte-equal to the whole file's), and
    must flag the same file when the window is the whole image."""
    from oracle import png as op
    file, model, _ = cases.build(cases.TALL)
    ref = _pil(file)
    h, w = ref.shape[:2]
    stream = op.parse(file)["idat"]
    cut = stream[:len(stream) * 3 // 4]
    y0, y1 = op.window_rows(h, 8)
    assert y1 == 304 and op.inflate(cut, y1 * (w + 1)) == model[:y1 * (w + 1)]  # the rows needed are all there
    short = write_png(np.zeros((h, w, 1), np.uint8), 0, zstream=cut)
    got, st, _ = _decode([file, short], (8, 8))
    assert st == [0, 0]
    np.testing.assert_array_equal(got[0], _window(ref, 8, 8))
    np.testing.assert_array_equal(got[1], _window(ref, 8, 8))
    _, st, _ = _decode([file, short], (h, w))
    assert st == [0, -1]
