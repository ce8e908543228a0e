"""CPU tests of the hand-built deflate cases (tests/_deflate_cases.py): streams in forms of RFC 1951 that zlib's
encoder never writes.  Three independent decoders must agree on every one of them: zlib's inflate, the C oracle
(oracle/png_oracle.c) and Pillow; the valid ones must come out as the encoder's model says, the malformed ones must be
refused by all three.  What a case is expected to do is never written down by hand: it is what zlib does with it.
The required-reach test keeps the table from passing vacuously: the encoder counts, while it writes, every form that
REQUIRED_REACH lists, and every count must be above zero over the table."""
import io
import os
import sys
import warnings
import zlib
from collections import Counter

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _deflate_cases as cases  # noqa: E402
import deflate_writer as dw  # noqa: E402


def _pil(data):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", list(cases.VALID))
def test_valid_case_zlib_oracle_pillow_agree(name):
    from oracle import png as op
    file, model, reach = cases.build(name)
    parsed = op.parse(file)
    stream = parsed["idat"]
    assert zlib.decompress(stream) == model
    got, stats = op.inflate(stream, len(model) + 1, stats=True)
    assert got == model
    cut = len(model) * 2 // 3
    assert op.inflate(stream, cut) == model[:cut]  # what a window decode asks for: stop mid-stream
    for k in cases.ORACLE_COUNTERS:  # the oracle saw what the encoder says it wrote
        assert stats[k] == reach.get(k, 0), (k, stats[k], reach.get(k, 0))
    ref = _pil(file)
    stride = 1 + ref.shape[1] * op.bytes_per_pixel(parsed["color_type"])
    assert ref.shape[0] * stride == len(model)  # the stream holds the scanlines and not a byte more
    np.testing.assert_array_equal(op.decode(file), ref)


@pytest.mark.parametrize("name", list(cases.INVALID))
def test_invalid_case_is_refused_by_all_three(name):
    from oracle import png as op
    file, _, _ = cases.build(name)
    stream = op.parse(file)["idat"]
    with pytest.raises(zlib.error, match=cases.ZLIB_SAYS[name]):  # refused for the damage the case is named after
        zlib.decompress(stream)
    with pytest.raises(op.Corrupt):
        op.inflate(stream, 1 << 20)
    with pytest.raises(op.Corrupt):
        op.decode(file)
    with pytest.raises(Exception):  # noqa: B017 - OSError / SyntaxError, whatever Pillow makes of zlib's error
        _pil(file)


@pytest.mark.parametrize("name", [n for n in cases.INVALID if n not in cases.NO_BODY])
def test_invalid_case_has_all_the_bytes_its_image_needs(name):
    """Behind its damage a malformed case holds every scanline of the image it declares, each with a legal filter
    type, as a decoder without validity checks reads them.  A decoder under test that flags the file therefore does
    so for the damage itself: running out of stream before the last scanline, which any decoder reports, cannot stand
    in for the check the case is about."""
    from oracle import png as op
    p = op.parse(cases.build(name)[0])
    stride = 1 + p["width"]
    got = dw.lenient_inflate(p["idat"], p["height"] * stride)
    assert len(got) == p["height"] * stride
    assert max(got[::stride]) <= 4


def test_lenient_inflate_reads_sound_streams_as_zlib_does():
    for name in ("stored_blocks_at_every_bit_offset", "repeat_codes_across_the_table_boundary",
                 "length_258_as_symbol_285_and_as_284_plus_31", "one_distance_code_of_one_bit"):
        file, model, _ = cases.build(name)
        from oracle import png as op
        assert dw.lenient_inflate(op.parse(file)["idat"], len(model) + 1) == model


def test_required_reach_is_complete():
    total = Counter()
    where = {}
    for name in cases.VALID:
        reach = cases.build(name)[2]
        total.update(reach)
        for k, v in reach.items():
            if v > where.get(k, ("", 0))[1]:
                where[k] = (name, v)
    missing = [(what, k) for what, keys in cases.REQUIRED_REACH.items() for k in keys if total[k] <= 0]
    assert not missing, missing
    for what, keys in cases.REQUIRED_REACH.items():
        print(what, "<-", {k: where[k][0] for k in keys})


def test_model_and_writer_basics():
    """The writer's own pieces against zlib: canonical codes (the fixed code's known values, RFC 1951 3.2.6), the
    length-limited Huffman and the deep profile give complete sets, the three header styles give the same bytes."""
    codes = dw.canonical_codes(dw.FIXED_LIT)
    rev = lambda c, n: int(format(c, "0%db" % n)[::-1], 2)  # noqa: E731
    assert codes[0] == (rev(0b00110000, 8), 8) and codes[144] == (rev(0b110010000, 9), 9)
    assert codes[256] == (0, 7) and codes[280] == (rev(0b11000000, 8), 8)
    kraft = lambda lens: sum(2.0 ** -l for l in lens if l)  # noqa: E731
    rng = np.random.default_rng(0)
    for n, maxbits in ((286, 15), (30, 15), (19, 7), (286, 9)):
        f = [int(v) for v in (rng.integers(0, 1000, n) ** 3) // 10 ** 6 + 1]  # skewed: the limit is reached
        lens = dw.huffman_lengths(f, maxbits)
        assert kraft(lens) == 1.0 and max(lens) <= maxbits and min(lens) >= 1
    lens = dw.deep_lengths(286, [0, 1, 2, 3, 4, 256], [])
    assert [lens[s] for s in (0, 1, 2, 3, 4, 256)] == [11, 12, 13, 14, 15, 11] and kraft(lens) == 1.0
    chain = dw.fill_lengths(20, {0: 11, 1: 12, 2: 13, 3: 14, 4: 15, 5: 15}, [], range(6, 20))
    assert sorted(l for l in chain if l) == list(range(1, 16)) + [15]  # 1, 2, ... 14, 15, 15
    sc = dw.Script(3).lits(500)
    for k in range(60):
        sc.match(3 + k, 1 + 7 * k).lit()
    model = None
    for style in ("none", "cross", "split"):
        for hclen in ("min", "full"):
            blocks = [dw.Block("dynamic", sc.syms + [dw.EOB], header=dw.Header(rle=style, hclen=hclen))]
            z, m, _, _ = dw.zlib_stream(blocks)
            assert zlib.decompress(z) == m and (model is None or m == model)
            model = m
    toks = dw.tokenize(model, [1, 2, 3, 4, 64])
    assert dw.interpret([dw.Block("fixed", toks + [dw.EOB])]) == model
