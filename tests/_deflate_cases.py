"""The case table of the hand-built deflate tests: PNG files whose zlib streams use forms of RFC 1951 that zlib's own
encoder never writes (tests/deflate_writer.py).  Test infrastructure, shared by test_png_deflate_host.py (zlib, the C
oracle and Pillow must agree on every case) and test_png_deflate_gpu.py (the device decoder against them).

VALID maps a name to a builder that returns (file bytes, model output, reach): the model output is what the symbol
lists stand for (deflate_writer.interpret), reach is what the encoder counted while it wrote.  INVALID maps a name to
a builder of a malformed file (model None): damage in the first block, which every decoder must refuse.

Two kinds of content.  Scripted symbols: 8-bit grey with every byte in 0..4, so every byte is a legal filter type
wherever the rows fall and the script places its symbols by output position alone; all five filters run on the
content, so a wrong inflated byte changes pixels.  Scripted tokenizer: real scanlines with all 256 byte values
(png_writer.filter_rows of synth_image, grey and RGB), matched at a fixed list of candidate distances and coded with
the deep profiles.
"""
from __future__ import annotations

from collections import Counter
from functools import lru_cache
from typing import Callable, Dict

import numpy as np

from deflate_writer import (EOB, DBASE, DEXT, GRID_DISTS, GRID_LENGTHS, LBASE, LEXT, Block, Header, RawBits, RawDist,
                            RawLit, Script, deep_lengths, fill_lengths, huffman_lengths, short_literal_lengths,
                            symbol_frequencies, tokenize, zlib_stream)
from png_writer import filter_rows, synth_image, write_png

LIT5 = [0, 1, 2, 3, 4]
W = 63  # scripted cases: 64-byte scanlines unless a case needs room


def _png(z: bytes, w: int, h: int, color_type: int = 0, idat_sizes=None) -> bytes:
    c = {0: 1, 2: 3}[color_type]
    return write_png(np.zeros((h, w, c), np.uint8), color_type, zstream=z, idat_sizes=idat_sizes)


def _rows(sc: Script, w: int = W) -> Script:
    """Literals up to the end of the scanline the script stands in."""
    stride = w + 1
    return sc.lits_to(-(-sc.pos // stride) * stride)


def _pack(sc: Script, w: int = W, idat_sizes=None):
    z, model, reach, _ = zlib_stream(sc.blocks)
    assert len(model) % (w + 1) == 0 and model
    return _png(z, w, len(model) // (w + 1), idat_sizes=idat_sizes), model, reach


def _pad_symbols(n, taken):
    return [s for s in range(n) if s not in taken]


# ---------------------------------------------------------------------------------------------------------- valid

def literal_codes_11_to_15_bits():
    sc = _rows(Script(1).lits(1000))
    lit = deep_lengths(286, LIT5, [EOB])
    return _pack(sc.end(lit_lens=lit, dist_lens=[0]))


def distance_codes_9_to_15_bits():
    sc = Script(2).lits(40)
    for rep in range(6):
        for ds in range(8):  # distance symbols 0..7: distances 1..16
            sc.match(3 + (7 * rep + ds) % 30, DBASE[ds] + (rep % (1 << DEXT[ds]))).lit()
    dist = deep_lengths(30, range(8), [], lo=9)
    return _pack(_rows(sc).end(dist_lens=dist))


def length_codes_11_to_15_bits():
    sc = Script(3).lits(30)
    deep = [257, 258, 265, 270, 285]
    for rep in range(5):
        for ls in deep:
            i = ls - 257
            sc.match(LBASE[i] + rep % (1 << LEXT[i]), 1 + (rep * 5 + i) % 29).lits(2)
    lit = deep_lengths(286, deep, LIT5 + [EOB])
    return _pack(_rows(sc).end(lit_lens=lit))


def end_of_block_codes_11_13_15_bits():
    sc = Script(4)
    for bits in (11, 13, 15):
        sc.lits(100).match(5, 3)
        if bits == 15:
            _rows(sc)
        sc.end(lit_lens=fill_lengths(286, {EOB: bits}, LIT5 + [259], _pad_symbols(286, LIT5 + [259, EOB])))
    return _pack(sc)


def long_code_behind_a_literal():
    """Short literal, then a 12/13-bit literal, a 14-bit length symbol, a 15-bit end-of-block: the pair lookup sees a
    literal in front of each and must not take the long code's first ten bits for a second literal."""
    sc = Script(5)
    fixed = {1: 12, 3: 13, 257: 14, EOB: 15}
    lit = fill_lengths(286, fixed, [0, 2, 4], _pad_symbols(286, [0, 2, 4] + list(fixed)))
    for blk in range(3):
        for k in range(120):
            sc.lit((0, 2, 4)[k % 3]).lit((1, 3)[k % 2])
            if k % 4 == 3:
                sc.lit((0, 2, 4)[k % 3]).match(3, 1 + k % 7)
        sc.lit(0)
        if blk == 2:
            _rows(sc)
        sc.end(lit_lens=lit)
    return _pack(sc)


def one_distance_code_of_one_bit():
    sc = Script(6).lits(20)
    for n in (3, 4, 5, 17, 64, 130, 258):
        sc.match(n, 4).lit()
    sc.end(dist_lens=[0, 0, 0, 1])
    for n in (3, 9, 33, 258):
        sc.match(n, 5).lit().match(n, 6).lit()  # symbol 4: one extra bit behind the single code
    return _pack(_rows(sc).end(dist_lens=[0, 0, 0, 0, 1]))


def zero_distance_codes():
    return _pack(_rows(Script(7).lits(700)).end(dist_lens=[0]))


def fixed_block_full_table():
    """Every length symbol 257..285 and every distance symbol 0..29 of the fixed code, each with its extra bits all
    zeros and all ones (symbol 29 with all ones: distance 32768)."""
    w = 255
    sc = Script(8).stored(32768)
    for ones in (0, 1):
        for i in range(30):
            li, di = i % 29, i
            sc.match(LBASE[li] + ones * ((1 << LEXT[li]) - 1), DBASE[di] + ones * ((1 << DEXT[di]) - 1), 257 + li).lit()
        sc.match(258, 9).lit()  # symbol 285, which i % 29 reaches only once
    return _pack(_rows(sc, w).end("fixed"), w)


def length_258_as_symbol_285_and_as_284_plus_31():
    sc = Script(9).lits(300)
    for kind in ("fixed", "dynamic"):
        for d in (1, 7, 300):
            sc.match(258, d).lit().match(258, d, 284).lit()
        sc.match(257, 2).lit()
        if kind == "dynamic":
            _rows(sc)
        sc.end(kind)
    return _pack(sc)


def distances_1_to_130_times_lengths():
    """Every distance 1..130 with lengths 3, 4, 63, 64, 65, 127, 128, 129, 257, 258: the overlapping copies
    (lane mod dist) and the 64-byte chunks of a copy; two fresh literals between matches keep the content moving."""
    w = 255
    sc = Script(10).lits(130)
    for d in GRID_DISTS:
        for n in GRID_LENGTHS:
            sc.match(n, d).lits(2)
    return _pack(_rows(sc, w).end(), w)


def distance_32768_and_just_below():
    """Distances 32768 - j, j = 0..8, whose batch must take the ordered path: with distance + length > 32768 the
    source's ring slot is overwritten by the copy itself."""
    w = 255
    sc = Script(11).stored(20000).lits(2000)
    while sc.pos < 32768 + 40:
        sc.match(37, 1 + sc.pos % 900).lits(3)
    sc.end()
    for j in range(9):
        for n in (3, 10, 64, 65, 258):
            sc.match(max(n, j + 1), 32768 - j).lits(1 + j % 3)
    return _pack(_rows(sc, w).end(), w)


def ring_wrap_flush_units_far_matches_stored_65535():
    """The large case: a stored block of 65535 bytes, then far matches (32768 - j) that straddle output positions
    65536 and 98304 (the ring wraps) and the multiples of 1024 between them (the flush unit), near matches at the same
    places, and a stored block as the last one."""
    w = 511
    sc = Script(12).stored(65535)
    sc.lit().end("fixed")                      # output position 65536 exactly
    sc.lits(7)
    j = 0
    while sc.pos < 98304 + 3000:
        nxt = (sc.pos // 1024 + 1) * 1024      # next flush-unit boundary (every 32nd is a ring wrap)
        room = nxt - sc.pos
        if room > 300:
            sc.match(258, 32768 - j % 9).lit()                 # filler: far matches all the way
        else:
            n = (3, 4, 64, 65, 130, 258)[j % 6]
            sc.lits_to(nxt - 1 - min(j % min(n - 1, 60), room - 1))
            if j % 3 == 2:
                sc.match(n, 1 + j % 70)                         # a near, overlapping match across the boundary
            else:
                sc.match(max(n, j % 9 + 1), 32768 - j % 9)      # a far one: the ordered path across the boundary
            sc.lits(2)
        j += 1
    sc.end()
    stride = w + 1
    sc.stored(-sc.pos % stride or stride)
    return _pack(sc, w)


def matches_straddle_1024_small():
    sc = Script(13).lits(900)
    for k, n in enumerate((3, 4, 31, 64, 65, 129, 258) * 2):
        nxt = (sc.pos // 1024 + 1) * 1024
        sc.lits_to(nxt - 1 - k % min(n - 1, 9)).match(n, (1, 2, 64, 65, 700)[k % 5]).lits(5)
    return _pack(_rows(sc).end())


def runs_of_one_and_two_bit_codes():
    """1500 one-bit literals; 1500 two-bit literals; 1100 x (one-bit literal, match of 3 at distance 1: two and one
    bits): more symbol starts in a 256-bit pass than the symbol queue has room for."""
    lit, dist = short_literal_lengths()
    sc = Script(14).lits(40).lits(1500, 1).lits(30).end(lit_lens=lit, dist_lens=dist)
    two = [0] * 257
    for s, l in ((0, 2), (1, 2), (2, 2), (3, 3), (4, 4), (EOB, 4)):
        two[s] = l
    sc.lits(20)
    for _ in range(1500):
        sc.lit(int(sc.rng.integers(0, 3)))
    sc.lits(20).end(lit_lens=two, dist_lens=[0])
    sc.lits(10)
    for _ in range(1100):
        sc.lit(1).match(3, 1)
    sc.lits(25)
    return _pack(_rows(sc).end(lit_lens=lit, dist_lens=dist))


def blocks_of_end_of_block_only():
    """Twenty fixed and twenty dynamic blocks that hold only end-of-block, in front of, between and behind data
    blocks; the dynamic ones both with the single 1-bit code (an incomplete set zlib allows) and with a complete set."""
    single = dict(lit_lens=[0] * 256 + [1], dist_lens=[0])
    full = dict(lit_lens=[1] + [0] * 255 + [1], dist_lens=[0])
    sc = Script(15).empty("fixed", 20).empty("dynamic", 20, **single)
    sc.lits(200).match(40, 7).end("fixed")
    sc.empty("dynamic", 10, **full).empty("fixed", 20).empty("dynamic", 10, **single)
    _rows(sc.lits(100).match(30, 250)).end()
    sc.empty("fixed", 10).empty("dynamic", 20, **full)
    return _pack(sc)


def stored_blocks_at_every_bit_offset():
    """Stored blocks whose 3-bit header starts at each of the 8 bit offsets, pad bits all ones; LEN 0; stored last.
    Behind a stored block the stream is byte aligned; fixed blocks of 10 bits (end-of-block only) and 23 bits (one
    match at distance 5 + end-of-block) move the next header to the offset wanted."""
    sc = Script(16).stored(70, pad=0xff)
    for k in (2, 4, 6, 7, 1, 3, 5, 0):
        if k % 2:
            sc.match(3, 5).end("fixed")
        sc.empty("fixed", (k - 7 * (k % 2)) % 8 // 2)
        sc.stored(0 if k == 4 else 40 + k, pad=0xff)
    sc.lits(50).end()
    stride = W + 1
    sc.stored(-sc.pos % stride or stride, pad=0xff)
    return _pack(sc)


_BOUNDARY_LIT = {0: 2, 1: 2, 2: 3, 3: 3, 4: 4, EOB: 4, 257: 4, 258: 4}


def _boundary_lens():
    lit = [0] * 259
    for s, l in _BOUNDARY_LIT.items():
        lit[s] = l
    return lit


def repeat_codes_across_the_table_boundary():
    """Code 16 repeating the last literal/length length into the distance lengths, code 18 running from the zeros
    behind the last length symbol into the zeros in front of the first distance code; the same tables once more with
    the runs broken at the boundary, and once with no repeat codes at all."""
    lit = _boundary_lens()
    sc = Script(17).lits(260)
    for k in range(40):
        sc.match(3 + k % 2, 1 + (k * 13) % 250).lit()
    sc.end(lit_lens=lit, dist_lens=[4] * 16, header=Header(rle="cross"))
    far = [0] * 10 + [2] * 4   # distance symbols 10..13: 33..128
    for k in range(40):
        sc.match(3 + k % 2, 33 + (k * 7) % 96).lit()
    sc.end(lit_lens=lit, dist_lens=far, header=Header(rle="cross", hlit=286))
    for style in ("split", "none"):
        for k in range(20):
            sc.match(3 + k % 2, 1 + (k * 11) % 250).lit()
        if style == "none":
            _rows(sc)
        sc.end(lit_lens=lit, dist_lens=[4] * 16, header=Header(rle=style))
    return _pack(sc)


def hclen_5_and_hclen_19():
    """HCLEN 5 is the smallest count a valid block can have (16, 17, 18, 0 and 8 are sent: every code 8 bits, so 256
    literal/length codes of 8 bits and no distance code; HCLEN 4 cannot name a non-zero length and is in the invalid
    family).  HCLEN 19 with zeros behind the last code-length code that is used."""
    sc = _rows(Script(18).lits(300))
    sc.end(lit_lens=[8] * 255 + [0, 8], dist_lens=[0], header=Header(rle="none"))
    sc.lits(100).match(20, 33)
    return _pack(_rows(sc).end(header=Header(hclen="full")))


def hlit_257_286_hdist_1_30():
    sc = Script(19).lits(200).end(dist_lens=[0])                      # HLIT 257, HDIST 1
    sc.lits(30).match(9, 100).match(258, 1)
    return _pack(_rows(sc).end(header=Header(hlit=286, hdist=30)))


def match_source_in_an_earlier_block_of_another_type():
    sc = Script(20).stored(200)
    sc.match(30, 200).lit().match(100, 150).end("fixed")              # from the stored block
    sc.match(50, 120).lits(3).match(258, 330).end()                   # from the fixed and the stored block
    sc.stored(77)
    sc.match(60, 70).match(40, 500)                                   # from the second stored block and the fixed one
    _rows(sc).end("fixed")
    return _pack(sc)


def idats_cut_through_header_and_first_symbols():
    """The long-code case again, its stream cut into IDATs of 1, 0, 3, 7, ... bytes through the zlib header, the
    dynamic block header and the first symbols."""
    sc = Script(5)
    fixed = {1: 12, 3: 13, 257: 14, EOB: 15}
    lit = fill_lengths(286, fixed, [0, 2, 4], _pad_symbols(286, [0, 2, 4] + list(fixed)))
    for k in range(400):
        sc.lit(k % 5)
        if k % 9 == 8:
            sc.match(3, 1 + k % 8)
    _rows(sc).end(lit_lens=lit)
    z, model, reach, marks = zlib_stream(sc.blocks)
    upto = 2 + (marks["first_symbols_end_bit"] + 7) // 8
    sizes, total = [], 0
    while total < upto + 8:
        s = (1, 0, 3, 7, 1, 1, 0, 0, 2, 5)[len(sizes) % 10]
        sizes.append(s)
        total += s
    reach = Counter(reach)
    reach["idat_cuts_in_header_and_first_symbols"] = sum(1 for i in range(len(sizes)) if sum(sizes[:i + 1]) <= upto)
    return _png(z, W, len(model) // (W + 1), idat_sizes=sizes), model, reach


def _tokenized(seed: int, h: int, w: int, c: int):
    rng = np.random.default_rng(seed)
    img = synth_image(rng, h, w, c, "mixed")
    raw = filter_rows(img, [int(v) for v in rng.integers(0, 5, h)])
    stride = 1 + w * c
    cands = [1, 2, 3, 4, stride, 2 * stride, 3 * stride, 32768, 32768 // stride * stride]
    syms = tokenize(raw, list(dict.fromkeys(cands))) + [EOB]
    lf, df = symbol_frequencies(syms)
    used_l = sorted((s for s in range(286) if lf[s]), key=lambda s: -lf[s])
    lits, lens = [s for s in used_l if s < 256], [s for s in used_l if s > 256]
    deep_l = lits[-5:] + lens[-4:] + [EOB] + lits[-12:-5]       # the rarest literals and length symbols, end-of-block
    lit = deep_lengths(286, deep_l, used_l)
    used_d = sorted((s for s in range(30) if df[s]), key=lambda s: -df[s])
    dist = deep_lengths(30, used_d[:7], used_d, lo=9)           # the commonest distance symbols: 9 to 15 bits
    z, model, reach, _ = zlib_stream([Block("dynamic", syms, lit_lens=lit, dist_lens=dist)])
    assert model == raw
    return _png(z, w, h, {1: 0, 3: 2}[c]), model, reach


def tokenized_grey_tall_deep_codes():
    return _tokenized(21, 600, 63, 1)


def tokenized_rgb_deep_codes():
    return _tokenized(22, 110, 120, 3)


VALID: Dict[str, Callable] = {f.__name__: f for f in (
    literal_codes_11_to_15_bits, distance_codes_9_to_15_bits, length_codes_11_to_15_bits,
    end_of_block_codes_11_13_15_bits, long_code_behind_a_literal, one_distance_code_of_one_bit, zero_distance_codes,
    fixed_block_full_table, length_258_as_symbol_285_and_as_284_plus_31, distances_1_to_130_times_lengths,
    distance_32768_and_just_below, ring_wrap_flush_units_far_matches_stored_65535, matches_straddle_1024_small,
    runs_of_one_and_two_bit_codes, blocks_of_end_of_block_only, stored_blocks_at_every_bit_offset,
    repeat_codes_across_the_table_boundary, hclen_5_and_hclen_19, hlit_257_286_hdist_1_30,
    match_source_in_an_earlier_block_of_another_type, idats_cut_through_header_and_first_symbols,
    tokenized_grey_tall_deep_codes, tokenized_rgb_deep_codes)}
TALL = "tokenized_grey_tall_deep_codes"  # 600 rows: a small window needs only the upper half of its stream

# One entry per bullet of the valid family: the reach keys that show it was written.  Every key must be counted at
# least once over the whole table.
REQUIRED_REACH = {
    "literal codes of 11 to 15 bits": ["lit_code_bits_%d" % b for b in range(11, 16)],
    "distance codes of 9 to 15 bits": ["dist_code_bits_%d" % b for b in range(9, 16)],
    "length symbols with long codes": ["len_code_bits_%d" % b for b in range(11, 16)],
    "end-of-block code longer than 10 bits": ["eob_code_bits_11", "eob_code_bits_13", "eob_code_bits_15"],
    "long-coded symbol directly behind a literal": ["long_code_behind_short_literal"],
    "exactly one distance code of length 1": ["one_dist_code_len1"],
    "zero distance codes": ["zero_dist_codes"],
    "the fixed block's full table": ["fixed_every_length_symbol", "fixed_every_distance_symbol",
                                     "fixed_extra_bits_all_ones_everywhere", "fixed_extra_bits_all_zeros_everywhere"],
    "258 as symbol 285 and as 284 + 31": ["len258_sym285", "len258_sym284"],
    "distances 1..130 x lengths": ["every_distance_1_to_130_at_every_grid_length"],
    "distance 32768 and 32768 - j on the ordered path": ["dist_32768", "dist_32760_to_32767", "resolve_ordered"],
    "the same across the ring wrap and the flush unit": ["resolve_ordered_straddles_32768",
                                                         "resolve_ordered_straddles_1024", "match_straddles_32768",
                                                         "match_straddles_1024"],
    "runs of 1024 one- and two-bit symbols": ["run_of_1024_one_bit_literals", "run_of_1024_two_bit_literals",
                                              "run_of_1024_one_bit_literal_then_short_match"],
    "blocks that hold only end-of-block": ["eob_only_fixed_blocks", "eob_only_dynamic_blocks",
                                           "twenty_eob_only_blocks_in_a_row", "empty_block_before_data",
                                           "empty_block_between_data", "empty_block_behind_data"],
    "stored blocks": ["stored_len_0", "stored_len_65535", "stored_nonzero_pad_bits", "stored_as_last_block"] +
                     ["stored_header_at_bit_%d" % k for k in range(8)],
    "repeat codes across the literal/distance boundary": ["rep16_cross", "rep18_cross", "rep_split_at_boundary",
                                                          "rle_none"],
    "HCLEN smallest and 19 with trailing zeros": ["hclen_5", "hclen_19_trailing_zeros"],
    "HLIT 257 and 286, HDIST 1 and 30": ["hlit_257", "hlit_286", "hdist_1", "hdist_30"],
    "match whose source lies in a block of another type": ["match_source_in_block_of_other_type"],
    "IDATs of 1, 0, 3, 7 bytes through header and first symbols": ["idat_cuts_in_header_and_first_symbols"],
}
# counters of oracle.png.inflate(..., stats=True) that the encoder keeps too
ORACLE_COUNTERS = ("long_codes", "codes_gt_11", "codes_gt_12", "overlapping", "dist_gt_16k", "stored_blocks",
                   "fixed_blocks", "dynamic_blocks", "literals", "matches")


# -------------------------------------------------------------------------------------------------------- invalid
# Every malformed file declares 63 x 32 grey (2048 bytes of scanlines) unless it says otherwise, and behind its damage
# carries a body that a decoder WITHOUT the check in question would read as at least that many bytes: the body is
# coded with the very (malformed) code lengths, canonically, as such a decoder would build them.  So a decoder that
# flags the file does so for the damage and not because the stream ran out before the last scanline.  Exceptions, by
# their nature: the truncated streams, block type 3, and HCLEN 4 (no length but zero can be named at all).  What a
# decoder without a check would do is not defined everywhere (an over-subscribed set, symbols 286 / 287); the bodies
# follow the canonical reading, first code first.

NEED = 32 * (W + 1)


def _bad(blocks, cut=None, w=W, h=32):
    z = zlib_stream(blocks)[0]
    return _png(z if cut is None else z[:cut], w, h), None, {}


def _lens(n, **kw):
    v = [0] * n
    for k, l in kw.items():
        v[int(k[1:])] = l
    return v


def _body(seed, n=NEED, lits=LIT5, dists=(1, 2)):
    """n bytes of seeded literals from `lits` and, when `dists` is not empty, matches of length 3 at those distances
    (length symbol 257, distance symbols 0 and 1: all that the damaged tables below need to hold)."""
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < n:
        if dists and pos >= 8 and n - pos >= 3 and rng.random() < 0.2:
            out.append((3, int(dists[int(rng.integers(0, len(dists)))])))
            pos += 3
        else:
            out.append(int(lits[int(rng.integers(0, len(lits)))]))
            pos += 1
    return out


_OK_LIT = _lens(258, s0=2, s1=2, s2=3, s3=3, s4=3, s256=4, s257=4)   # complete: 2/4 + 3/8 + 2/16


def _dyn(seed, lit=_OK_LIT, dist=(1, 1), eob=True, **body):
    """A dynamic first block with the code lengths given (sound ones unless the case is about them) and a full body."""
    return _bad([Block("dynamic", _body(seed, **body) + [EOB] * eob, lit_lens=lit, dist_lens=list(dist))])


def _hdr(seed, lit=_OK_LIT, dist=(1, 1), body=None, **kw):
    """The same with sound tables and the damage in how the header is written (Header fields)."""
    return _bad([Block("dynamic", _body(seed, **(body or {})) + [EOB], lit_lens=lit, dist_lens=list(dist),
                       header=Header(**kw))])


def _cl(seed, syms, lit=_OK_LIT, dist=(1, 1), cl=None, body=None, **kw):
    """The code-length sequence written symbol by symbol as given ((symbol, extra value) pairs); `lit` and `dist` are
    the lengths a decoder without the check would take from it, which the body is coded with.  cl: the code-length
    code's own lengths; None: a Huffman code for the symbols the sequence uses."""
    if cl is None:
        f = [0] * 19
        for s, _ in syms:
            f[s] += 1
        cl = huffman_lengths(f, 7)
    return _hdr(seed, lit, dist, body, cl_lens=cl, cl_syms=syms, **kw)


def _plain(lens):
    return [(l, 0) for l in lens]


_LIT_256x8 = [8] * 255 + [0, 8]          # literals 0..254 and end-of-block, eight bits each: complete
_LIT_257x9 = [9] * 257                   # what a single code-length code (9) can say: far from complete
_NO_012 = _lens(258, s3=1, s4=2, s256=3, s257=3)   # repeat 16 first, previous length taken as 0: symbols 0..2 get none


def _bad_symbol(kind, seed, front, bad):
    """`front` sound symbols, the bad ones, then a whole image's worth of literals: whatever a decoder without the
    check makes of the bad symbols, it has the bytes it needs."""
    return _bad([Block(kind, front + bad + _body(seed, dists=()) + [EOB],
                       **({} if kind == "fixed" else dict(lit_lens=_OK_LIT, dist_lens=[1])))])


def _far_fixed_distance(sym):
    """Distance symbol 30 / 31 of the fixed code with more than 32768 bytes in front: whatever distance a decoder made
    of it would be in reach."""
    sc = Script(32).lits(33000)
    tail = [RawLit(257), RawDist(sym, 0x155, 13)] + [int(v) for v in sc.rng.integers(0, 5, 130 * 256 - 33003)]
    return _bad([Block("fixed", sc.syms + tail + [EOB])], w=255, h=130)


INVALID: Dict[str, Callable] = {
    "oversubscribed_literal_set": lambda: _dyn(40, _lens(257, s0=1, s1=1, s2=2, s3=2, s4=2, s256=2), dists=()),
    "oversubscribed_distance_set": lambda: _dyn(41, dist=[1, 1, 1]),
    "oversubscribed_code_length_set": lambda: _cl(42, _plain(_LIT_256x8 + [0]), _LIT_256x8, [0],
                                                  cl=_lens(19, s0=1, s8=1, s9=1), body=dict(dists=())),
    "incomplete_literal_set": lambda: _dyn(43, _lens(258, s0=2, s1=3, s2=3, s3=3, s4=3, s256=4, s257=4)),
    # (a block of end-of-block only; the body follows in a sound second block)
    "incomplete_literal_set_single_2_bit_code": lambda: _bad([
        Block("dynamic", [EOB], lit_lens=_lens(257, s256=2), dist_lens=[0]), Block("fixed", _body(44) + [EOB])]),
    "incomplete_distance_set_two_2_bit_codes": lambda: _dyn(45, dist=[2, 2]),
    "incomplete_distance_set_single_2_bit_code": lambda: _dyn(46, dist=[2], dists=(1,)),
    # one code-length code only: every length is 9, which no complete set can be made of (the two-code case below is)
    "incomplete_code_length_set_single_code": lambda: _cl(47, _plain(_LIT_257x9 + [9]), _LIT_257x9, [9],
                                                          cl=_lens(19, s9=1), body=dict(dists=())),
    "incomplete_code_length_set": lambda: _cl(48, _plain(_LIT_256x8 + [0]), _LIT_256x8, [0],
                                              cl=_lens(19, s0=2, s8=2), body=dict(dists=())),
    "no_end_of_block_code": lambda: _dyn(49, _lens(258, s0=2, s1=2, s2=2, s3=3, s4=4, s257=4), eob=False),
    # HCLEN 4 sends 16, 17, 18 and 0 only: no length but zero can be named, so no end-of-block code either
    "hclen_4_cannot_name_a_length": lambda: _bad([Block(
        "dynamic", [EOB], lit_lens=_OK_LIT, dist_lens=[1, 1],
        header=Header(cl_lens=_lens(19, s0=1, s18=1), hclen=4, cl_syms=[(18, 127), (18, 111)]))]),
    "repeat_16_as_first_length": lambda: _cl(50, [(16, 0)] + _plain(_NO_012[3:] + [1, 1]), _NO_012,
                                             body=dict(lits=[3, 4])),
    # the last repeat asks for 11 / 6 lengths where 3 are left: a decoder that clamps it reads sound tables
    "repeat_18_overruns_hlit_plus_hdist": lambda: _cl(51, _plain(_OK_LIT + [1, 1]) + [(18, 0)], hdist=5),
    "repeat_16_overruns_hlit_plus_hdist": lambda: _cl(52, _plain(_OK_LIT + [2]) + [(16, 3)], dist=[2, 2, 2, 2]),
    # 287 / 288 length and 31 / 32 distance lengths, all of them sent: well formed but for the count itself
    "hlit_field_30": lambda: _hdr(53, hlit=287),
    "hlit_field_31": lambda: _hdr(54, hlit=288),
    "hdist_field_30": lambda: _hdr(55, hdist=31),
    "hdist_field_31": lambda: _hdr(56, hdist=32),
    "unused_bit_of_single_distance_code": lambda: _bad_symbol("dynamic", 57, _body(1, 60, dists=()),
                                                              [RawLit(257), RawBits(1, 1)]),
    # (a distance code behind it, for a decoder that takes 286 / 287 for one more length symbol)
    "fixed_literal_symbol_286": lambda: _bad_symbol("fixed", 58, [0, 1], [RawLit(286), RawDist(0)]),
    "fixed_literal_symbol_287": lambda: _bad_symbol("fixed", 59, [0, 1], [RawLit(287), RawDist(0)]),
    "fixed_distance_symbol_30": lambda: _far_fixed_distance(30),
    "fixed_distance_symbol_31": lambda: _far_fixed_distance(31),
    "distance_before_the_start_fixed": lambda: _bad_symbol("fixed", 60, [0, 1, 2], [(3, 4)]),
    "distance_before_the_start_dynamic": lambda: _bad([Block("dynamic", [0] * 40 + [(5, 32768)] + _body(61) + [EOB])]),
    "stored_len_nlen_mismatch": lambda: _bad([Block("stored", data=bytes(NEED), nlen_field=0xf7fe)]),
    "stream_ends_inside_a_block": lambda: _bad(_rows(Script(30).lits(NEED)).end().blocks, cut=300),
    "stream_ends_inside_a_stored_block": lambda: _bad([Block("stored", data=bytes(NEED))], cut=900),
    "stream_ends_inside_a_dynamic_header": lambda: _bad(_rows(Script(31).lits(NEED)).end().blocks, cut=9),
    "block_type_3": lambda: _bad([Block("stored", btype=3)]),
}

# What zlib says to each (a substring of its message, observed once): holds every case to the damage it is named for.
ZLIB_SAYS = {
    "oversubscribed_literal_set": "invalid literal/lengths set",
    "oversubscribed_distance_set": "invalid distances set",
    "oversubscribed_code_length_set": "invalid code lengths set",
    "incomplete_literal_set": "invalid literal/lengths set",
    "incomplete_literal_set_single_2_bit_code": "invalid literal/lengths set",
    "incomplete_distance_set_two_2_bit_codes": "invalid distances set",
    "incomplete_distance_set_single_2_bit_code": "invalid distances set",
    "incomplete_code_length_set_single_code": "invalid code lengths set",
    "incomplete_code_length_set": "invalid code lengths set",
    "no_end_of_block_code": "missing end-of-block",
    "hclen_4_cannot_name_a_length": "missing end-of-block",
    "repeat_16_as_first_length": "invalid bit length repeat",
    "repeat_18_overruns_hlit_plus_hdist": "invalid bit length repeat",
    "repeat_16_overruns_hlit_plus_hdist": "invalid bit length repeat",
    "hlit_field_30": "too many length or distance symbols",
    "hlit_field_31": "too many length or distance symbols",
    "hdist_field_30": "too many length or distance symbols",
    "hdist_field_31": "too many length or distance symbols",
    "unused_bit_of_single_distance_code": "invalid distance code",
    "fixed_literal_symbol_286": "invalid literal/length code",
    "fixed_literal_symbol_287": "invalid literal/length code",
    "fixed_distance_symbol_30": "invalid distance code",
    "fixed_distance_symbol_31": "invalid distance code",
    "distance_before_the_start_fixed": "invalid distance too far back",
    "distance_before_the_start_dynamic": "invalid distance too far back",
    "stored_len_nlen_mismatch": "invalid stored block lengths",
    "stream_ends_inside_a_block": "incomplete or truncated stream",
    "stream_ends_inside_a_stored_block": "incomplete or truncated stream",
    "stream_ends_inside_a_dynamic_header": "incomplete or truncated stream",
    "block_type_3": "invalid block type",
}
assert set(ZLIB_SAYS) == set(INVALID)
# the cases that cannot carry a body: the stream ends, or names no block a decoder could read
NO_BODY = ("hclen_4_cannot_name_a_length", "stream_ends_inside_a_block", "stream_ends_inside_a_stored_block",
           "stream_ends_inside_a_dynamic_header", "block_type_3")


@lru_cache(maxsize=None)
def build(name: str):
    """(file bytes, model output or None, reach) of a case, built once per process."""
    return (VALID.get(name) or INVALID[name])()
