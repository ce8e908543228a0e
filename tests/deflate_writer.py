"""A deflate encoder driven by hand, for the PNG inflate tests.  Test infrastructure (no pytest, no GPU).

`png_writer.py` forces the container, the filters and the block types but leaves compression to zlib, whose encoder
uses a small corner of RFC 1951.  Here every bit is chosen by the caller: the symbol list of each block (literals,
matches with the length symbol named when wanted, end-of-block), the code lengths of both alphabets, how the code
lengths are run-length coded in a dynamic header, HCLEN / HLIT / HDIST, the pad bits and LEN / NLEN of a stored block.
Nothing is validated: the same writer produces the malformed streams of the invalid family.

While it writes, the encoder counts what the stream reaches (`reach`): it knows the length of every code it emits and
the output position of every symbol.  `interpret` is the model: symbol lists -> the bytes they stand for, in plain
Python; it is what a case is meant to contain, and it never looks at the bits.
"""
from __future__ import annotations

import heapq
import struct
import zlib
from collections import Counter
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

EOB = 256
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
         258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # 286 and 287 have codes and are never valid
FIXED_DIST = [5] * 32                                    # so have 30 and 31
GRID_LENGTHS = (3, 4, 63, 64, 65, 127, 128, 129, 257, 258)
GRID_DISTS = range(1, 131)


class BitWriter:
    """LSB-first bit writer (RFC 1951 3.1.1).  Huffman codes go out most significant bit first: the caller passes
    them already reversed (`canonical_codes`), so a code is one call."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value: int, n: int) -> None:
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 512:
            self._flush()

    def _flush(self) -> None:
        k = self.n >> 3
        self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    @property
    def bitpos(self) -> int:
        return len(self.buf) * 8 + self.n

    def align(self, fill: int = 0) -> int:
        pad = -self.bitpos % 8
        self.bits(fill, pad)
        return pad

    def raw(self, data: bytes) -> None:
        assert self.bitpos % 8 == 0
        self._flush()
        self.buf += data

    def getvalue(self) -> bytes:
        self.align()
        self._flush()
        return bytes(self.buf)


def canonical_codes(lengths: Sequence[int]) -> List[tuple]:
    """RFC 1951 3.2.2: (code reversed for the LSB-first writer, length) of every symbol.  Over-subscribed lengths are
    not refused; the codes that overflow are cut to their length."""
    count = Counter(l for l in lengths if l)
    nxt, code = {}, 0
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if not l:
            out.append((0, 0))
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def length_symbol(length: int) -> int:
    return 257 + max(i for i in range(29) if LBASE[i] <= length)


def dist_symbol(dist: int) -> int:
    return max(i for i in range(30) if DBASE[i] <= dist)


# ---- code-length makers

def huffman_lengths(freqs: Sequence[int], maxbits: int = 15, min_codes: int = 2) -> List[int]:
    """Ordinary length-limited Huffman code lengths.  At least `min_codes` symbols get a code (as zlib forces two);
    with min_codes=1 a lone symbol gets the single 1-bit code of an incomplete set."""
    n = len(freqs)
    w = {s: freqs[s] for s in range(n) if freqs[s] > 0}
    spare = [s for s in range(n) if freqs[s] <= 0]
    lens = [0] * n
    if not w:
        return lens
    while len(w) < min_codes:
        w[spare.pop(0)] = 0
    if len(w) == 1:
        lens[next(iter(w))] = 1
        return lens
    depth = dict.fromkeys(w, 0)
    heap = [(f, s, [s]) for s, f in w.items()]
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    num = [0] * (max(max(depth.values()), maxbits) + 1)
    for d in depth.values():
        num[d] += 1
    for d in range(maxbits + 1, len(num)):   # clamp, then give code space back until the set is complete again
        num[maxbits] += num[d]
    num = num[:maxbits + 1]
    total = sum(num[d] << (maxbits - d) for d in range(1, maxbits + 1))
    while total > (1 << maxbits):
        num[maxbits] -= 1
        for d in range(maxbits - 1, 0, -1):
            if num[d]:
                num[d] -= 1
                num[d + 1] += 2
                break
        total -= 1
    order = sorted(w, key=lambda s: (depth[s], -w[s], s))
    it = iter(order)
    for d in range(1, maxbits + 1):
        for _ in range(num[d]):
            lens[next(it)] = d
    return lens


def fill_lengths(n: int, fixed: Dict[int, int], used: Sequence[int], pad: Sequence[int] = ()) -> List[int]:
    """A complete set of code lengths over n symbols in which the symbols of `fixed` have exactly the lengths given.
    What they leave of the code space is, written in binary, a chain of free codes of distinct lengths: fixed lengths
    11, 12, 13, 14, 15, 15 leave 1, 2, ... 10 (the "deep" profile).  The symbols of `used` (most frequent first) take
    those, the shortest being split in two until there are enough; codes left over go to symbols of `pad`, which the
    data never uses."""
    left = (1 << 15) - sum(1 << (15 - l) for l in fixed.values())
    assert left >= 0, "the fixed lengths alone are over-subscribed"
    slots = [l for l in range(1, 16) if (left >> (15 - l)) & 1]
    heapq.heapify(slots)
    while len(slots) < len(used):
        d = heapq.heappop(slots)
        assert d < 15, "no room for that many symbols"
        heapq.heappush(slots, d + 1)
        heapq.heappush(slots, d + 1)
    slots = sorted(slots)
    others = [s for s in list(used) + list(pad) if s not in fixed]
    assert len(others) >= len(slots), "not enough pad symbols to complete the set"
    lens = [0] * n
    for s, l in zip(others, slots):
        lens[s] = l
    for s, l in fixed.items():
        lens[s] = l
    return lens


def deep_lengths(n: int, deep: Sequence[int], used: Sequence[int], lo: int = 11) -> List[int]:
    """The deep profile: the symbols of `deep` get lengths lo, lo + 1, ... 15, and again from lo when there are more
    of them; everything else as `fill_lengths` places it (an odd number of 15-bit codes leaves one more 15-bit code
    free, which goes to a pad symbol: the chain closes on 15, 15)."""
    fixed, l = {}, lo
    for s in deep:
        fixed[s] = l
        l = l + 1 if l < 15 else lo
    pad = [s for s in range(n) if s not in fixed and s not in used]
    return fill_lengths(n, fixed, [s for s in used if s not in fixed], pad)


def short_literal_lengths() -> tuple:
    """The profile with a 1-bit and a 2-bit code: literal 1 has one bit, length symbol 257 (length 3) two, then
    literals 0, 2, 3, 4 three to six and end-of-block six; one 1-bit distance code (distance 1)."""
    lit = [0] * 258
    for s, l in ((1, 1), (257, 2), (0, 3), (2, 4), (3, 5), (4, 6), (EOB, 6)):
        lit[s] = l
    return lit, [1]


# ---- symbols that only the invalid family uses

@dataclass
class RawLit:
    """The code of literal/length symbol `sym` and nothing else (no extra bits, no distance)."""
    sym: int


@dataclass
class RawDist:
    sym: int
    extra: int = 0
    nbits: int = 0


@dataclass
class RawBits:
    value: int
    n: int


@dataclass
class Header:
    """How a dynamic block's header is written."""
    rle: str = "cross"             # "none" | "cross" (greedy 16/17/18, runs may pass from the literal/length
    #                                lengths into the distance lengths) | "split" (greedy, runs broken there)
    hclen: object = "min"          # "min" | "full" | a count
    hlit: Optional[int] = None     # number of literal/length lengths sent (padded with zeros); None: the minimum
    hdist: Optional[int] = None
    hlit_field: Optional[int] = None    # malformed: the raw 5-bit fields, whatever is sent behind them
    hdist_field: Optional[int] = None
    cl_lens: Optional[Sequence[int]] = None   # the 19 code-length code lengths, instead of a Huffman code for them
    cl_syms: Optional[Sequence[tuple]] = None  # the (symbol, extra value) sequence itself, instead of run-length coding


@dataclass
class Block:
    kind: str                      # "stored" | "fixed" | "dynamic"
    symbols: Sequence = ()
    data: bytes = b""              # stored
    lit_lens: Optional[Sequence[int]] = None   # dynamic; None: ordinary Huffman from the symbols' frequencies
    dist_lens: Optional[Sequence[int]] = None
    header: Header = field(default_factory=Header)
    last: Optional[bool] = None    # None: set on the final block of the stream
    pad: int = 0                   # stored: the bits between the block type and the byte boundary
    len_field: Optional[int] = None   # malformed stored blocks
    nlen_field: Optional[int] = None
    btype: Optional[int] = None    # malformed: the 2-bit type as sent (3)


def symbol_frequencies(symbols) -> tuple:
    lf, df = [0] * 286, [0] * 30
    for s in symbols:
        if isinstance(s, int):
            lf[s] += 1
        elif isinstance(s, tuple):
            lf[s[2] if len(s) > 2 else length_symbol(s[0])] += 1
            df[dist_symbol(s[1])] += 1
    return lf, df


def run_length_code(seq: Sequence[int]) -> List[tuple]:
    """Greedy 16/17/18 coding of a code-length sequence: (symbol, extra value, first index, count)."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, i, r))
                i, run = i + r, run - r
            if run >= 3:
                out.append((17, run - 3, i, run))
                i, run = i + run, 0
        else:
            out.append((v, 0, i, 1))
            i, run = i + 1, run - 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3, i, r))
                i, run = i + r, run - r
        for _ in range(run):
            out.append((v, 0, i, 1))
            i += 1
    return out


class Encoder:
    """Writes blocks, keeps the output position, counts what the stream reaches."""

    def __init__(self):
        self.bw = BitWriter()
        self.reach: Counter = Counter()
        self.pos = 0
        self.spans: List[tuple] = []   # (first output byte, end, kind) of every block written
        self._grid, self._fixed = set(), {"len": set(), "dist": set(), "ones": set(), "zeros": set()}
        self._eob_run = 0
        self.marks: Dict[str, int] = {}

    # -- dynamic header
    def _dynamic_header(self, lit_lens, dist_lens, h: Header) -> None:
        bw, reach = self.bw, self.reach
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        hlit = h.hlit or max(257, max((i + 1 for i, l in enumerate(lit_lens) if l), default=0))
        hdist = h.hdist or max(1, max((i + 1 for i, l in enumerate(dist_lens) if l), default=0))
        lit = (lit_lens + [0] * hlit)[:hlit]
        dist = (dist_lens + [0] * hdist)[:hdist]
        if h.cl_syms is not None:
            seq = [(s, e, 0, 0) for s, e in h.cl_syms]
        elif h.rle == "none":
            seq = [(v, 0, i, 1) for i, v in enumerate(lit + dist)]
            reach["rle_none"] += 1
        elif h.rle == "cross":
            seq = run_length_code(lit + dist)
            for s, _, at, cnt in seq:
                if s >= 16 and at < hlit < at + cnt:
                    reach["rep%d_cross" % s] += 1
        else:
            seq = run_length_code(lit) + [(s, e, at + hlit, c) for s, e, at, c in run_length_code(dist)]
            # counted only where the coding that may cross would have run a repeat over the boundary
            reach["rep_split_at_boundary"] += any(s >= 16 and at < hlit < at + cnt
                                                  for s, _, at, cnt in run_length_code(lit + dist))
        if h.cl_lens is not None:
            cl = list(h.cl_lens)
        else:
            f = [0] * 19
            for s, *_ in seq:
                f[s] += 1
            cl = huffman_lengths(f, 7)
        sent = [cl[s] for s in CL_ORDER]
        least = max(4, max((i + 1 for i, l in enumerate(sent) if l), default=0))
        hclen = {"min": least, "full": 19}.get(h.hclen, h.hclen)
        reach["hclen_%d" % hclen] += 1
        if hclen == 19 and sent[18] == 0:
            reach["hclen_19_trailing_zeros"] += 1
        reach["hlit_%d" % hlit] += 1
        reach["hdist_%d" % hdist] += 1
        bw.bits(h.hlit_field if h.hlit_field is not None else hlit - 257, 5)
        bw.bits(h.hdist_field if h.hdist_field is not None else hdist - 1, 5)
        bw.bits(hclen - 4, 4)
        for l in sent[:hclen]:
            bw.bits(l, 3)
        codes = canonical_codes(cl)
        for s, e, *_ in seq:
            bw.bits(*codes[s])
            if s >= 16:
                bw.bits(e, (2, 3, 7)[s - 16])
        nd = [l for l in dist if l]
        if nd == [1]:
            reach["one_dist_code_len1"] += 1
        if not nd:
            reach["zero_dist_codes"] += 1

    # -- one symbol
    def _litlen(self, codes, sym: int, what: str) -> int:
        rev, l = codes[sym]
        self.bw.bits(rev, l)
        r = self.reach
        r["%s_code_bits_%d" % (what, l)] += 1
        r["long_codes"] += l > 10
        r["codes_gt_11"] += l > 11
        r["codes_gt_12"] += l > 12
        return l

    def _match(self, lcodes, dcodes, s, fixed: bool, block_start: int) -> None:
        bw, r, pos = self.bw, self.reach, self.pos
        length, dist = s[0], s[1]
        ls = s[2] if len(s) > 2 else length_symbol(length)
        self._litlen(lcodes, ls, "len")
        le = length - LBASE[ls - 257]
        bw.bits(le, LEXT[ls - 257])
        ds = dist_symbol(dist)
        rev, l = dcodes[ds]
        bw.bits(rev, l)
        de = dist - DBASE[ds]
        bw.bits(de, DEXT[ds])
        r["dist_code_bits_%d" % l] += 1
        r["matches"] += 1
        r["overlapping"] += dist < length
        r["dist_gt_16k"] += dist > 16384
        if length == 258:
            r["len258_sym%d" % ls] += 1
        if fixed:
            f = self._fixed
            f["len"].add(ls)
            f["dist"].add(ds)
            for kind, e, nb in (("l", le, LEXT[ls - 257]), ("d", de, DEXT[ds])):
                if nb:
                    sym = ls if kind == "l" else ds
                    if e == (1 << nb) - 1:
                        f["ones"].add((kind, sym))
                    if e == 0:
                        f["zeros"].add((kind, sym))
        if dist in GRID_DISTS and length in GRID_LENGTHS:
            self._grid.add((dist, length))
        wrap = (pos + length - 1) // 32768 != pos // 32768
        r["match_straddles_32768"] += wrap
        r["match_straddles_1024"] += (pos + length - 1) // 1024 != pos // 1024
        r["dist_32768"] += dist == 32768
        r["dist_32760_to_32767"] += 32760 <= dist < 32768
        r["resolve_ordered"] += dist + length > 32768     # holds whatever else shares the match's batch
        r["resolve_ordered_straddles_32768"] += wrap and dist + length > 32768
        r["resolve_ordered_straddles_1024"] += (pos + length - 1) // 1024 != pos // 1024 and dist + length > 32768
        src = pos - dist
        if 0 <= src < block_start:
            kind = next(k for a, b, k in self.spans if a <= src < b)
            r["match_source_in_block_of_other_type"] += kind != ("fixed" if fixed else "dynamic")

    # -- blocks
    def block(self, b: Block, last: bool) -> None:
        bw, r = self.bw, self.reach
        start = self.pos
        bw.bits(1 if last else 0, 1)
        bw.bits({"stored": 0, "fixed": 1, "dynamic": 2}[b.kind] if b.btype is None else b.btype, 2)
        if b.btype == 3:
            return
        if b.kind == "stored":
            r["stored_blocks"] += 1
            r["stored_header_at_bit_%d" % ((bw.bitpos - 3) % 8)] += 1
            npad = bw.align(b.pad)
            r["stored_nonzero_pad_bits"] += bool(npad and b.pad & ((1 << npad) - 1))
            n = len(b.data)
            ln = n if b.len_field is None else b.len_field
            bw.raw(struct.pack("<HH", ln, (~ln & 0xffff) if b.nlen_field is None else b.nlen_field))
            bw.raw(b.data)
            r["stored_len_0"] += n == 0
            r["stored_len_65535"] += n == 65535
            r["stored_as_last_block"] += last
            self.pos += n
            self._eob_run = 0
        else:
            fixed = b.kind == "fixed"
            if fixed:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                lit_lens, dist_lens = b.lit_lens, b.dist_lens
                if lit_lens is None or dist_lens is None:
                    lf, df = symbol_frequencies(b.symbols)
                    lit_lens = huffman_lengths(lf) if lit_lens is None else lit_lens
                    dist_lens = huffman_lengths(df) if dist_lens is None else dist_lens
                self._dynamic_header(lit_lens, dist_lens, b.header)
            r["fixed_blocks" if fixed else "dynamic_blocks"] += 1
            if "first_header_end_bit" not in self.marks:
                self.marks["first_header_end_bit"] = bw.bitpos
            lcodes = canonical_codes(list(lit_lens) + [0] * (288 - len(lit_lens)))
            dcodes = canonical_codes(list(dist_lens) + [0] * (32 - len(dist_lens)))
            prev_short_lit = False
            run1 = run2 = alt = 0
            for k, s in enumerate(b.symbols):
                if isinstance(s, int) and s < 256:
                    l = self._litlen(lcodes, s, "lit")
                    r["literals"] += 1
                    r["long_code_behind_short_literal"] += prev_short_lit and l > 10
                    prev_short_lit = l <= 10
                    self.pos += 1
                    run1 = run1 + 1 if l == 1 else 0
                    run2 = run2 + 1 if l == 2 else 0
                    alt = alt + 1 if l == 1 and alt % 2 == 0 else 0
                elif isinstance(s, int):
                    l = self._litlen(lcodes, s, "eob")
                    r["long_code_behind_short_literal"] += prev_short_lit and l > 10
                    prev_short_lit = False
                    run1 = run2 = alt = 0
                elif isinstance(s, tuple):
                    self._match(lcodes, dcodes, s, fixed, start)
                    r["long_code_behind_short_literal"] += prev_short_lit and lcodes[
                        s[2] if len(s) > 2 else length_symbol(s[0])][1] > 10
                    self.pos += s[0]
                    prev_short_lit = False
                    run1 = run2 = 0
                    alt = alt + 1 if s[0] <= 4 and alt % 2 == 1 else 0
                else:
                    prev_short_lit = False
                    if isinstance(s, RawLit):
                        bw.bits(*lcodes[s.sym])
                    elif isinstance(s, RawDist):
                        bw.bits(*dcodes[s.sym])
                        bw.bits(s.extra, s.nbits)
                    else:
                        bw.bits(s.value, s.n)
                r["run_of_1024_one_bit_literals"] += run1 == 1024
                r["run_of_1024_two_bit_literals"] += run2 == 1024
                r["run_of_1024_one_bit_literal_then_short_match"] += alt == 1024
                if k == 7 and "first_symbols_end_bit" not in self.marks:
                    self.marks["first_symbols_end_bit"] = bw.bitpos
            if self.pos == start and list(b.symbols) == [EOB]:
                r["eob_only_%s_blocks" % b.kind] += 1
                self._eob_run += 1
                r["twenty_eob_only_blocks_in_a_row"] += self._eob_run == 20
            else:
                self._eob_run = 0
        self.spans.append((start, self.pos, b.kind))

    def finish(self) -> Counter:
        r = self.reach
        end = self.pos
        data = [(a, b) for a, b, _ in self.spans if b > a]
        for a, b, _ in self.spans:
            if a == b and data:
                r["empty_block_before_data"] += a <= data[0][0]
                r["empty_block_between_data"] += data[0][1] <= a <= data[-1][0] and len(data) > 1
                r["empty_block_behind_data"] += a >= end
        f = self._fixed
        ext_l = {("l", s) for s in range(257, 286) if LEXT[s - 257]}
        ext_d = {("d", s) for s in range(30) if DEXT[s]}
        r["fixed_every_length_symbol"] += f["len"] >= set(range(257, 286))
        r["fixed_every_distance_symbol"] += f["dist"] >= set(range(30))
        r["fixed_extra_bits_all_ones_everywhere"] += f["ones"] >= ext_l | ext_d
        r["fixed_extra_bits_all_zeros_everywhere"] += f["zeros"] >= ext_l | ext_d
        r["every_distance_1_to_130_at_every_grid_length"] += len(self._grid) == len(GRID_DISTS) * len(GRID_LENGTHS)
        return Counter({k: int(v) for k, v in r.items() if v})


def interpret(blocks: Sequence[Block]) -> bytes:
    """The model: what the symbol lists stand for.  Malformed pieces are passed over."""
    out = bytearray()
    for b in blocks:
        if b.kind == "stored":
            out += b.data
            continue
        for s in b.symbols:
            if isinstance(s, int):
                if s == EOB:
                    break
                out.append(s)
            elif isinstance(s, tuple):
                length, dist = s[0], s[1]
                if dist > len(out):
                    out += bytes(length)
                elif dist >= length:
                    at = len(out) - dist
                    out += out[at:at + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
    return bytes(out)


def lenient_inflate(stream: bytes, cap: int) -> bytes:
    """What a decoder WITHOUT any validity check reads from a zlib stream, up to `cap` bytes: canonical codes first
    code first whatever the set of lengths (over-subscribed, incomplete, no end-of-block), any count of lengths, a
    repeat clamped to the count (16 in front: of length 0), symbols past the tables read as the nearest one, a distance
    before the start as zeros, LEN taken without NLEN.  It stops where the stream ends or names block type 3.  The
    malformed cases are measured with it: behind its damage a case must hold all the bytes its image needs."""
    data, at, out = stream[2:], 0, bytearray()

    def bits(n):
        nonlocal at
        v = 0
        for i in range(n):
            if at >> 3 >= len(data):
                raise EOFError
            v |= ((data[at >> 3] >> (at & 7)) & 1) << i
            at += 1
        return v

    def table(lens):
        return [sum(1 for l in lens if l == k) for k in range(16)], sorted((s for s, l in enumerate(lens) if l),
                                                                           key=lambda s: (lens[s], s))

    def decode(t):
        count, syms = t
        code = first = index = 0
        for l in range(1, 16):
            code |= bits(1)
            if code - count[l] < first:
                return syms[min(index + code - first, len(syms) - 1)]
            index, first, code = index + count[l], (first + count[l]) << 1, code << 1
        return 0

    try:
        last = 0
        while not last and len(out) < cap:
            last, kind = bits(1), bits(2)
            if kind == 0:
                at = (at + 7) & ~7
                n = bits(16)
                bits(16)
                out += bytes(bits(8) for _ in range(n))
                continue
            if kind == 3:
                break
            if kind == 1:
                lit, dist = table(FIXED_LIT), table(FIXED_DIST)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits(3)
                cl, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s = decode(cl)
                    rep, v = (1, s) if s < 16 else ((3 + bits(2), lens[-1] if lens else 0) if s == 16 else
                                                    (3 + bits(3), 0) if s == 17 else (11 + bits(7), 0))
                    lens += [v] * min(rep, hlit + hdist - len(lens))
                lit, dist = table(lens[:hlit]), table(lens[hlit:])
            while len(out) < cap:
                s = decode(lit)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    i = min(s - 257, 28)
                    n = LBASE[i] + bits(LEXT[i])
                    d = min(decode(dist) if dist[1] else 0, 29)
                    d = DBASE[d] + bits(DEXT[d])
                    for _ in range(n):
                        out.append(out[-d] if d <= len(out) else 0)
    except EOFError:
        pass
    return bytes(out[:cap])


def zlib_stream(blocks: Sequence[Block]) -> tuple:
    """Blocks in sequence -> (zlib stream: 78 9c, the blocks, Adler-32 of the model output; model output; reach;
    marks: bit positions inside the raw deflate data)."""
    enc = Encoder()
    for i, b in enumerate(blocks):
        enc.block(b, (i == len(blocks) - 1) if b.last is None else b.last)
    model = interpret(blocks)
    z = b"\x78\x9c" + enc.bw.getvalue() + struct.pack(">I", zlib.adler32(model) & 0xffffffff)
    return z, model, enc.finish(), enc.marks


class Script:
    """Symbol lists written with the output position in view, for exact placement.  Literals default to seeded bytes
    in 0..4: as 8-bit grey scanlines every one of them is a legal filter type wherever the rows fall."""

    def __init__(self, seed: int = 0, top: int = 5):
        self.rng = np.random.default_rng(seed)
        self.top = top
        self.blocks: List[Block] = []
        self.syms: list = []
        self.pos = 0

    def lit(self, v: Optional[int] = None) -> "Script":
        self.syms.append(int(self.rng.integers(0, self.top)) if v is None else v)
        self.pos += 1
        return self

    def lits(self, n: int, v: Optional[int] = None) -> "Script":
        for _ in range(n):
            self.lit(v)
        return self

    def lits_to(self, pos: int) -> "Script":
        assert pos >= self.pos, (pos, self.pos)
        return self.lits(pos - self.pos)

    def match(self, length: int, dist: int, lsym: Optional[int] = None) -> "Script":
        assert 3 <= length <= 258 and 1 <= dist <= min(self.pos, 32768), (length, dist, self.pos)
        self.syms.append((length, dist) if lsym is None else (length, dist, lsym))
        self.pos += length
        return self

    def end(self, kind: str = "dynamic", **kw) -> "Script":
        self.blocks.append(Block(kind, self.syms + [EOB], **kw))
        self.syms = []
        return self

    def stored(self, n: int, **kw) -> "Script":
        assert not self.syms
        self.blocks.append(Block("stored", data=bytes(self.rng.integers(0, self.top, n).astype(np.uint8)), **kw))
        self.pos += n
        return self

    def empty(self, kind: str, count: int = 1, **kw) -> "Script":
        assert not self.syms
        for _ in range(count):
            self.blocks.append(Block(kind, [EOB], **kw))
        return self


def tokenize(data: bytes, distances: Sequence[int]) -> list:
    """The scripted tokenizer: at each position the longest match (>= 3, <= 258) among the candidate distances, the
    first candidate winning a tie; else a literal."""
    a = np.frombuffer(data, np.uint8)
    n = a.size
    runs = {}
    for d in distances:
        if d >= n:
            continue
        stop = np.flatnonzero(np.concatenate([a[d:] != a[:-d], [True]]))   # first mismatch at or behind i
        runs[d] = stop[np.searchsorted(stop, np.arange(n - d))] - np.arange(n - d)
    out, p = [], 0
    while p < n:
        best, bd = 2, 0
        for d, r in runs.items():
            if d <= p and r[p - d] > best:
                best, bd = int(r[p - d]), d
        if bd:
            best = min(best, 258)
            out.append((best, bd))
            p += best
        else:
            out.append(int(a[p]))
            p += 1
    return out
