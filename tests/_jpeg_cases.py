"""_jpeg_cases.py - TEST INFRASTRUCTURE.  One named table of hand-built JPEG streams (tests/jpeg_writer.py) for the
host tests (test_jpeg_host.py: emulator, stager, sanitised stand-alone program) and the GPU tests
(test_jpeg_streams_gpu.py).  Every case says what it is there for and asserts its own non-vacuity from the writer's
statistics; what only the staged header or the emulator can tell (`use2`, `nsegments`, subsequence geometry, hand-over
rounds) is stated in `expect` and asserted by the host tests.

REFERENCE RULE.  Where every coefficient comes from the forward DCT of 8-bit pixels or has |value| <= 150 the expected
image is live Pillow (libjpeg-turbo), and oracle/jpeg.py must agree with it (`ref == "pillow"`).  The
extreme-magnitude cases (`ref == "oracle"`) are compared with oracle/jpeg.py alone: libjpeg-turbo's SIMD IDCT saturates
its 16-bit intermediates there, the C islow IDCT that the decoder restates does not.  Nothing is ever compared with the
emulator's or a kernel's own output.
"""
from __future__ import annotations

import functools
import io
import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_writer as jw  # noqa: E402

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2
BIG_WINDOW = (264, 264)     # >= every small image: all MCUs reconstructed, 1089 MCUs of the 264 x 264 cases in the DC scan
SMALL_WINDOW = (31, 45)     # inside most images (last_mcu short of the last MCU); 45 % 4 != 0: jpeg_color_kernel<1>


@dataclass
class Case:
    name: str
    why: str
    data: bytes
    stats: Dict
    ref: str = "pillow"                      # "pillow" or "oracle" (reference rule above)
    expect: Dict = field(default_factory=dict)
    big: bool = False                         # exceeds the 264 x 264 / 40 KB size rule (named exception)
    _expected: np.ndarray = None

    def expected(self) -> np.ndarray:
        """The whole decoded image [H, W, 3] by the case's reference."""
        if self._expected is None:
            if self.ref == "pillow":
                self._expected = np.asarray(Image.open(io.BytesIO(self.data)).convert("RGB"))
            else:
                from oracle import jpeg as oj
                self._expected = oj.decode(self.data)
        return self._expected

    def window(self, wh: int, ww: int) -> np.ndarray:
        return center_window(self.expected(), wh, ww)


def center_window(rgb: np.ndarray, wh: int, ww: int) -> np.ndarray:
    """torchvision CenterCrop((wh, ww)): zero padding to the window, crop at round((dim - win) / 2)."""
    h, w = rgb.shape[:2]
    ph, pw = max(wh - h, 0), max(ww - w, 0)
    if ph or pw:
        rgb = np.pad(rgb, ((ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2), (0, 0)))
        h, w = rgb.shape[:2]
    top, left = int(round((h - wh) / 2.0)), int(round((w - ww) / 2.0))
    return rgb[top:top + wh, left:left + ww]


# ---- ingredients ------------------------------------------------------------------------------------------------
def synth(rng, h: int, w: int, grey: bool = False, noise: int = 20) -> np.ndarray:
    """A smooth random field plus noise: coefficients of every frequency, DC differences of both signs."""
    gh, gw = h // 16 + 2, w // 16 + 2
    base = rng.integers(0, 256, (gh, gw, 3)).astype(np.float64)
    y, x = np.linspace(0, gh - 1.001, h), np.linspace(0, gw - 1.001, w)
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
    a = (base[y0][:, x0] * (1 - fy) * (1 - fx) + base[y0 + 1][:, x0] * fy * (1 - fx) +
         base[y0][:, x0 + 1] * (1 - fy) * fx + base[y0 + 1][:, x0 + 1] * fy * fx)
    a += rng.integers(-noise, noise + 1, a.shape)
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return a[..., 1] if grey else a


def q_ramp(q0: float, slope: float = 0.5) -> np.ndarray:
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    return np.maximum(1, np.rint(q0 * (1 + slope * (i + j)))).astype(np.int64).reshape(64)


FIXED_DC = jw.table_from_lengths([(s, 4) for s in range(12)])            # 12 DC codes of 4 bits
FIXED_AC = jw.table_from_lengths([(s, 8) for s in jw.ALL_AC_SYMBOLS])    # 162 AC codes of 8 bits
_FREQ = sorted(jw.ALL_AC_SYMBOLS, key=jw.ac_symbol_rank)
# 22 RARE symbols on 6 bits, the 140 frequent ones on 12 bits: 2240 prefixes behind the lookup -> range search
RANGE12_AC = jw.table_from_lengths([(s, 6) for s in _FREQ[140:]] + [(s, 12) for s in _FREQ[:140]])
# 14 frequent symbols on 5 bits, 148 on 16 bits: an incomplete table whose 16-bit codes are in use
RANGE16_AC = jw.table_from_lengths([(s, 5) for s in _FREQ[:14]] + [(s, 16) for s in _FREQ[14:]])
CHROMA_DC = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))


def tables_for(sampling, dc=None, ac=None) -> Tuple[Dict, List[Tuple[int, int]]]:
    """One DC and one AC table shared by every component."""
    t = {(0, 0): dc or jw.generic_dc_table(), (1, 0): ac or jw.generic_ac_table()}
    return t, [(0, 0)] * len(jw.component_layout(sampling))


def from_pixels(rng, h, w, sampling, quant, tables, selectors, noise=20, **kw):
    img = synth(rng, h, w, grey=sampling == "grey", noise=noise)
    quant = quant if isinstance(quant, list) else [quant]
    blocks = jw.blocks_from_pixels(img, sampling, quant, kw.get("quant_sel"))
    return jw.write_jpeg(h, w, sampling, blocks, tables, selectors, quant=quant, **kw)


def random_blocks(rng, by, bx, ac_syms, mean_syms=5.0, dc_amp=40) -> np.ndarray:
    """Blocks drawn symbol by symbol from `ac_syms` (run/size bytes; |value| < 2^size), DC uniform in +-dc_amp."""
    out = np.zeros((by, bx, 64), np.int64)
    syms = [s for s in ac_syms if s not in (0x00, 0xF0)]
    for y in range(by):
        for x in range(bx):
            z = out[y, x]
            z[0] = rng.integers(-dc_amp, dc_amp + 1)
            k = 1
            for _ in range(rng.poisson(mean_syms)):
                cand = [s for s in syms if k + (s >> 4) <= 63]
                if not cand:
                    break
                s = cand[rng.integers(len(cand))]
                k += s >> 4
                size = s & 15
                z[k] = int(rng.integers(1 << (size - 1), 1 << size)) * (1 if rng.integers(2) else -1)
                k += 1
    return out


def fit_stream_bytes(write, blocks, lo: int, hi: int):
    """Zero AC coefficients from the end of the scan until lo < unstuffed stream bytes <= hi (one-component blocks)."""
    flat = blocks[0].reshape(-1, 64)
    pos = [(b, k) for b in range(flat.shape[0] - 1, -1, -1) for k in range(63, 0, -1) if flat[b, k]]

    def attempt(n):
        f = flat.copy()
        for b, k in pos[:n]:
            f[b, k] = 0
        return write([f.reshape(blocks[0].shape)])

    a, b = 0, len(pos)
    assert attempt(0)[1]["stream_bytes"] > hi >= attempt(b)[1]["stream_bytes"]
    while b - a > 1:
        m = (a + b) // 2
        if attempt(m)[1]["stream_bytes"] > hi:
            a = m
        else:
            b = m
    data, st = attempt(b)
    assert lo < st["stream_bytes"] <= hi, st["stream_bytes"]
    return data, st


# ---- the accepted cases ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Case]:
    out: Dict[str, Case] = {}

    def add(name, why, data_stats, **kw):
        data, st = data_stats
        assert name not in out
        out[name] = Case(name, why, data, st, **kw)
        return st

    rng = np.random.default_rng(20261021)

    # ---- tables ----
    t, sel = tables_for((1, 1), ac=RANGE12_AC)
    st = add("tab_range12", "use2 == 0 (2240 long prefixes): >= 1000 symbols on 12-bit codes reach the range search",
             from_pixels(rng, 64, 64, (1, 1), q_ramp(3), t, sel), expect=dict(fast=0))
    assert st["long_symbols"][(1, 0)] >= 1000, st["long_symbols"]

    t, sel = tables_for((2, 1), ac=RANGE16_AC)
    st = add("tab_range16", "use2 == 0, incomplete table: 16-bit codes in use through the range search",
             from_pixels(rng, 48, 80, (2, 1), q_ramp(4), t, sel), expect=dict(fast=0))
    assert st["long_symbols"][(1, 0)] >= 200, st["long_symbols"]

    t, sel = tables_for((2, 2), ac=jw.generic_ac_table(reverse=True))
    st = add("tab_look2", "complete K.5 profile, use2 == 1, FREQUENT symbols on the 12- to 16-bit codes: look2",
             from_pixels(rng, 72, 56, (2, 2), q_ramp(4), t, sel), expect=dict(fast=1))
    assert st["long_symbols"][(1, 0)] >= 1000, st["long_symbols"]

    four = {(0, 0): jw.generic_dc_table(), (0, 1): CHROMA_DC, (1, 0): jw.generic_ac_table(),
            (1, 1): jw.generic_ac_table(reverse=True)}
    st = add("tab_four", "four distinct tables: Y on DC0/AC0, Cb on DC1/AC1, Cr on DC0/AC1; two quantisation tables",
             from_pixels(rng, 56, 72, (2, 2), [q_ramp(3), q_ramp(5, 1.0)], four, [(0, 0), (1, 1), (0, 1)],
                         quant_sel=[0, 1, 1]), expect=dict(fast=1, nx_off32=True))
    assert st["long_symbols"][(1, 1)] > 100 and st["long_symbols"][(1, 0)] > 0

    one_dc = {(0, 0): ([1] + [0] * 15, [0]), (1, 0): jw.generic_ac_table()}
    blk = random_blocks(rng, 5, 7, _FREQ[1:30], dc_amp=0)
    st = add("tab_dc_one", "a one-symbol DC table (category 0 on the 1-bit code '0'): every DC difference is 0",
             jw.write_jpeg(40, 56, "grey", [blk], one_dc, [(0, 0)], quant=[q_ramp(2)]), expect=dict(fast=0))
    assert st["max_dc_cat"] == 0 and st["symbols"] > 100

    # ---- symbols ----
    blk = np.zeros((4, 4, 64), np.int64)
    blk[..., 0] = np.where((np.arange(16).reshape(4, 4) % 2) == 0, -1024, 1023)   # differences of +-2047: category 11
    blk[1, 2, 1], blk[2, 1, 8], blk[3, 3, 2] = 1023, -600, 512                      # AC size 10
    st = add("sym_extreme", "DC category 11 and AC size 10 in sparse blocks (q = 1); reference: oracle/jpeg.py alone",
             jw.write_jpeg(32, 32, "grey", [blk], *tables_for("grey"), quant=[np.ones(64, np.int64)]), ref="oracle",
             expect=dict(fast=1))
    assert st["max_dc_cat"] == 11 and st["max_ac_size"] == 10

    blk = [random_blocks(rng, 6, 6, _FREQ[1:12], mean_syms=1.0, dc_amp=60) for _ in range(3)]
    for c in range(3):
        blk[c][0, 1, 1:] = 0
        blk[c][0, 1, 17] = 5                       # a run of 16 zeros: one ZRL
        blk[c][1, 2, 1:] = 0
        blk[c][1, 2, 33] = -3                      # 32 zeros: two ZRL
        blk[c][2, 3, 1:] = 0
        blk[c][2, 3, 49], blk[c][2, 3, 63] = 2, 1  # 48 zeros: three ZRL; coefficient 63 set: no EOB
        blk[c][3, 4, 63] = -1
        blk[c][5, 5, 1:] = 7                       # a dense block that ends at coefficient 63
    st = add("sym_zrl_noeob", "runs of 16, 32 and 48 zeros (chained ZRL), blocks that end without an EOB",
             jw.write_jpeg(48, 48, (1, 1), blk, *tables_for((1, 1)), quant=[q_ramp(2)]), expect=dict(fast=1))
    assert st["zrl"] >= 18 and st["no_eob"] >= 9 and st["max_zero_run"] >= 48

    blk = [np.zeros((33, 33, 64), np.int64) for _ in range(3)]
    st = add("sym_all_eob", "all-EOB blocks with DC difference 0: the most blocks per subsequence (32 per 128 bits)",
             jw.write_jpeg(264, 264, (1, 1), blk, *tables_for((1, 1))), expect=dict(fast=1))
    assert st["symbols"] == 2 * 3267 and st["stream_bytes"] * 8 <= 4 * 3267 + 7

    blk = [np.zeros((8, 8, 64), np.int64)]
    blk[0][..., 0] = rng.integers(-30, 31, (8, 8))
    blk[0][..., 1:40] = rng.choice([127, 63, 31, 15], (8, 8, 39))      # magnitudes whose bits are all ones
    st = add("sym_stuffed", ">= 5 % stuffed bytes: all-ones magnitudes behind the 0xFF.. codes of the reversed table",
             jw.write_jpeg(64, 64, "grey", blk, *tables_for("grey", ac=jw.generic_ac_table(reverse=True)),
                           quant=[np.ones(64, np.int64)]), expect=dict(fast=1))
    assert st["stuffed"] >= 0.05 * st["stream_bytes"], (st["stuffed"], st["stream_bytes"])

    # ---- synchronisation: fixed-length codes never re-synchronise ----
    fixed, sel = tables_for((1, 1), dc=FIXED_DC, ac=FIXED_AC)
    nblk = [random_blocks(rng, 24, 24, [s for s in _FREQ if (s & 15) == 4 and (s >> 4) < 4], mean_syms=4.0, dc_amp=5)
            for _ in range(3)]
    for b in nblk:                                   # every symbol 12 bits long: DC 4 + 8 (category 8), AC 8 + 4
        b[..., 0] = np.where(np.indices(b.shape[:2]).sum(0) % 2 == 0, -100, 100)
    never = lambda ri: jw.write_jpeg(192, 192, (1, 1), nblk, fixed, sel, restart=ri)  # noqa: E731
    st = add("sync_never", "fixed-length codes, no restart: rounds >= nact / 2, > 256 chains live after round 1 "
             "(the in-place branch), thread 0 decodes everything", never(0),
             expect=dict(fast=0, min_rounds_frac=0.5, live1_over=256))
    assert st["stream_bytes"] < 40 * 1024
    add("sync_ri100", "the same stream with restart interval 100: between 20 and 200 rounds", never(100),
        expect=dict(fast=0, rounds=(20, 200)))
    add("sync_ri3", "the same stream with restart interval 3: a handful of rounds", never(3),
        expect=dict(fast=0, rounds=(2, 10), nseg=192))

    add("sync_ri1", "the same stream with restart interval 1: every chain is put right at the next MCU, so at most 256 "
        "are live after round 1 (the compaction queue from round 2 on)", never(1),
        expect=dict(fast=0, live1_atmost=256, nseg=576))

    # ---- DC scan: 1089 MCUs in the window, chunk >= 2 ----
    img = synth(rng, 264, 264, noise=6)
    q = [q_ramp(12, 1.0)]
    dblk = jw.blocks_from_pixels(img, (1, 1), q)
    t, sel = tables_for((1, 1))
    # (one table pair for all three components: a chain that starts in the wrong block of the MCU never merges, so
    # without restart markers these streams, too, take about nact rounds)
    for ri, why in [(3, "restart boundaries inside every thread's chunk; at most 256 chains live after round 1 (the "
                        "compaction queue from round 2 on)"),
                    (100, "a segment crosses a wave's 64 * chunk MCUs"),
                    (1, "restart interval 1: 1089 segments"),
                    (5000, "an interval larger than the MCU count: one segment"),
                    (7, "an interval that does not divide mcus_x = 33")]:
        add(f"dc_ri{ri}", f"264 x 264 at 4:4:4 = 1089 MCUs, chunk >= 2 in the DC scan; {why}",
            jw.write_jpeg(264, 264, (1, 1), dblk, t, sel, quant=q, restart=ri),
            expect=dict(fast=1, nseg=-(-1089 // ri), chunk2=True, **(dict(live1_atmost=256) if ri == 3 else {})))

    # ---- geometry of the re-laid stream ----
    st = add("geo_nact1", "nact == 1: a one-byte stream",
             jw.write_jpeg(8, 8, "grey", [np.zeros((1, 1, 64), np.int64)], *tables_for("grey")),
             expect=dict(fast=1, nact=1))
    assert st["stream_bytes"] == 1

    gimg = synth(rng, 176, 176, grey=True, noise=25)
    gq = [q_ramp(2, 0.25)]
    gblk = jw.blocks_from_pixels(gimg, "grey", gq)
    t, sel = tables_for("grey")
    add("geo_nact_T", "nact == T at 1024 threads: 16368 < stream bytes <= 16384, every thread owns a subsequence",
        fit_stream_bytes(lambda b: jw.write_jpeg(176, 176, "grey", b, t, sel, quant=gq), gblk, 16368, 16384),
        expect=dict(fast=1, nact=1024))

    bimg = synth(rng, 320, 320, grey=True, noise=60)
    bq = [q_ramp(1, 0.1)]
    t, sel = tables_for("grey")
    st = add("geo_wps33", "a dense, re-synchronising stream above 64 KB: wps > 32 at 512 threads (second tile row of "
             "the interleave kernel); exceeds the size rule on purpose",
             jw.write_jpeg(320, 320, "grey", jw.blocks_from_pixels(bimg, "grey", bq), t, sel, quant=bq, restart=64),
             expect=dict(fast=1, wps512_over=32), big=True)
    assert st["stream_bytes"] > 66 * 1024

    # ---- format ----
    q16 = q_ramp(40, 2.0)
    q16[0] = 260
    t, sel = tables_for((2, 1))
    st = add("fmt_sof1_q16", "SOF1 with 16-bit quantisation tables holding values above 255 (DC step 260)",
             from_pixels(rng, 40, 72, (2, 1), q16, t, sel, sof=0xC1), expect=dict(fast=1))
    assert q16.max() > 255 and b"\xff\xc1" in out["fmt_sof1_q16"].data and st["max_dc_cat"] >= 2

    t, sel = tables_for((2, 2))
    st = add("fmt_fill_rst", "three fill FF bytes in front of every RSTn; 20 intervals, so the marker index wraps",
             from_pixels(rng, 64, 80, (2, 2), q_ramp(3), t, sel, restart=1, fill=3), expect=dict(fast=1, nseg=20))
    assert st["markers"] == 19 and b"\xff\xff\xff\xff\xd0" in out["fmt_fill_rst"].data
    return out


# ---- about 48 distinct small streams: the edge sizes on every Huffman instantiation -----------------------------------
@functools.lru_cache(maxsize=None)
def small_cases() -> List[Case]:
    rng = np.random.default_rng(48)
    sizes = [(1, 1), (3, 5), (17, 3), (8, 8), (33, 17), (40, 56), (64, 64), (50, 70)]
    out = []
    for rep in range(2):
        for si, (h, w) in enumerate(sizes[:8 if rep == 0 else 4]):
            for ki, sampling in enumerate(["grey", (1, 1), (2, 1), (2, 2)]):
                i = len(out)
                ri = (0, 1, 3)[(si + ki + rep) % 3]
                slow = i % 6 == 5      # fixed-length tables: use2 == 0, sends a whole batch to the generic loop
                t, sel = tables_for(sampling, dc=FIXED_DC if slow else None, ac=FIXED_AC if slow else None)
                data, st = from_pixels(rng, h, w, sampling, q_ramp(2 + rep * 6), t, sel, restart=ri)
                out.append(Case(f"small{i:02d}_{h}x{w}_{sampling}_ri{ri}{'_fixed' if slow else ''}".replace(" ", ""),
                                "edge sizes x samplings x restart intervals", data, st, expect=dict(fast=0 if slow else 1)))
    assert len(out) == 48 and len({c.data for c in out}) == 48
    return out


# ---- files the stager must reject (host tests only) --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rejected_cases() -> List[Tuple[str, bytes, int]]:
    rng = np.random.default_rng(7)
    img = synth(rng, 32, 32)
    q = [q_ramp(4)]
    blk = jw.blocks_from_pixels(img, (1, 1), q)
    t, sel = tables_for((1, 1))
    good, _ = jw.write_jpeg(32, 32, (1, 1), blk, t, sel, quant=q)
    out = []
    t2 = {(0, 2): t[(0, 0)], (1, 0): t[(1, 0)]}
    out.append(("table_id_2", jw.write_jpeg(32, 32, (1, 1), blk, t2, [(2, 0)] * 3, quant=q)[0], ERR_UNSUPPORTED))
    out.append(("precision_12", jw.write_jpeg(32, 32, (1, 1), blk, t, sel, quant=q, precision=12)[0], ERR_UNSUPPORTED))
    sos = b"\xff\xda\x00\x0c\x03\x01\x00\x02\x00\x03\x00\x00\x3f\x00"
    assert good.count(sos) == 1
    out.append(("non_interleaved", good.replace(sos, b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"), ERR_UNSUPPORTED))
    for hv in [(1, 2), (4, 1)]:
        out.append((f"luma_{hv[0]}x{hv[1]}", jw.write_jpeg(32, 32, (1, 1), blk, t, sel, quant=q,
                                                         frame_sampling=[hv, (1, 1), (1, 1)])[0], ERR_UNSUPPORTED))
    out.append(("rgb_ids_no_jfif", jw.write_jpeg(32, 32, (1, 1), blk, t, sel, quant=q, jfif=False,
                                                 comp_ids=(ord("R"), ord("G"), ord("B")))[0], ERR_UNSUPPORTED))
    out.append(("too_many_rst", jw.write_jpeg(32, 32, (1, 1), blk, t, sel, quant=q, restart=4, extra_rst=2)[0],
                ERR_INVALID))
    return out
