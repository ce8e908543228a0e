"""jpeg_writer.py - TEST INFRASTRUCTURE.  A coefficient-level writer of baseline / extended-sequential JPEG files
(ITU T.81), the JPEG counterpart of png_writer.py / deflate_writer.py: the tests hand it quantised coefficients and
Huffman tables of their own choice and get streams no encoder writes (fixed-length codes, 16-bit codes in use, four
tables split across components, restart interval 1, fill bytes in front of RSTn, blocks without an EOB ...).
Pure Python + numpy; nothing of it is linked into the library.

    data, stats = write_jpeg(height, width, sampling, blocks, tables, ...)

`blocks[c]` is an int array [mcus_y * v_c, mcus_x * h_c, 64]: the component's quantised coefficients in ZIGZAG order,
DC values absolute (the writer forms the differences and resets the predictors at restart boundaries).
`tables` maps (tc, th) -> (bits[16], vals); tc 0 = DC, 1 = AC.  `stats` is the writer's own bookkeeping, which the
tests assert on so that no case is vacuous.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# zigzag position -> natural (row-major) index
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63], dtype=np.int64)

Table = Tuple[List[int], List[int]]

# code-length profiles of T.81 Annex K (K.3 luminance DC, K.5 luminance AC); the symbol ORDER is the caller's
DC_BITS_K3 = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
AC_BITS_K5 = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
ALL_AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


def canonical_codes(bits: Sequence[int], vals: Sequence[int]) -> Dict[int, Tuple[int, int]]:
    """symbol -> (code, length), T.81 Annex C: codes of one length are consecutive, each length starts at twice the
    end of the one before."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            assert code < (1 << ln), "more codes of one length than fit"
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return out


def table_from_lengths(pairs: Sequence[Tuple[int, int]]) -> Table:
    """(symbol, code length) pairs -> (bits, vals); symbols of one length keep the order given."""
    bits = [0] * 16
    for _, ln in pairs:
        bits[ln - 1] += 1
    vals = [s for ln in range(1, 17) for s, l2 in pairs if l2 == ln]
    canonical_codes(bits, vals)  # checks that the lengths fit
    return bits, vals


def ac_symbol_rank(sym: int) -> float:
    """Rough cost order of AC symbols in photographic content (small run + small size first, EOB in front)."""
    if sym == 0x00:
        return -1.0
    if sym == 0xF0:
        return 9.0
    return (sym >> 4) * 1.5 + (sym & 15) * 2.0


def generic_dc_table() -> Table:
    return list(DC_BITS_K3), list(range(12))


def generic_ac_table(reverse: bool = False) -> Table:
    """All 162 AC symbols on the K.5 length profile (long codes span 192 of the 16-bit prefixes); reverse=True puts
    the FREQUENT symbols on the 12- to 16-bit codes."""
    vals = sorted(ALL_AC_SYMBOLS, key=ac_symbol_rank, reverse=reverse)
    return list(AC_BITS_K5), vals


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v: int, n: int):
        self.acc = (self.acc << n) | v
        self.n += n
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def flush(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # 1-bit padding in front of a marker
        data, self.out = bytes(self.out), bytearray()
        return data


def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def component_layout(sampling) -> List[Tuple[int, int]]:
    """[(h, v)] per component: "grey" or the luma factors (1, 1) / (2, 1) / (2, 2) with 1x1 chroma."""
    if sampling == "grey":
        return [(1, 1)]
    return [tuple(sampling), (1, 1), (1, 1)]


def grid(height: int, width: int, sampling) -> Tuple[int, int]:
    h, v = component_layout(sampling)[0]
    return -(-height // (8 * v)), -(-width // (8 * h))


def write_jpeg(height: int, width: int, sampling, blocks: Sequence[np.ndarray], tables: Dict[Tuple[int, int], Table],
               selectors: Optional[Sequence[Tuple[int, int]]] = None, quant: Optional[Sequence[np.ndarray]] = None,
               quant_sel: Optional[Sequence[int]] = None, sof: int = 0xC0, restart: int = 0, fill: int = 0,
               precision: int = 8, jfif: bool = True, comp_ids: Sequence[int] = (1, 2, 3),
               frame_sampling: Optional[Sequence[Tuple[int, int]]] = None, extra_rst: int = 0):
    """Returns (file bytes, stats).  quant: tables [64] in NATURAL order (written 16-bit when a value needs it);
    selectors: (DC table id, AC table id) per component; fill: FF bytes put in front of every RSTn;
    precision / jfif / comp_ids / frame_sampling (the sampling bytes of the frame header, the blocks stay laid out by
    `sampling`) / extra_rst (RSTn markers appended behind the last interval) build files the stager must reject."""
    comps = component_layout(sampling)
    nc = len(comps)
    my, mx = grid(height, width, sampling)
    selectors = list(selectors) if selectors is not None else [(0, 0)] + [(1, 1)] * (nc - 1)
    quant = [np.asarray(q, dtype=np.int64) for q in (quant if quant is not None else [np.ones(64, np.int64)])]
    quant_sel = list(quant_sel) if quant_sel is not None else [0] * nc
    for c, (h, v) in enumerate(comps):
        assert blocks[c].shape == (my * v, mx * h, 64), (c, blocks[c].shape, (my * v, mx * h, 64))
    codes = {k: canonical_codes(*t) for k, t in tables.items()}

    out = bytearray(b"\xff\xd8")
    if jfif:
        out += _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tq, q in enumerate(quant):
        wide = bool((q > 255).any())
        body = q[ZIGZAG].astype(">u2" if wide else "u1").tobytes()
        out += _seg(0xDB, bytes([(16 if wide else 0) | tq]) + body)
    fs = list(frame_sampling) if frame_sampling is not None else comps
    frame = struct.pack(">BHHB", precision, height, width, nc)
    for c in range(nc):
        frame += bytes([comp_ids[c], (fs[c][0] << 4) | fs[c][1], quant_sel[c]])
    out += _seg(sof, frame)
    for (tc, th), (bits, vals) in tables.items():
        out += _seg(0xC4, bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))
    if restart:
        out += _seg(0xDD, struct.pack(">H", restart))
    scan = bytes([nc])
    for c in range(nc):
        scan += bytes([comp_ids[c], (selectors[c][0] << 4) | selectors[c][1]])
    out += _seg(0xDA, scan + b"\x00\x3f\x00")

    stats = dict(long_symbols={k: 0 for k in tables}, symbols=0, stuffed=0, zrl=0, no_eob=0, max_dc_cat=0,
                 max_ac_size=0, max_zero_run=0, segments=[], blocks=0, markers=0)
    bw = _Bits()
    pred = [0] * nc
    blk_lists = [b.tolist() for b in blocks]

    def emit(key, sym, extra, nextra):
        code, ln = codes[key][sym]
        bw.put(code, ln)
        if nextra:
            bw.put(extra, nextra)
        stats["symbols"] += 1
        if ln > 11:
            stats["long_symbols"][key] += 1

    def close_segment(last: bool):
        seg = bw.flush()
        stats["segments"].append(seg)
        stats["stuffed"] += seg.count(0xFF)
        out.extend(seg.replace(b"\xff", b"\xff\x00"))
        if not last:
            out.extend(b"\xff" * fill + bytes([0xFF, 0xD0 + (stats["markers"] & 7)]))
            stats["markers"] += 1

    nmcu = mx * my
    for mcu in range(nmcu):
        if restart and mcu and mcu % restart == 0:
            close_segment(False)
            pred = [0] * nc
        yy, xx = divmod(mcu, mx)
        for c, (h, v) in enumerate(comps):
            dck, ack = (0, selectors[c][0]), (1, selectors[c][1])
            for by in range(v):
                for bx in range(h):
                    z = blk_lists[c][yy * v + by][xx * h + bx]
                    d = z[0] - pred[c]
                    pred[c] = z[0]
                    s = abs(d).bit_length()
                    stats["max_dc_cat"] = max(stats["max_dc_cat"], s)
                    emit(dck, s, d if d >= 0 else d + (1 << s) - 1, s)
                    run = 0
                    for k in range(1, 64):
                        a = z[k]
                        if a == 0:
                            run += 1
                            continue
                        stats["max_zero_run"] = max(stats["max_zero_run"], run)
                        while run > 15:
                            emit(ack, 0xF0, 0, 0)
                            stats["zrl"] += 1
                            run -= 16
                        s = abs(a).bit_length()
                        stats["max_ac_size"] = max(stats["max_ac_size"], s)
                        emit(ack, (run << 4) | s, a if a >= 0 else a + (1 << s) - 1, s)
                        run = 0
                    if run:
                        emit(ack, 0x00, 0, 0)
                    else:
                        stats["no_eob"] += 1
                    stats["blocks"] += 1
    close_segment(True)
    for k in range(extra_rst):
        out.extend(bytes([0xFF, 0xD0 + ((stats["markers"] + k) & 7), 0x5A]))
    out += b"\xff\xd9"
    stats["stream_bytes"] = sum(len(s) for s in stats["segments"])
    return bytes(out), stats


# ---- from pixels to coefficients: float64 forward DCT + quantisation ------------------------------------------------
def _dct_matrix() -> np.ndarray:
    k, n = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    c = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    c[0] *= np.sqrt(0.5)
    return c


_C = _dct_matrix()


def _plane_blocks(plane: np.ndarray, q_nat: np.ndarray) -> np.ndarray:
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128.0
    coef = np.einsum("ij,yxjk,lk->yxil", _C, b, _C).reshape(by, bx, 64)
    qc = np.rint(coef / q_nat.astype(np.float64)).astype(np.int64)
    return qc[..., ZIGZAG]


def blocks_from_pixels(img: np.ndarray, sampling, quant: Sequence[np.ndarray],
                       quant_sel: Optional[Sequence[int]] = None) -> List[np.ndarray]:
    """uint8 [H, W] (grey) or [H, W, 3] (RGB) -> per-component zigzag blocks: JFIF YCbCr, edge replication up to the
    MCU grid, box-filter chroma downsampling, float64 DCT-II, round(coef / q)."""
    comps = component_layout(sampling)
    quant_sel = list(quant_sel) if quant_sel is not None else [0] * len(comps)
    a = np.asarray(img, dtype=np.float64)
    if sampling == "grey":
        assert a.ndim == 2
        planes = [a]
    else:
        r, g, b = a[..., 0], a[..., 1], a[..., 2]
        planes = [0.299 * r + 0.587 * g + 0.114 * b,
                  -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0,
                  0.5 * r - 0.418688 * g - 0.081312 * b + 128.0]
    hmax, vmax = comps[0]
    my, mx = grid(a.shape[0], a.shape[1], sampling)
    out = []
    for c, (h, v) in enumerate(comps):
        p = planes[c]
        p = np.pad(p, ((0, my * 8 * vmax - p.shape[0]), (0, mx * 8 * hmax - p.shape[1])), mode="edge")
        fy, fx = vmax // v, hmax // h
        if fy > 1 or fx > 1:
            p = p.reshape(p.shape[0] // fy, fy, p.shape[1] // fx, fx).mean(axis=(1, 3))
        out.append(_plane_blocks(p, np.asarray(quant[quant_sel[c]])))
    return out
