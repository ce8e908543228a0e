"""The LDS layout of the transposed-read kernels (csrc/tr_layout.h: gemm_tn.hip, conv_bwd.hip, stem_train.hip) on the
CPU: the fill is a permutation of each row, the transposed reads find what the fill stored, and the reads of a half-wave
are free of bank conflicts.  A wrong XOR key leaves every output correct and the kernel merely slow, so the last
property is the one no GPU test can see; one negative case per width shows that this test can.  No GPU."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (bytes per row, rows of the staged tile): stem_train's [256][64], conv_bwd's [64][128] (and [64][64] at 128 B),
# gemm_tn's [64][256] fp16
TILES = [(128, 256), (256, 64), (512, 64)]
OTHER = {128: 256, 256: 128, 512: 128}     # the width whose key is the wrong one


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtr_layout_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "tr_layout_emul.cpp"), "-o", so])
    return ctypes.CDLL(so)


def _read_addr(rowb, row, c32, p4, key):
    """tr_read_off with the key given: pinned to the header by test_read_finds_what_fill_stored."""
    return row * rowb + ((c32 ^ key) << 5) + 8 * p4


def _bank_loads(emul, rowb, rows, addr):
    """For every transposed read (ks, hf, c32) of the tile and each 32-lane half: the number of distinct dword
    addresses each of the 64 banks receives.  Bank of byte a: (a / 4) % 64; a lane reads the 8 B at its address, so
    it touches the banks of a and a + 4; equal addresses broadcast (cdna_hip_programming.md §2)."""
    for ks in range(rows // 32):
        for hf in range(2):
            for c32 in range(rowb // 32):
                for half in range(2):
                    banks = [set() for _ in range(64)]
                    for lane in range(32 * half, 32 * half + 32):
                        a = addr(emul.emul_tr_lane_row(lane, ks, hf), c32, emul.emul_tr_lane_p4(lane))
                        assert a % 8 == 0
                        for dword in (a // 4, a // 4 + 1):
                            banks[dword % 64].add(dword)
                    yield (ks, hf, c32, half), [len(b) for b in banks]


def test_unsupported_width_is_refused_by_the_emulation(emul):
    assert emul.emul_tr_key(64, 0) == -1 and emul.emul_tr_fill_off(1024, 0, 0) == -1


def test_lane_decomposition(emul):
    # lane = 16 g + 4 q + p: row 32 ks + 8 g + 4 hf + q, piece p; the 64 lanes of the two reads of a substep cover its
    # 32 rows, four lanes (the four 8-B pieces of the 32-B chunk) on each
    for ks in range(8):
        seen = {}
        for hf in range(2):
            for lane in range(64):
                row = emul.emul_tr_lane_row(lane, ks, hf)
                assert row == 32 * ks + 8 * (lane >> 4) + 4 * hf + ((lane >> 2) & 3)
                seen.setdefault(row, []).append(emul.emul_tr_lane_p4(lane))
        assert sorted(seen) == list(range(32 * ks, 32 * ks + 32))
        assert all(sorted(p) == [0, 1, 2, 3] for p in seen.values())


@pytest.mark.parametrize("rowb,rows", TILES)
def test_fill_is_a_permutation_of_each_row(emul, rowb, rows):
    for row in range(rows):
        offs = sorted(emul.emul_tr_fill_off(rowb, row, ch16) for ch16 in range(rowb // 16))
        assert offs == [row * rowb + 16 * slot for slot in range(rowb // 16)]


@pytest.mark.parametrize("rowb,rows", TILES)
def test_read_finds_what_fill_stored(emul, rowb, rows):
    for row in range(rows):
        for c32 in range(rowb // 32):
            lo, hi = (emul.emul_tr_fill_off(rowb, row, 2 * c32 + i) for i in range(2))
            assert hi == lo + 16 and lo % 32 == 0          # the two halves of a 32-B chunk stay one aligned pair
            for p4 in range(4):
                off = emul.emul_tr_read_off(rowb, row, c32, p4)
                assert off == lo + 8 * p4
                assert off == _read_addr(rowb, row, c32, p4, emul.emul_tr_key(rowb, row))


@pytest.mark.parametrize("rowb,rows", TILES)
def test_reads_are_free_of_bank_conflicts(emul, rowb, rows):
    # 32 lanes x 2 dwords on 64 banks: exactly one address per bank, for every read of the tile
    for where, loads in _bank_loads(emul, rowb, rows, lambda row, c32, p4: emul.emul_tr_read_off(rowb, row, c32, p4)):
        assert loads == [1] * 64, (rowb, where)


@pytest.mark.parametrize("rowb,rows", TILES)
def test_the_other_widths_key_is_seen_to_conflict(emul, rowb, rows):
    # the same reads with the key of the other row width (cut to this width's chunks): data still found - XOR with any
    # key below the chunk count is a permutation - but some bank gets two addresses
    chunks = rowb // 32

    def wrong(row, c32, p4):
        return _read_addr(rowb, row, c32, p4, emul.emul_tr_key(OTHER[rowb], row) & (chunks - 1))

    for row in range(rows):
        assert sorted(wrong(row, c32, 0) for c32 in range(chunks)) == [row * rowb + 32 * c for c in range(chunks)]
    worst = max(max(loads) for _, loads in _bank_loads(emul, rowb, rows, wrong))
    assert worst > 1, rowb
