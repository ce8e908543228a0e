"""CPU tests of the persistent GEMM kernels' stage-issuer arithmetic: csrc/gemm_stage_addr.h compiled for the host
(tests/gemm_stage_addr_emul.cpp), against a transcription of the per-piece formulas it replaced.

Sources: for both geometries (256 x 256 / 512 threads / 8 pieces, 128 x 192 / 256 threads / 10 pieces), every thread
and every piece: wave-uniform base + lane offset == the old tile base + soff[i], on a full tile and on ragged tiles
with 1, 63, 64, 65 and TM - 1 rows left (wave tiles wholly past M among them), dense and pitched rows, the first and
the last k-step, tiles at row 0 and at 2^31 / ld rows (bases past 32 bits); every piece stays inside its operand.
Tile order: the (n0, m0) of every tile of every workgroup equals the old walk, and every tile is visited once.
Origin queue: the origin handed to a tile's epilogue (GemmTileOrigins, the issuer one or two tiles ahead) is that
tile's, from one k-step per tile upwards.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_stage_addr_emul.cpp")
CXX = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
G256, GMID = 0, 1
I64, I32 = ctypes.c_int64, ctypes.c_int


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libgemm_stage_addr_emul.so")
    subprocess.check_call(CXX + ["-fPIC", "-shared", SRC, "-o", so])
    L = ctypes.CDLL(so)
    L.emul_check_sources.argtypes = [I32, I64, I32, I64, I64, I32, I64, I32, ctypes.c_void_p]
    L.emul_check_sources.restype = I64
    L.emul_check_tiles.argtypes = [I32] * 4
    L.emul_check_tiles.restype = I64
    L.emul_check_origin_queue.argtypes = [I32] * 6
    L.emul_check_origin_queue.restype = I64
    return L


def sources(L, geo, m, n, lda, ldw, n0, m0, kc):
    bad = np.zeros(4, np.int64)
    nbad = L.emul_check_sources(geo, m, n, lda, ldw, n0, m0, kc, bad.ctypes.data)
    assert nbad == 0, f"{nbad} pieces differ; first (tid, piece, want, got) = {bad.tolist()}"


@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("k", [64, 768])
@pytest.mark.parametrize("geo", [G256, GMID], ids=["g256", "gmid"])
def test_piece_sources_equal_the_old_formulas(emul, geo, k, pitched):
    tm, tn = emul.emul_tile_rows(geo), emul.emul_tile_cols(geo)
    lda, ldw = (k + 8, k + 16) if pitched else (k, k)
    far = 2 ** 31 // lda // tm                      # tile row whose base lies past 2^32 bytes
    assert far * tm * lda * 2 > 2 ** 32 - 2 * tm * lda
    for mtile in (0, 3, far):
        for left in (tm, 1, 63, 64, 65, tm - 1):    # rows of the matrix in this tile
            for kc in (0, k // 64 - 1):
                for n0 in (0, 2 * tn):
                    sources(emul, geo, mtile * tm + left, 3 * tn, lda, ldw, n0, mtile * tm, kc)


def test_a_wrong_clamp_is_seen(emul):
    """The check itself: a matrix one row SHORTER than the tile is told makes pieces differ or leave the operand."""
    bad = np.zeros(4, np.int64)
    assert emul.emul_check_sources(G256, 300, 256, 64, 64, 0, 256, 0, bad.ctypes.data) == 0
    assert emul.emul_check_sources(G256, 256, 256, 64, 64, 0, 256, 0, bad.ctypes.data) > 0   # m0 == m: no row left


@pytest.mark.parametrize("grid", [7, 8, 255, 256])
@pytest.mark.parametrize("tiles_m", [4, 5, 678])
@pytest.mark.parametrize("tiles_n", [1, 3, 6, 9, 12])
def test_tile_order_equals_the_old_walk(emul, tiles_n, tiles_m, grid):
    for geo in (G256, GMID):
        assert emul.emul_check_tiles(geo, tiles_n, tiles_m, grid) == 0


@pytest.mark.parametrize("nkc", [1, 2, 3, 12])
def test_epilogue_gets_its_own_tiles_origin(emul, nkc):
    for geo in (G256, GMID):
        for tiles_n, tiles_m, grid in ((1, 4, 8), (1, 4, 3), (3, 5, 7), (6, 5, 8), (12, 678, 256), (9, 678, 255), (1, 1, 1)):
            for wg in sorted({0, 1 % grid, grid // 2, grid - 1}):
                assert emul.emul_check_origin_queue(geo, tiles_n, tiles_m, grid, wg, nkc) == 0, (geo, tiles_n, tiles_m, grid, wg)


def test_stand_alone_program(emul):
    """The same translation unit with its own main(): the form a sanitizer build of it runs as."""
    exe = os.path.join(ROOT, "tests", "_build", "gemm_stage_addr_main")
    subprocess.check_call(CXX + ["-DGEMM_ADDR_MAIN", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
