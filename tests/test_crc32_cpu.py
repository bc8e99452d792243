"""The CRC-32 math of the high-level managers' checksums (hipcomp-core_amd/csrc/crc32_math.hpp) on the CPU,
against zlib.crc32 (IEEE 802.3: reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF).
The header is compiled with tests/crc32_driver.cpp alone (g++, standard headers, no HIP): the slice tables,
the bytewise and slice-by-16 forms, crc32_shift and the many-part XOR that the kernels build with atomicXor."""
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
CXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
POLY = 0xEDB88320


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crc32") / "crc32_driver")
    r = subprocess.run(CXX + ["-O1", os.path.join(TESTS, "crc32_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stderr)
    return r.stdout


def _raw(data: bytes, reg: int = 0) -> int:
    """The CRC register after `data` from `reg`, without conditioning (zlib.crc32 conditions both ends)."""
    return ~zlib.crc32(data, ~reg & 0xFFFFFFFF) & 0xFFFFFFFF


def test_slice_tables_are_the_byte_table_followed_by_zero_bytes(driver):
    rows = [[int(w, 16) for w in line.split()] for line in _run(driver, "tables").splitlines()]
    assert len(rows) == 16 and all(len(r) == 256 for r in rows)
    for k in range(16):
        for b in range(256):
            assert rows[k][b] == _raw(bytes([b]) + bytes(k)), (k, b)


@pytest.mark.parametrize("n", [0, 1, 3, 15, 16, 17, 31, 32, 33, 255, 4096, 65536 + 7])
def test_plain_and_sliced_crc_equal_zlib(driver, tmp_path, n):
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    p = tmp_path / "d"
    p.write_bytes(data)
    got = [int(v) for v in _run(driver, "crc", p).split()]
    assert got == [zlib.crc32(data)] * 17


def _py_shift(crc: int, n: int) -> int:
    """crc * x^(8n) mod P, written out again here: square and multiply in the reflected representation."""
    def mul(a, b):
        p = 0
        for k in range(31, -1, -1):
            if (a >> k) & 1:
                p ^= b
            b = (b >> 1) ^ (POLY if b & 1 else 0)
        return p
    sq = 1 << 30                  # x^1
    for _ in range(3):
        sq = mul(sq, sq)          # x^8
    while n:
        if n & 1:
            crc = mul(sq, crc)
        sq = mul(sq, sq)
        n >>= 1
    return crc


@pytest.mark.parametrize("la,lb", [(0, 0), (5, 0), (0, 5), (1, 1), (3, 3), (100, 65536), (65536, 1), (65536, 65536)])
def test_shift_joins_two_crcs_as_zlib_sees_the_concatenation(driver, la, lb):
    rng = np.random.default_rng(la * 7 + lb)
    a = rng.integers(0, 256, la, dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, lb, dtype=np.uint8).tobytes()
    shifted = int(_run(driver, "shift", zlib.crc32(a), lb))
    assert shifted ^ zlib.crc32(b) == zlib.crc32(a + b)
    # and the shift by lb bytes is the CRC register run over lb zero bytes, from zero
    assert shifted == _raw(bytes(lb), zlib.crc32(a)) or lb == 0


@pytest.mark.parametrize("n", [(1 << 32) + 1, (1 << 32) * 3 + 12345, (1 << 40) + (1 << 33) + 7, (1 << 63) + 1, (1 << 64) - 1])
def test_shift_beyond_four_gib(driver, n):
    c = 0x9E3779B9
    got = int(_run(driver, "shift", c, n))
    assert got == _py_shift(c, n)
    # composition: the shift by a + b is the shift by a then by b
    a = n // 3
    assert int(_run(driver, "shift", int(_run(driver, "shift", c, a)), n - a)) == got


def test_many_parts_xor_formula_with_unequal_lengths(driver, tmp_path):
    rng = np.random.default_rng(1)
    lens = [0, 1, 3, 4096, 17, 0, 65536, 65535, 2, 1000]
    data = rng.integers(0, 256, sum(lens), dtype=np.uint8).tobytes()
    p = tmp_path / "d"
    p.write_bytes(data)
    assert int(_run(driver, "parts", p, *lens)) == zlib.crc32(data)
    # the same in Python from zlib's per-part values (the order of the XOR does not matter)
    full, at = 0, 0
    parts = []
    for ln in lens:
        parts.append((zlib.crc32(data[at:at + ln]), len(data) - at - ln))
        at += ln
    for crc, behind in reversed(parts):
        full ^= int(_run(driver, "shift", crc, behind))
    assert full == zlib.crc32(data)
    assert int(_run(driver, "parts", p, len(data))) == zlib.crc32(data)
