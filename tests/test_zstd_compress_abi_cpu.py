"""The C ABI of the Zstandard encoder's library (include/hipcomp/zstd_compress.h,
lib/libhipcomp_zstd_compress.so) without a GPU: its exports, the header as C99, the argument checks, the output
bound and the temp size."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_zstd_compress.so")
HEADER = os.path.join(ROOT, "include", "hipcomp", "zstd_compress.h")
DECLARED = {"hipcompBatchedZstdCompressGetTempSize", "hipcompBatchedZstdCompressGetMaxOutputChunkSize",
            "hipcompBatchedZstdCompressAsync"}
INVALID = 10


def temp_bytes(chunks: int, max_chunk: int) -> int:
    """the formula of csrc/zstd_compress/zstd_compress_sizing.hpp, restated"""
    waves = min(chunks, 256 * 12)
    return waves * (8 * ((max_chunk // 4 + 64) // 64 * 64) + (max_chunk + 256) // 256 * 256)


def test_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_header_is_c99_and_includes_only_hipcomp_h(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/zstd_compress.h"\n'
                   "int main(void) { size_t t = 1; hipcompBatchedZstdOpts_t o = hipcompBatchedZstdDefaultOpts;\n"
                   "  return (int)hipcompBatchedZstdCompressGetTempSize(1, HIPCOMP_ZSTD_COMPRESS_MAX_CHUNK_BYTES, o, &t) + (int)t + o.level + o.checksum; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "hipcomp.h"']
    for word in ("65536", "Single_Segment", "Last_Block", "XXH64", "Determinism", "Temp space", "Output bound", "n + 14",
                 "RLE_Block", "Raw_Block", "28 b5 2f fd 20 00 01 00 00"):
        assert word in text, word


def test_argument_checks(hc):
    lib = hc.api.zstd_compress_library()
    assert hc.api.zstd_compress_library() is lib
    ok, summed = hc.api.ZstdOpts(0, 0), hc.api.ZstdOpts(0, 1)
    t = ctypes.c_size_t(7)
    p = 0x1000   # never dereferenced: a refused argument is refused before anything is launched
    # null pointers, each in turn
    assert lib.hipcompBatchedZstdCompressGetTempSize(10, 65536, ok, None) == INVALID
    assert lib.hipcompBatchedZstdCompressGetMaxOutputChunkSize(65536, ok, None) == INVALID
    for k in (0, 1, 6, 7):
        args = [p, p, 65536, 1, p, 1 << 30, p, p, ok, None]
        args[k] = None
        assert lib.hipcompBatchedZstdCompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedZstdCompressAsync(p, p, 65536, 1, None, 1 << 30, p, p, ok, None) == INVALID   # temp
    # level = 1, checksum = 2 or -1, max chunk 65537
    for bad, mx in ((hc.api.ZstdOpts(1, 0), 65536), (hc.api.ZstdOpts(0, 2), 65536), (hc.api.ZstdOpts(0, -1), 65536),
                    (hc.api.ZstdOpts(-1, 1), 65536), (ok, 65537), (summed, 1 << 40)):
        assert lib.hipcompBatchedZstdCompressGetTempSize(10, mx, bad, ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedZstdCompressGetMaxOutputChunkSize(mx, bad, ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedZstdCompressAsync(p, p, mx, 1, p, 1 << 30, p, p, bad, None) == INVALID
        assert lib.hipcompBatchedZstdCompressAsync(p, p, mx, 0, p, 1 << 30, p, p, bad, None) == INVALID   # (even an empty batch)
    assert t.value == 7
    # a temp buffer smaller than the query's answer, and a misaligned one
    need = lib.compress_temp_size(3, 65536)
    assert need > 0
    assert lib.hipcompBatchedZstdCompressAsync(p, p, 65536, 3, p, need - 1, p, p, ok, None) == INVALID
    for off in (1, 2, 3):
        assert lib.hipcompBatchedZstdCompressAsync(p, p, 65536, 3, p + off, need, p, p, summed, None) == INVALID
    # batch_size == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedZstdCompressAsync(p, p, 65536, 0, None, 0, p, p, ok, None) == 0
    assert lib.hipcompBatchedZstdCompressAsync(p, p, 65536, 0, None, 0, p, p, summed, None) == 0
    assert lib.hipcompBatchedZstdCompressGetTempSize(10, 65536, summed, ctypes.byref(t)) == 0 and t.value == temp_bytes(10, 65536)


def test_output_bound(hc):
    lib = hc.api.zstd_compress_library()
    for n in (0, 1, 2, 100, 255, 256, 4096, 32768, 65534, 65535, 65536):
        assert lib.max_output_chunk_size(n) == n + 14
        assert lib.max_output_chunk_size(n, hc.api.ZstdOpts(0, 1)) == n + 14
    assert hc.batch.ZstdEncoder().max_output_chunk_size(65536) == 65550
    assert hc.batch.ZstdEncoder(checksum=True).max_output_chunk_size(65536) == 65550


def test_temp_size_is_the_restated_formula_and_bounded_by_the_waves_in_flight(hc):
    lib = hc.api.zstd_compress_library()
    for chunks in (0, 1, 2, 100, 3071, 3072, 3073, 100000, 1000000):
        for mx in (0, 1, 3, 4, 255, 256, 1000, 4095, 65535, 65536):
            assert lib.compress_temp_size(chunks, mx) == temp_bytes(chunks, mx), (chunks, mx)
    assert lib.compress_temp_size(100000, 65536) == lib.compress_temp_size(3072, 65536) == 3072 * lib.compress_temp_size(1, 65536)
    assert lib.compress_temp_size(1, 65536) % 4 == 0
    assert hc.batch.ZstdEncoder(checksum=True).compress_temp_size(7, 4096) == lib.compress_temp_size(7, 4096) <= lib.compress_temp_size(7, 65536)
