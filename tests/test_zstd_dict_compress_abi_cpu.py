"""The C ABI of the Zstandard encoder with dictionaries (include/hipcomp/zstd_dict_compress.h,
lib/libhipcomp_zstd_dict_compress.so) without a GPU: its exports, the header as C99, the argument checks, the output
bound and the temp size."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_zstd_dict_compress.so")
HEADER = os.path.join(ROOT, "include", "hipcomp", "zstd_dict_compress.h")
DECLARED = {"hipcompBatchedZstdDictCompressGetPreparedSize", "hipcompBatchedZstdDictCompressPrepareAsync",
            "hipcompBatchedZstdDictCompressGetTempSize", "hipcompBatchedZstdDictCompressGetMaxOutputChunkSize",
            "hipcompBatchedZstdDictCompressAsync"}
INVALID = 10
MAX = 32768


def temp_bytes(chunks: int, max_chunk: int) -> int:
    """the formula of csrc/zstd_compress/zstd_compress_sizing.hpp, restated: the plain encoder's"""
    waves = min(chunks, 256 * 12)
    return waves * (8 * ((max_chunk // 4 + 64) // 64 * 64) + (max_chunk + 256) // 256 * 256)


def test_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_header_is_c99_and_states_the_limits(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/zstd_dict_compress.h"\n'
                   "int main(void) { size_t t = 1, p = 0; hipcompBatchedZstdOpts_t o = hipcompBatchedZstdDefaultOpts;\n"
                   "  return (int)hipcompBatchedZstdDictCompressGetTempSize(1, HIPCOMP_ZSTD_DICT_COMPRESS_MAX_CHUNK_BYTES, o, &t)\n"
                   "       + (int)hipcompBatchedZstdDictCompressGetPreparedSize(HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES, &p) + (int)t + (int)p; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "hipcomp/zstd_compress.h"']
    for word in ("32768", "65535", "shorter than 8 bytes", "Dictionary_ID", "n + 18", "Treeless", "Repeat_Mode", "NULL",
                 "invalid", "16-byte aligned", "HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES 14080", "repeat offsets 2 and 3",
                 "level 0", "hipcompErrorCannotDecompress", "Determinism".lower()):
        assert word in text, word


def test_argument_checks(hc):
    lib = hc.api.zstd_dict_compress_library()
    assert hc.api.zstd_dict_compress_library() is lib
    ok, summed = hc.api.ZstdOpts(0, 0), hc.api.ZstdOpts(0, 1)
    t = ctypes.c_size_t(7)
    p = 0x1000   # never dereferenced: a refused argument is refused before anything is launched
    assert lib.hipcompBatchedZstdDictCompressGetTempSize(10, MAX, ok, None) == INVALID
    assert lib.hipcompBatchedZstdDictCompressGetMaxOutputChunkSize(MAX, ok, None) == INVALID
    for k in (0, 1, 6, 7, 8):     # null pointers, each in turn; the prepared dictionaries' array among them
        args = [p, p, MAX, 1, p, 1 << 30, p, p, p, ok, None]
        args[k] = None
        assert lib.hipcompBatchedZstdDictCompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedZstdDictCompressAsync(p, p, MAX, 1, None, 1 << 30, p, p, p, ok, None) == INVALID   # temp
    for k in (0, 1, 3, 4, 5):
        args = [p, p, 1, p, p, p, None]
        args[k] = None
        assert lib.hipcompBatchedZstdDictCompressPrepareAsync(*args) == INVALID, k
    assert lib.hipcompBatchedZstdDictCompressPrepareAsync(p, p, 0, p, p, p, None) == 0
    # level = 1, checksum = 2 or -1, max chunk 32769
    for bad, mx in ((hc.api.ZstdOpts(1, 0), MAX), (hc.api.ZstdOpts(0, 2), MAX), (hc.api.ZstdOpts(0, -1), MAX),
                    (hc.api.ZstdOpts(-1, 1), MAX), (ok, MAX + 1), (ok, 65536), (summed, 1 << 40)):
        assert lib.hipcompBatchedZstdDictCompressGetTempSize(10, mx, bad, ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedZstdDictCompressGetMaxOutputChunkSize(mx, bad, ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedZstdDictCompressAsync(p, p, mx, 1, p, 1 << 30, p, p, p, bad, None) == INVALID
        assert lib.hipcompBatchedZstdDictCompressAsync(p, p, mx, 0, p, 1 << 30, p, p, p, bad, None) == INVALID   # (even an empty batch)
    assert t.value == 7
    need = lib.compress_temp_size(3, MAX)
    assert need > 0
    assert lib.hipcompBatchedZstdDictCompressAsync(p, p, MAX, 3, p, need - 1, p, p, p, ok, None) == INVALID
    for off in (1, 2, 3):
        assert lib.hipcompBatchedZstdDictCompressAsync(p, p, MAX, 3, p + off, need, p, p, p, summed, None) == INVALID
    # batch_size == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedZstdDictCompressAsync(p, p, MAX, 0, None, 0, p, p, p, ok, None) == 0
    assert lib.hipcompBatchedZstdDictCompressGetTempSize(10, MAX, summed, ctypes.byref(t)) == 0 and t.value == temp_bytes(10, MAX)


def test_output_bound_and_temp_size(hc):
    lib = hc.api.zstd_dict_compress_library()
    for n in (0, 1, 2, 100, 255, 256, 4096, 32767, 32768):
        assert lib.max_output_chunk_size(n) == n + 18
        assert lib.max_output_chunk_size(n, hc.api.ZstdOpts(0, 1)) == n + 18
    assert hc.batch.ZstdDictEncoder(checksum=True).max_output_chunk_size(MAX) == MAX + 18
    plain = hc.api.zstd_compress_library()
    for chunks in (0, 1, 100, 3072, 3073, 100000):
        for mx in (0, 1, 4, 255, 256, 4095, 32768):
            assert lib.compress_temp_size(chunks, mx) == temp_bytes(chunks, mx) == plain.compress_temp_size(chunks, mx), (chunks, mx)
    assert lib.compress_temp_size(1, MAX) % 4 == 0
