"""The C ABI of the Zstandard decoder's library (include/hipcomp/zstd.h, lib/libhipcomp_zstd.so) without a GPU: its
exports, the header as C99, the host-side errors and the temp size."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_zstd.so")
HEADER = os.path.join(ROOT, "include", "hipcomp", "zstd.h")
DECLARED = {"hipcompBatchedZstdDecompressGetTempSize", "hipcompBatchedZstdGetDecompressSizeAsync",
            "hipcompBatchedZstdDecompressAsync"}
INVALID = 10


def test_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_header_is_c99_and_includes_only_hipcomp_h(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/zstd.h"\n'
                   "int main(void) { size_t t = 1; return (int)hipcompBatchedZstdDecompressGetTempSize(1, 65536, &t) + (int)t; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "hipcomp.h"']
    for word in ("Skippable", "Dictionary_ID", "XXH64", "Documented differences", "Containment", "DECLARED"):
        assert word in text, word


def test_argument_checks(hc):
    lib = hc.api.zstd_library()
    assert hc.api.zstd_library() is lib
    p = 0x1000   # never dereferenced: a refused argument is refused before anything is launched
    assert lib.hipcompBatchedZstdDecompressGetTempSize(10, 65536, None) == INVALID
    for k in (0, 1, 2):
        args = [p, p, p, 1, None]
        args[k] = None
        assert lib.hipcompBatchedZstdGetDecompressSizeAsync(*args) == INVALID, k
    for k in (0, 1, 2, 7):
        args = [p, p, p, p, 1, p, 1 << 30, p, p, None]
        args[k] = None
        assert lib.hipcompBatchedZstdDecompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedZstdDecompressAsync(p, p, p, p, 1, None, 1 << 30, p, p, None) == INVALID   # temp
    need = lib.decompress_temp_size(3, 1)
    assert lib.hipcompBatchedZstdDecompressAsync(p, p, p, p, 3, p, need - 1, p, p, None) == INVALID
    # batch_size == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedZstdDecompressAsync(p, p, p, p, 0, None, 0, p, p, None) == 0
    assert lib.hipcompBatchedZstdGetDecompressSizeAsync(p, p, p, 0, None) == 0


def test_temp_size_against_a_restatement(hc):
    lib = hc.api.zstd_library()
    waves = 256 * 3 * 4     # 256 CUs, 3 workgroups of 4 waves by the kernel's LDS

    def restated(chunks, max_chunk):
        return min(chunks, waves) * (-(-min(max_chunk, 128 * 1024) // 256) * 256)
    for chunks in (0, 1, 2, 100, waves - 1, waves, waves + 1, 100000, 1000000):
        for max_chunk in (0, 1, 256, 257, 4096, 65536, 128 * 1024, 128 * 1024 + 1, 300 * 1024, 1 << 30):
            assert lib.decompress_temp_size(chunks, max_chunk) == restated(chunks, max_chunk), (chunks, max_chunk)
    assert hc.batch.ZstdDecoder().decompress_temp_size(7, 4096) == 7 * 4096
