"""The C ABI of the Zstandard dictionary decoder's library (include/hipcomp/zstd_dict.h, lib/libhipcomp_zstd_dict.so)
without a GPU: its exports, the header as C99, the host-side errors and the two size queries."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_zstd_dict.so")
HEADER = os.path.join(ROOT, "include", "hipcomp", "zstd_dict.h")
DECLARED = {"hipcompBatchedZstdDictGetPreparedSize", "hipcompBatchedZstdDictPrepareAsync",
            "hipcompBatchedZstdDictDecompressGetTempSize", "hipcompBatchedZstdDictGetDecompressSizeAsync",
            "hipcompBatchedZstdDictDecompressAsync"}
INVALID = 10


def test_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_header_is_c99_and_includes_only_hipcomp_h(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/zstd_dict.h"\n'
                   "int main(void) { size_t t = 1; return (int)hipcompBatchedZstdDictGetPreparedSize(1, &t) + (int)t; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "hipcomp.h"']
    for word in ("Dictionary_ID", "RAW CONTENT", "FORMATTED", "PREPARED BLOB", "Documented differences", "Containment",
                 "prepare never wrote", "0xEC30A437") + tuple(DECLARED):
        assert word in text, word


def test_argument_checks(hc):
    lib = hc.api.zstd_dict_library()
    assert hc.api.zstd_dict_library() is lib
    p = 0x1000   # never dereferenced: a refused argument is refused before anything is launched
    assert lib.hipcompBatchedZstdDictGetPreparedSize(10, None) == INVALID
    assert lib.hipcompBatchedZstdDictDecompressGetTempSize(10, 65536, None) == INVALID
    for k in (0, 1, 3, 4, 5):
        args = [p, p, 1, p, p, p, None]
        args[k] = None
        assert lib.hipcompBatchedZstdDictPrepareAsync(*args) == INVALID, k
    for k in (0, 1, 2, 3):
        args = [p, p, p, p, 1, None]
        args[k] = None
        assert lib.hipcompBatchedZstdDictGetDecompressSizeAsync(*args) == INVALID, k
    for k in (0, 1, 2, 7, 9):
        args = [p, p, p, p, 1, p, 1 << 30, p, p, p, None]
        args[k] = None
        assert lib.hipcompBatchedZstdDictDecompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedZstdDictDecompressAsync(p, p, p, p, 1, None, 1 << 30, p, p, p, None) == INVALID   # temp
    need = lib.decompress_temp_size(3, 1)
    assert lib.hipcompBatchedZstdDictDecompressAsync(p, p, p, p, 3, p, need - 1, p, p, p, None) == INVALID
    # batch_size == 0 and num_dicts == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedZstdDictDecompressAsync(p, p, p, p, 0, None, 0, p, p, p, None) == 0
    assert lib.hipcompBatchedZstdDictGetDecompressSizeAsync(p, p, p, p, 0, None) == 0
    assert lib.hipcompBatchedZstdDictPrepareAsync(p, p, 0, p, p, p, None) == 0


def test_size_queries(hc):
    lib = hc.api.zstd_dict_library()
    for n in (0, 1, 15, 16, 17, 4096, 16 * 1024, 112640, 1 << 30):
        assert lib.prepared_size(n) == 9280 + -(-n // 16) * 16, n
    out = ctypes.c_size_t(7)
    assert lib.hipcompBatchedZstdDictGetPreparedSize((1 << 30) + 1, ctypes.byref(out)) == INVALID and out.value == 7
    # the temp space is that of the decoder without dictionaries
    plain = hc.api.zstd_library()
    for chunks in (0, 1, 100, 3071, 3072, 3073, 100000):
        for max_chunk in (0, 1, 256, 257, 65536, 128 * 1024 + 1, 300 * 1024):
            assert lib.decompress_temp_size(chunks, max_chunk) == plain.decompress_temp_size(chunks, max_chunk)
    assert hc.batch.ZstdDictDecoder().decompress_temp_size(7, 4096) == 7 * 4096
