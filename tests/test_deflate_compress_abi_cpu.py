"""The C ABI of the Deflate encoder's library (include/hipcomp/deflate_compress.h,
lib/libhipcomp_deflate_compress.so) without a GPU: its exports, the header as C99, the argument checks, the output
bound and the temp size."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_deflate_compress.so")
HEADER = os.path.join(ROOT, "include", "hipcomp", "deflate_compress.h")
DECLARED = {"hipcompBatchedDeflateCompressGetTempSize", "hipcompBatchedDeflateCompressGetMaxOutputChunkSize",
            "hipcompBatchedDeflateCompressAsync"}
INVALID = 10


def test_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_header_is_c99_and_includes_only_hipcomp_h(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/deflate_compress.h"\n'
                   "int main(void) { size_t t = 1; hipcompBatchedDeflateOpts_t o = hipcompBatchedDeflateDefaultOpts;\n"
                   "  return (int)hipcompBatchedDeflateCompressGetTempSize(1, HIPCOMP_DEFLATE_COMPRESS_MAX_CHUNK_BYTES, o, &t) + (int)t; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "hipcomp.h"']
    for word in ("65536", "BFINAL", "Determinism", "Temp space", "Output bound", "gzip"):
        assert word in text, word


def test_argument_checks(hc):
    lib = hc.api.deflate_compress_library()
    assert hc.api.deflate_compress_library() is lib
    ok, bad = hc.api.DeflateOpts(0), hc.api.DeflateOpts(1)
    t = ctypes.c_size_t(7)
    p = 0x1000   # never dereferenced: a refused argument is refused before anything is launched
    # null pointers
    assert lib.hipcompBatchedDeflateCompressGetTempSize(10, 65536, ok, None) == INVALID
    assert lib.hipcompBatchedDeflateCompressGetMaxOutputChunkSize(65536, ok, None) == INVALID
    for k in (0, 1, 6, 7):
        args = [p, p, 65536, 1, p, 1 << 30, p, p, ok, None]
        args[k] = None
        assert lib.hipcompBatchedDeflateCompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedDeflateCompressAsync(p, p, 65536, 1, None, 1 << 30, p, p, ok, None) == INVALID   # temp
    # algo = 1
    assert lib.hipcompBatchedDeflateCompressGetTempSize(10, 65536, bad, ctypes.byref(t)) == INVALID
    assert lib.hipcompBatchedDeflateCompressGetMaxOutputChunkSize(65536, bad, ctypes.byref(t)) == INVALID
    assert lib.hipcompBatchedDeflateCompressAsync(p, p, 65536, 1, p, 1 << 30, p, p, bad, None) == INVALID
    # max_chunk = 65537
    assert lib.hipcompBatchedDeflateCompressGetTempSize(10, 65537, ok, ctypes.byref(t)) == INVALID
    assert lib.hipcompBatchedDeflateCompressGetMaxOutputChunkSize(65537, ok, ctypes.byref(t)) == INVALID
    assert lib.hipcompBatchedDeflateCompressAsync(p, p, 65537, 1, p, 1 << 30, p, p, ok, None) == INVALID
    assert t.value == 7
    # a temp buffer smaller than the query's answer
    need = lib.compress_temp_size(3, 65536)
    assert need > 0
    assert lib.hipcompBatchedDeflateCompressAsync(p, p, 65536, 3, p, need - 1, p, p, ok, None) == INVALID
    # batch_size == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedDeflateCompressAsync(p, p, 65536, 0, None, 0, p, p, ok, None) == 0


def test_output_bound(hc):
    lib = hc.api.deflate_compress_library()
    assert [lib.max_output_chunk_size(n) for n in (0, 1, 65535, 65536)] == [5, 6, 65540, 65546]
    for n in (2, 100, 4096, 32768, 65534):
        assert lib.max_output_chunk_size(n) == n + 5 * max(1, -(-n // 65535))
    assert hc.batch.DeflateEncoder().max_output_chunk_size(65536) == 65546


def test_temp_size_is_bounded_by_the_waves_in_flight(hc):
    lib = hc.api.deflate_compress_library()
    sizes = [lib.compress_temp_size(b, 65536) for b in (1, 2, 100, 1000, 100000, 1000000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[1] == 2 * sizes[0]
    assert lib.compress_temp_size(100000, 65536) == lib.compress_temp_size(1000000, 65536)
    assert sizes[-1] <= 8192 * sizes[0]
    assert lib.compress_temp_size(0, 65536) == 0
    assert hc.batch.DeflateEncoder().compress_temp_size(7, 4096) == lib.compress_temp_size(7, 4096) <= lib.compress_temp_size(7, 65536)
