"""The C ABI of the gzip / zlib / BGZF library (include/hipcomp/gzip.h, lib/libhipcomp_gzip.so) without a GPU: its
exports, what it links, the header as C99, the argument checks, the output bound, the temp sizes and the host's
BGZF splitter."""
import ctypes
import os
import subprocess

import gzip_membergen as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_gzip.so")
HEADER = os.path.join(ROOT, "include", "hipcomp", "gzip.h")
DECLARED = {"hipcompBatchedGzipDecompressGetTempSize", "hipcompBatchedGzipGetDecompressSizeAsync",
            "hipcompBatchedGzipDecompressAsync", "hipcompBatchedGzipCompressGetTempSize",
            "hipcompBatchedGzipCompressGetMaxOutputChunkSize", "hipcompBatchedGzipCompressAsync",
            "hipcompBgzfSplitHost"}
INVALID = 10


def test_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_library_links_the_two_deflate_libraries():
    """one copy of the Deflate kernels: both libraries are NEEDED and found next to this one"""
    out = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    needed = [line for line in out.splitlines() if "(NEEDED)" in line]
    assert any("[libhipcomp_deflate.so]" in line for line in needed), needed
    assert any("[libhipcomp_deflate_compress.so]" in line for line in needed), needed
    paths = [line for line in out.splitlines() if "(RUNPATH)" in line or "(RPATH)" in line]
    assert paths and all("$ORIGIN" in line for line in paths), paths
    # and it defines none of their kernels itself
    syms = subprocess.run(["nm", "-C", LIB], capture_output=True, text=True, check=True).stdout
    assert "deflate_launch" not in syms


def test_header_is_c99_and_includes_only_hipcomp_h(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/gzip.h"\n'
                   "int main(void) { size_t t = 1; hipcompBatchedGzipOpts_t o = hipcompBatchedGzipDefaultOpts;\n"
                   "  o.wrapper = HIPCOMP_WRAPPER_BGZF;\n"
                   "  return (int)hipcompBatchedGzipCompressGetTempSize(1, HIPCOMP_BGZF_MAX_CHUNK_BYTES, o, &t) + (int)t\n"
                   "         + hipcompBgzfEofBlock[HIPCOMP_BGZF_EOF_BLOCK_BYTES - 1]; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "hipcomp.h"']
    for word in ("One member per chunk", "difference from zlib", "Multi-member", "hipcompBgzfEofBlock", "65280",
                 "hipcompErrorBadChecksum", "Determinism", "Temp space", "Output bound"):
        assert word in text, word
    eof = text.split("hipcompBgzfEofBlock[HIPCOMP_BGZF_EOF_BLOCK_BYTES] = {")[1].split("}")[0]
    assert bytes(int(v, 16) for v in eof.replace("\n", " ").split(",")) == M.BGZF_EOF


def test_argument_checks(hc):
    lib = hc.api.gzip_library()
    assert hc.api.gzip_library() is lib
    O = hc.api.GzipOpts
    t = ctypes.c_size_t(7)
    p = 0x1000   # never dereferenced: a refused argument is refused before anything is launched
    big = 1 << 30
    # null pointers
    assert lib.hipcompBatchedGzipDecompressGetTempSize(10, 65536, None) == INVALID
    assert lib.hipcompBatchedGzipCompressGetTempSize(10, 65536, O(0), None) == INVALID
    assert lib.hipcompBatchedGzipCompressGetMaxOutputChunkSize(65536, O(0), None) == INVALID
    for k in (0, 1, 6, 7):
        args = [p, p, 65536, 1, p, big, p, p, O(0), None]
        args[k] = None
        assert lib.hipcompBatchedGzipCompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedGzipCompressAsync(p, p, 65536, 1, None, big, p, p, O(0), None) == INVALID   # temp
    for k in (0, 1, 2, 7):     # (actual and statuses, 3 and 8, may be NULL)
        args = [p, p, p, p, 1, p, big, p, p, 0, None]
        args[k] = None
        assert lib.hipcompBatchedGzipDecompressAsync(*args) == INVALID, k
    assert lib.hipcompBatchedGzipDecompressAsync(p, p, p, p, 1, None, big, p, p, 0, None) == INVALID     # temp
    for k in (0, 1, 2):
        args = [p, p, p, 1, 0, p, big, None]
        args[k] = None
        assert lib.hipcompBatchedGzipGetDecompressSizeAsync(*args) == INVALID, k
    assert lib.hipcompBatchedGzipGetDecompressSizeAsync(p, p, p, 1, 0, None, big, None) == INVALID       # temp
    # an unknown wrapper
    for w in (-1, 3, 255):
        assert lib.hipcompBatchedGzipCompressGetTempSize(10, 65536, O(w), ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedGzipCompressGetMaxOutputChunkSize(65536, O(w), ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedGzipCompressAsync(p, p, 65536, 1, p, big, p, p, O(w), None) == INVALID
        assert lib.hipcompBatchedGzipDecompressAsync(p, p, p, p, 1, p, big, p, p, w, None) == INVALID
        assert lib.hipcompBatchedGzipGetDecompressSizeAsync(p, p, p, 1, w, p, big, None) == INVALID
    # the chunk limits: 65536, and 65280 for BGZF
    for w, limit in ((0, 65536), (1, 65536), (2, 65280)):
        assert lib.hipcompBatchedGzipCompressGetTempSize(10, limit, O(w), ctypes.byref(t)) == 0
        t.value = 7
        assert lib.hipcompBatchedGzipCompressGetTempSize(10, limit + 1, O(w), ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedGzipCompressGetMaxOutputChunkSize(limit + 1, O(w), ctypes.byref(t)) == INVALID
        assert lib.hipcompBatchedGzipCompressAsync(p, p, limit + 1, 1, p, big, p, p, O(w), None) == INVALID
        assert t.value == 7
    # a temp buffer smaller than the query's answer, and a misaligned one
    need = lib.compress_temp_size(3, 65536)
    assert need > 0
    assert lib.hipcompBatchedGzipCompressAsync(p, p, 65536, 3, p, need - 1, p, p, O(0), None) == INVALID
    assert lib.hipcompBatchedGzipCompressAsync(p, p, 65536, 3, p + 4, need, p, p, O(0), None) == INVALID
    need = lib.decompress_temp_size(3, 65536)
    assert need > 0
    assert lib.hipcompBatchedGzipDecompressAsync(p, p, p, p, 3, p, need - 1, p, p, 0, None) == INVALID
    assert lib.hipcompBatchedGzipDecompressAsync(p, p, p, p, 3, p + 4, need, p, p, 0, None) == INVALID
    assert lib.hipcompBatchedGzipGetDecompressSizeAsync(p, p, p, 3, 0, p, need - 1, None) == INVALID
    assert lib.hipcompBatchedGzipGetDecompressSizeAsync(p, p, p, 3, 0, p + 1, need, None) == INVALID
    # batch_size == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedGzipCompressAsync(p, p, 65536, 0, None, 0, p, p, O(2 - 2), None) == 0
    assert lib.hipcompBatchedGzipDecompressAsync(p, p, p, None, 0, None, 0, p, None, 2, None) == 0
    assert lib.hipcompBatchedGzipGetDecompressSizeAsync(p, p, p, 0, 1, None, 0, None) == 0
    # the splitter's own
    assert lib.hipcompBgzfSplitHost(None, 5, None, 0, ctypes.byref(t), ctypes.byref(t)) == INVALID
    assert lib.hipcompBgzfSplitHost(b"x", 1, None, 1, ctypes.byref(t), ctypes.byref(t)) == INVALID
    assert lib.hipcompBgzfSplitHost(b"x", 1, None, 0, None, ctypes.byref(t)) == INVALID
    assert lib.hipcompBgzfSplitHost(b"x", 1, None, 0, ctypes.byref(t), None) == INVALID


def test_max_member_bytes(hc):
    lib = hc.api.gzip_library()
    raw = hc.api.deflate_compress_library()
    for n in (0, 1, 65280, 65535, 65536):
        bound = n + 5 * max(1, -(-n // 65535))
        assert raw.max_output_chunk_size(n) == bound
        for name, w, extra in (("gzip", 0, 18), ("zlib", 1, 6), ("bgzf", 2, 26)):
            if w == 2 and n > 65280:
                continue   # (refused: test_argument_checks)
            assert lib.max_output_chunk_size(n, w) == bound + extra, (n, name)
            assert hc.batch.GzipCodec(name).max_output_chunk_size(n) == bound + extra
    assert lib.max_output_chunk_size(65280, 2) <= 65536   # BSIZE can express a stored BGZF block


def test_temp_sizes_are_monotone_and_zero_for_an_empty_batch(hc):
    lib = hc.api.gzip_library()
    raw = hc.api.deflate_compress_library()
    batches = (0, 1, 2, 100, 1000, 100000, 1000000)
    for w in (0, 1, 2):
        sizes = [lib.compress_temp_size(b, 65280, w) for b in batches]
        assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] > 0
        for b, s in zip(batches, sizes):
            assert raw.compress_temp_size(b, 65280) + 8 * b <= s <= raw.compress_temp_size(b, 65280) + 8 * b + 8
        assert lib.compress_temp_size(7, 4096, w) <= lib.compress_temp_size(7, 65280, w)
    sizes = [lib.decompress_temp_size(b, 65536) for b in batches]
    assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] > 0
    assert sizes[3] == 100 * sizes[1]
    codec = hc.batch.GzipCodec("zlib")
    assert codec.compress_temp_size(7, 4096) == lib.compress_temp_size(7, 4096, 1)
    assert codec.decompress_temp_size(7, 4096) == lib.decompress_temp_size(7, 4096)


def test_bgzf_split_through_the_library(hc):
    lib = hc.api.gzip_library()
    chunks = [b"first block", b"", bytes(3000), b"last"]
    blocks = [M.bgzf_block(c) for c in chunks] + [hc.api.BGZF_EOF_BLOCK]
    assert hc.api.BGZF_EOF_BLOCK == M.BGZF_EOF
    whole = b"".join(blocks)
    starts = [sum(len(b) for b in blocks[:k]) for k in range(len(blocks))]
    assert lib.bgzf_split(whole) == (starts, len(whole))
    assert lib.bgzf_split(whole, capacity=2) == (starts[:2], starts[2])
    assert lib.bgzf_split(whole[:-1]) == (starts[:-1], starts[-1])
    assert lib.bgzf_split(b"") == ([], 0)
