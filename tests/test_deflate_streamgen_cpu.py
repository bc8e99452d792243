"""tests/deflate_streamgen.py proven on the CPU: zlib decodes every legal planned stream to exactly the planned
bytes and refuses every illegal one (an exception, or no `eof`); the plans cover every form their lists name.
Also here: the C ABI of the Deflate companion library (exports, header as C99, null arguments)."""
import ctypes
import os
import subprocess
import zlib

import pytest

import deflate_streamgen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib", "libhipcomp_deflate.so")
DECLARED = {"hipcompBatchedDeflateDecompressGetTempSize", "hipcompBatchedDeflateGetDecompressSizeAsync",
            "hipcompBatchedDeflateDecompressAsync"}


def test_zlib_decodes_every_legal_plan_to_the_planned_bytes():
    plans = G.legal_plans()
    names = [n for n, _, _ in plans]
    assert len(set(names)) == len(names)
    for name, stream, want in plans:
        d = zlib.decompressobj(-15)
        got = d.decompress(stream)
        assert d.eof and got == want, name
    for size in (0, 1, 65535):
        for off in range(8):
            assert f"stored{size}_at_bit{off}" in names
    for need in ("empty_fixed", "all_length_symbols_fixed", "all_length_symbols_dynamic", "all_distance_symbols_fixed",
                 "all_distance_symbols_dynamic", "overlapping_matches", "match_across_blocks", "zero_run_across_the_two_sets",
                 "repeat_across_the_two_sets", "hclen_5", "hclen_19", "dynamic_without_distance_code", "single_distance_code",
                 "max_alphabets_15_bit_codes", "ends_on_the_last_bit", "trailing_bytes", "blocks_200"):
        assert need in names, need
    by = {n: s for n, s, _ in plans}
    d = zlib.decompressobj(-15)
    d.decompress(by["trailing_bytes"])
    assert d.eof and len(d.unused_data) > 0
    d = zlib.decompressobj(-15)
    d.decompress(by["ends_on_the_last_bit"])
    assert d.eof and d.unused_data == b""
    assert not G.zlib_verdict(by["ends_on_the_last_bit"][:-1])[0]


def test_the_planned_symbols_are_the_ones_written():
    """258 through code 285 and through 284 + 31; every length and distance symbol; the runs 16 / 17 / 18 across
    the border of the two sets."""
    toks = [t for t in (("m", 258, 1, 285), ("m", 258, 2, 284))]
    syms = G.token_symbols(toks)
    assert syms[0][:3] == (285, 0, 0) and syms[1][:3] == (284, 31, 5)
    assert {G.dist_symbol(G.DIST_BASE[s] + x) for s in range(30) for x in (0, (1 << G.DIST_EXTRA[s]) - 1)} == set(range(30))
    assert {G.length_symbol(G.LENGTH_BASE[i]) for i in range(29)} == set(range(257, 286))
    lit = [8] * 254 + [0, 0] + [9] * 4 + [0] * 20
    cl = G.code_length_symbols(lit + [0] * 6 + [1, 1])
    at, crossing = 0, False
    for s, x in cl:
        n = 1 if s < 16 else (3 + x if s in (16, 17) else 11 + x)
        crossing = crossing or (s >= 16 and at < len(lit) < at + n)
        at += n
    assert at == len(lit) + 8 and crossing


def test_zlib_refuses_every_illegal_plan():
    plans = G.illegal_plans()
    names = [n for n, _ in plans]
    assert len(set(names)) == len(names)
    for name, stream in plans:
        d = zlib.decompressobj(-15)
        try:
            d.decompress(stream)
        except zlib.error:
            continue
        assert not d.eof, name
    for need in ("btype_3", "len_nlen_mismatch", "distance_before_start_fixed", "fixed_litlen_symbol_286",
                 "fixed_litlen_symbol_287", "fixed_distance_symbol_30", "fixed_distance_symbol_31", "missing_final_block",
                 "truncated_at_0", "hclen_4_all_lengths_zero"):
        assert need in names, need
    assert sum(n.startswith("truncated_at_") for n in names) >= 100


# ------------------------------------------------------------------------------------------------- the C ABI
def test_deflate_library_exports_exactly_the_declared_functions():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names == DECLARED, names ^ DECLARED


def test_deflate_header_is_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipcomp/deflate.h"\n'
                   "int main(void) { size_t t = 1; return (int)hipcompBatchedDeflateDecompressGetTempSize(1, 1, &t) + (int)t; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                        "-I", "/opt/rocm/include", "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "include", "hipcomp", "deflate.h")).read()
    includes = [l for l in text.splitlines() if l.startswith("#include")]
    assert includes == ['#include "hipcomp.h"']
    assert "ISIZE" in text and "gzip" in text and "zlib" in text


def test_null_arguments_return_invalid_value(hc):
    lib = hc.api.deflate_library()
    assert hc.api.deflate_library() is lib
    t = ctypes.c_size_t(7)
    assert lib.hipcompBatchedDeflateDecompressGetTempSize(10, 65536, None) == 10
    assert lib.hipcompBatchedDeflateDecompressGetTempSize(10, 65536, ctypes.byref(t)) == 0 and t.value == 0
    p = 0x1000   # never dereferenced: a null argument is refused before anything is launched
    assert lib.hipcompBatchedDeflateGetDecompressSizeAsync(None, p, p, 1, None) == 10
    assert lib.hipcompBatchedDeflateGetDecompressSizeAsync(p, None, p, 1, None) == 10
    assert lib.hipcompBatchedDeflateGetDecompressSizeAsync(p, p, None, 1, None) == 10
    for k in (0, 1, 2, 7):
        args = [p, p, p, p, 1, None, 0, p, p, None]
        args[k] = None
        assert lib.hipcompBatchedDeflateDecompressAsync(*args) == 10, k
    # batch_size == 0: success, nothing launched (no device is needed for it)
    assert lib.hipcompBatchedDeflateDecompressAsync(p, p, p, None, 0, None, 0, p, None, None) == 0
    assert lib.hipcompBatchedDeflateGetDecompressSizeAsync(p, p, p, 0, None) == 0
