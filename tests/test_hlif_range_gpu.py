"""Ranged reads of the high-level managers (hipcomp/hipcompManager.hpp, decompress_range; INTEGRATION.md has the
contract), through tests/hlif_range_driver.cpp, a C++ program written against include/ and linked to libhipcomp.so,
each call a child process under a timeout.  The oracle is the input: a ranged read must return the slice of what was
compressed.  The driver puts guard bytes on both sides of the output (and behind a caller-owned scratch buffer) and
reports whether they survived: asserted for every call, the refused and the failing ones too."""
import os
import struct
import subprocess

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "hlif_ref_tool")
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

NO_COMPUTE_NO_VERIFY, COMPUTE_NO_VERIFY, VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT, COMPUTE_AND_VERIFY = range(5)
INVALID_VALUE, CANNOT_DECOMPRESS, BAD_CHECKSUM, CANNOT_VERIFY = 10, 12, 13, 14
CHAR, SHORT, INT = 0, 2, 4
FORMAT_HEADER = {"lz4": 4, "snappy": 1, "cascaded": 24}
GUARD = 0xA5

# (codec spec, chunk bytes, element bytes): the five of tests/test_hlif_checksums_gpu.py
CODECS = {
    "lz4_char": ("lz4:65536:%d" % CHAR, 65536, 1),
    "lz4_int": ("lz4:16384:%d" % INT, 16384, 4),
    "snappy": ("snappy:32768", 32768, 1),
    "cascaded_rle_delta_bp": ("cascaded:4096:%d:1:1:1" % INT, 4096, 4),
    "cascaded_rle2": ("cascaded:8192:%d:2:0:0" % INT, 8192, 4),
}
# Cascaded with 1- and 2-byte elements: whole elements that leave chunks off the decoder's 4-byte boundary
NARROW = {
    "cascaded_char": ("cascaded:4096:%d:1:1:1" % CHAR, 4096, 1),
    "cascaded_short": ("cascaded:4096:%d:2:1:1" % SHORT, 4096, 2),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("hlif_range") / "hlif_range_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "hlif_range_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _call(args, timeout=300):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def compress(driver, tmp_path, codec, policy, data, name="c.bin"):
    (tmp_path / "in.bin").write_bytes(data)
    out = _call([driver, "compress", codec, policy, tmp_path / "in.bin", tmp_path / name])
    assert out.split() == ["status", "0"], out
    return (tmp_path / name).read_bytes()


def read_range(driver, tmp_path, codec, policy, container, first, num, *extra):
    """(status, the bytes of out[0, num) afterwards, the driver's other words); guards asserted"""
    path = container if isinstance(container, (str, os.PathLike)) else tmp_path / "c_in.bin"
    if path is not container:
        path.write_bytes(container)
    out = _call([driver, "range", codec, policy, path, tmp_path / "r.bin", first, num, *extra])
    words = out.split()
    w = dict(zip(words[0::2], words[1::2]))
    assert w["guards"] == "1", ("bytes outside out[0, num_bytes) were written", codec, first, num, extra, out)
    assert w["scratch_guard"] == "1", ("bytes behind the scratch buffer were written", codec, first, num, extra, out)
    return int(w["status"]), (tmp_path / "r.bin").read_bytes(), w


def parse(c, fmt):
    n, = struct.unpack_from("<Q", c, 24)
    data_off, = struct.unpack_from("<I", c, 56)
    at = (64 + FORMAT_HEADER[fmt] + 7) & ~7
    return {"n": n, "data": data_off, "flags": (c[44], c[45]),
            "offsets": np.frombuffer(c, "<u8", n, at), "sizes": np.frombuffer(c, "<u8", n, at + 8 * n),
            "comp_sums_at": at + 16 * n, "decomp_sums_at": at + 20 * n}


def _data(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "text":
        return datagen.text_like(seed, n)[:n]
    return datagen.random_runs_int32(seed, (n + 3) // 4).tobytes()[:n]


def _flip(c, at):
    b = bytearray(c)
    b[at] ^= 0x5A
    return bytes(b)


def _ranges(c, es, d):
    """(name, first_byte, num_bytes) on a buffer of nine chunks and a short tenth (d bytes), whole elements"""
    assert 9 * c < d < 10 * c
    return [
        ("whole buffer", 0, d),
        ("first byte", 0, es),
        ("last byte", d - es, es),
        ("inside one chunk", 2 * c + 8 * es, 40 * es),
        ("exactly one chunk", 3 * c, c),
        ("two bytes across a chunk boundary", 4 * c - es, 2 * es),
        ("mid-chunk to mid-chunk", c + c // 2, 4 * c - c // 4),
        ("chunk start to mid-chunk", 5 * c, 2 * c + c // 2),
        ("mid-chunk to the end, last chunk short", 7 * c + c // 2, d - (7 * c + c // 2)),
        ("the short last chunk", 9 * c, d - 9 * c),
        ("nothing", c, 0),
        ("nothing at the end", d, 0),
    ]


@pytest.mark.parametrize("name", sorted(CODECS))
def test_ranges_return_the_slice_of_the_input(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 9 * chunk + chunk // 3 // es * es
    data = _data({"lz4_char": "text", "snappy": "text"}.get(name, "runs"), d, 21)
    for policy in (NO_COMPUTE_NO_VERIFY, COMPUTE_AND_VERIFY):
        c = compress(driver, tmp_path, codec, policy, data)
        (tmp_path / "c_keep.bin").write_bytes(c)
        ranges = _ranges(chunk, es, d)
        for what, first, num in ranges if policy == COMPUTE_AND_VERIFY else ranges[:1] + ranges[5:9]:
            st, got, _ = read_range(driver, tmp_path, codec, policy, tmp_path / "c_keep.bin", first, num)
            assert st == 0 and got == data[first:first + num], (name, policy, what, st)
    # the whole buffer is what decompress gives
    st, got, w = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", 0, d, "full")
    assert st == 0 and got == data and w["same_as_decompress"] == "1"
    st, got, w = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", chunk // 2, 3 * chunk, "full")
    assert st == 0 and got == data[chunk // 2: chunk // 2 + 3 * chunk] and w["same_as_decompress"] == "1"


@pytest.mark.parametrize("name", ["lz4_char", "lz4_int", "snappy"])
def test_out_at_odd_addresses(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 9 * chunk + chunk // 3
    data = _data("text" if name != "lz4_int" else "runs", d, 22)
    c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    (tmp_path / "c_keep.bin").write_bytes(c)
    for mis in (1, 3, 7):
        for what, first, num in _ranges(chunk, 1, d)[:10]:
            if what in ("first byte", "exactly one chunk", "the short last chunk"):
                continue
            # (LZ4 with 4-byte elements: the container is bytes all the same -- any first_byte, any length)
            first, num = first + (mis if first + mis + num <= d else 0), num
            st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", first, num, mis)
            assert st == 0 and got == data[first:first + num], (name, mis, what, st)


@pytest.mark.parametrize("name", sorted(NARROW))
def test_cascaded_chunks_off_the_decoders_alignment(driver, tmp_path, name):
    """Whole elements of 1 or 2 bytes: the interior chunks of such a range would land off the batched decoder's
    4-byte contract (hipcomp/cascaded.h) -- they go through scratch slots.  Also: an out that is itself off."""
    codec, chunk, es = NARROW[name]
    d = 9 * chunk + chunk // 3 // es * es
    runs = np.repeat(np.arange(d // es // 5 + 1), 5)[: d // es]
    data = (runs % (251 if es == 1 else 60013)).astype("<u%d" % es).tobytes()
    assert len(data) == d
    c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    (tmp_path / "c_keep.bin").write_bytes(c)
    cases = [(first, num, 0) for _, first, num in _ranges(chunk, es, d)]
    for k in range(es, 4, es):
        cases += [(chunk + k, 3 * chunk, 0), (k, d - k, 0), (2 * chunk - k, 5 * chunk + 2 * k, 0), (0, d, k), (chunk, 4 * chunk, k),
                  (chunk + k, 4 * chunk, 4 - k)]
    for first, num, mis in cases:
        st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", first, num, mis)
        assert st == 0 and got == data[first:first + num], (name, first, num, mis, st)
    if es == 2:   # not whole elements
        for first, num in ((1, 2), (0, 3), (chunk + 1, chunk - 1)):
            st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", first, num)
            assert st == INVALID_VALUE and got == bytes([GUARD]) * num, (first, num, st)


@pytest.mark.parametrize("name", sorted(CODECS))
def test_refused_ranges_and_hostile_headers(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 5 * chunk + 16 * es
    data = _data("runs", d, 23)
    c = compress(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, data)
    (tmp_path / "c_keep.bin").write_bytes(c)
    for first, num in ((d, es), (0, d + es), (d - es, 2 * es), (d + es, 0), (4 * es, 2 ** 64 - 4 * es), (2 ** 64 - es, 2 * es),
                       (es, 2 ** 64 - es)):
        st, got, _ = read_range(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, tmp_path / "c_keep.bin", first, num)
        assert st == INVALID_VALUE and got == b"", (name, first, num, st)
    if es > 1:
        for first, num in ((1, es), (0, es + 1)):
            st, got, _ = read_range(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, tmp_path / "c_keep.bin", first, num)
            assert (st == INVALID_VALUE) == name.startswith("cascaded"), (name, first, num, st)
    # the header changes after configure_decompression: chunk count, chunk size, data offset
    for policy in (NO_COMPUTE_NO_VERIFY, COMPUTE_AND_VERIFY):
        for poke in ("poke=24:1", "poke=49:1", "poke=56:8", "poke=6:7"):
            for first, num in ((0, d), (chunk + 8 * es, 2 * chunk)) if poke == "poke=24:1" else ((chunk + 8 * es, 2 * chunk),):
                st, got, _ = read_range(driver, tmp_path, codec, policy, tmp_path / "c_keep.bin", first, num, poke)
                assert st == CANNOT_DECOMPRESS and got == bytes([GUARD]) * num, (name, policy, poke, first, st)


def test_only_the_chunks_of_the_range_are_read_and_verified(driver, tmp_path):
    codec, chunk, _ = CODECS["lz4_char"]
    d = 9 * chunk + 1000
    data = _data("random", d, 7)       # (random bytes: one literal run per chunk, a flipped byte decodes -- wrongly)
    summed = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    h = parse(summed, "lz4")
    assert h["flags"] == (1, 1)
    first, num = chunk + chunk // 2, 4 * chunk          # edge chunks 1 and 5, interior chunks 2, 3, 4
    want = data[first:first + num]

    def comp_byte(i):
        return h["data"] + int(h["offsets"][i]) + int(h["sizes"][i]) // 2

    verifying = (COMPUTE_AND_VERIFY, VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT)
    for i in (1, 3, 5):                                  # inside the range: edge, interior, edge
        for policy in verifying:
            st, _, _ = read_range(driver, tmp_path, codec, policy, _flip(summed, comp_byte(i)), first, num)
            assert st == BAD_CHECKSUM, (i, policy, st)
        st, got, _ = read_range(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, _flip(summed, comp_byte(i)), first, num)
        assert st == 0 and (got != want or i != 3)   # (the flipped literal of an edge chunk may lie outside the span)
    for i in (0, 6, 7, 9):                               # outside the range
        st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, _flip(summed, comp_byte(i)), first, num)
        assert st == 0 and got == want, (i, st)
    # stored values: of an edge chunk, of an interior chunk, of chunks outside; the full-buffer words are not checked
    for at, bad in ((h["decomp_sums_at"] + 4 * 5, True), (h["decomp_sums_at"] + 4 * 1, True), (h["comp_sums_at"] + 4 * 3, True),
                    (h["comp_sums_at"] + 4 * 1, True), (h["decomp_sums_at"] + 4 * 6, False), (h["comp_sums_at"] + 4 * 0, False),
                    (36, False), (40, False)):
        st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, _flip(summed, at), first, num)
        assert st == (BAD_CHECKSUM if bad else 0) and (bad or got == want), (at, st)
    # a chunk that cannot be decoded at all: CannotDecompress without checksums, BadChecksum with them
    broken = bytearray(summed)
    at0 = h["data"] + int(h["offsets"][5])
    broken[at0:at0 + 8] = bytes(8)                       # (no literals, then a match at offset 0)
    st, got, _ = read_range(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, bytes(broken), first, num)
    assert st == CANNOT_DECOMPRESS and got[:-(chunk // 2)] == want[:-(chunk // 2)] and got[-(chunk // 2):] == bytes([GUARD]) * (chunk // 2)
    st, _, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, bytes(broken), first, num)
    assert st == BAD_CHECKSUM


def test_container_without_checksums(driver, tmp_path):
    for name in ("lz4_int", "snappy", "cascaded_rle_delta_bp"):
        codec, chunk, es = CODECS[name]
        d = 4 * chunk + 8 * es
        data = _data("runs", d, 5)
        c = compress(driver, tmp_path, codec, "old", data)
        first, num = chunk // 2, 3 * chunk
        st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, c, first, num)
        assert st == CANNOT_VERIFY and got == data[first:first + num], name
        for policy in (VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT, COMPUTE_NO_VERIFY, "old"):
            st, got, _ = read_range(driver, tmp_path, codec, policy, c, first, num)
            assert st == 0 and got == data[first:first + num], (name, policy)


def test_more_chunks_than_one_pass_and_caller_owned_scratch(driver, tmp_path):
    """270 000 chunks of 512 bytes are two passes of a read of everything; a range that starts in chunk 3 has its own
    pass boundary 262 144 chunks on.  With the caller's scratch buffer of exactly the required size (guard bytes
    behind it: read_range asserts them)."""
    chunk, n = 512, 270000
    piece = datagen.text_like(23, 1 << 20) + bytes(np.random.default_rng(78).integers(0, 256, 1 << 19, dtype=np.uint8)) + bytes(1 << 18)
    data = (piece * (n * chunk // len(piece) + 1))[: n * chunk - 76]
    codec = "snappy:%d" % chunk
    c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    h = parse(c, "snappy")
    assert h["n"] == n
    (tmp_path / "c_keep.bin").write_bytes(c)
    for first, num, extras in ((3 * chunk + 100, 269000 * chunk, (("scratch",), ("3",))), (262143 * chunk + 511, 2, (("scratch",),)),
                               (5 * chunk, 262145 * chunk, (("scratch",),))):
        for extra in extras:
            st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", first, num, *extra)
            assert st == 0 and got == data[first:first + num], (first, num, extra, st)
    # a flipped stored value in the range's second pass, and one just outside the range
    first, num = 3 * chunk + 100, 269000 * chunk
    st, _, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, _flip(c, h["decomp_sums_at"] + 4 * 268000), first, num, "scratch")
    assert st == BAD_CHECKSUM
    st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, _flip(c, h["decomp_sums_at"] + 4 * 269500), first, num, "scratch")
    assert st == 0 and got == data[first:first + num]


def test_every_chunk_through_a_slot_in_several_passes(driver, tmp_path):
    """Cascaded with 1-byte elements, 40 000 chunks of 512 bytes read from an odd first_byte: every chunk is an edge
    chunk and a pass holds as many as there are scratch slots -- with the manager's own scratch and the caller's."""
    chunk, n = 512, 40000
    codec = "cascaded:%d:%d:1:1:1" % (chunk, CHAR)
    runs = np.repeat(np.arange(n * chunk // 7 + 1), 7)[: n * chunk - 30]
    data = (runs % 253).astype(np.uint8).tobytes()
    c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    (tmp_path / "c_keep.bin").write_bytes(c)
    h = parse(c, "cascaded")
    for first, num in ((chunk + 1, 39000 * chunk), (3, len(data) - 3)):
        for extra in ((), ("scratch",), ("scratch", "2")):
            st, got, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, tmp_path / "c_keep.bin", first, num, *extra)
            assert st == 0 and got == data[first:first + num], (first, num, extra, st)
    st, _, _ = read_range(driver, tmp_path, codec, COMPUTE_AND_VERIFY, _flip(c, h["decomp_sums_at"] + 4 * 38000), chunk + 1, 39000 * chunk)
    assert st == BAD_CHECKSUM


@pytest.mark.skipif(not os.path.exists(REF_TOOL), reason="reference build of the high-level interface not present")
def test_container_written_by_the_reference_manager(driver, tmp_path):
    chunk = 65536
    data = _data("text", 9 * chunk + 777, 11)
    (tmp_path / "in.bin").write_bytes(data)
    r = subprocess.run([REF_TOOL, "compress", "lz4", str(chunk), str(CHAR), str(tmp_path / "in.bin"), str(tmp_path / "ref.bin")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    codec = "lz4:%d:%d" % (chunk, CHAR)
    for first, num, mis in ((0, len(data), 0), (chunk // 2, 6 * chunk, 0), (3 * chunk - 1, 2, 1), (8 * chunk + 5, chunk + 772 - 5, 7)):
        for policy in (NO_COMPUTE_NO_VERIFY, COMPUTE_VERIFY_IF_PRESENT):
            st, got, _ = read_range(driver, tmp_path, codec, policy, tmp_path / "ref.bin", first, num, mis)
            assert st == 0 and got == data[first:first + num], (first, num, mis, policy, st)
