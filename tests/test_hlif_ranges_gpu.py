"""Reads of many ranges in one call (hipcomp/hipcompManager.hpp, decompress_ranges; INTEGRATION.md has the contract),
through tests/hlif_ranges_driver.cpp, a C++ program written against include/ and linked to libhipcomp.so, several
cases per child process, each process under a timeout.  The oracle is the input: every range must equal the slice
of what was compressed (and what decompress_range of the same build writes for it), the offsets the restated sums.
The driver puts guard bytes on both sides of the output and of the offsets array (and behind a caller-owned scratch
buffer) and reports whether they survived: asserted for every call, the refused and the failing ones too."""
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
M64 = (1 << 64) - 1

# (codec spec, chunk bytes, element bytes): the five of tests/test_hlif_range_gpu.py and its two narrow Cascaded ones
CODECS = {
    "lz4_char": ("lz4:65536:%d" % CHAR, 65536, 1),
    "lz4_int": ("lz4:16384:%d" % INT, 16384, 4),
    "snappy": ("snappy:32768", 32768, 1),
    "cascaded_rle_delta_bp": ("cascaded:4096:%d:1:1:1" % INT, 4096, 4),
    "cascaded_rle2": ("cascaded:8192:%d:2:0:0" % INT, 8192, 4),
    "cascaded_char": ("cascaded:4096:%d:1:1:1" % CHAR, 4096, 1),
    "cascaded_short": ("cascaded:4096:%d:2:1:1" % SHORT, 4096, 2),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("hlif_ranges") / "hlif_ranges_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "hlif_ranges_driver.cpp"), "-L", LIB, "-lhipcomp",
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


class Read:
    """one case of a driver call: the container (bytes or a path), the ranges [(first, num)], the driver's options"""

    def __init__(self, container, ranges, *extra):
        self.container, self.ranges, self.extra = container, [(int(f), int(n)) for f, n in ranges], extra


def read_many(driver, tmp_path, codec, policy, cases):
    """-> per case (status, out bytes, offsets or None, the driver's words); guards asserted.  One child process."""
    args = [driver, "ranges", codec, policy]
    for k, case in enumerate(cases):
        path = case.container
        if not isinstance(path, (str, os.PathLike)):
            path = tmp_path / ("c_in_%d.bin" % k)
            path.write_bytes(case.container)
        rpath = tmp_path / ("ranges_%d.bin" % k)
        rpath.write_bytes(np.array([[f & M64, n & M64] for f, n in case.ranges], dtype="<u8").reshape(-1, 2).tobytes())
        args += (["--"] if k else []) + [path, rpath, tmp_path / ("out_%d.bin" % k), *case.extra]
    lines = _call(args).splitlines()
    assert len(lines) == len(cases), lines
    got = []
    for k, (case, line) in enumerate(zip(cases, lines)):
        w = dict(zip(line.split()[0::2], line.split()[1::2]))
        assert w["guards"] == "1", ("bytes outside out[0, total) were written", codec, case.extra, line)
        assert w["offs_guards"] == "1", ("words outside the offsets array were written", codec, case.extra, line)
        assert w["scratch_guard"] == "1", ("bytes behind the scratch buffer were written", codec, case.extra, line)
        offs = np.frombuffer((tmp_path / ("out_%d.bin.offs" % k)).read_bytes(), "<u8")
        got.append((int(w["status"]), (tmp_path / ("out_%d.bin" % k)).read_bytes(), None if "nooffs" in case.extra else offs, w))
    return got


def read_one(driver, tmp_path, codec, policy, container, ranges, *extra):
    return read_many(driver, tmp_path, codec, policy, [Read(container, ranges, *extra)])[0]


def expected(data, ranges):
    """(the bytes of every range back to back, the offsets) restated"""
    first = np.array([f for f, _ in ranges], dtype=np.int64)
    num = np.array([n for _, n in ranges], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(num)])
    idx = np.repeat(first - offs[:-1], num) + np.arange(offs[-1])
    return np.frombuffer(data, np.uint8)[idx].tobytes(), offs.astype("<u8")


def check_exact(data, ranges, got, which=None):
    """every range (or those of `which`) holds exactly its slice"""
    want, offs = expected(data, ranges)
    for r, (f, n) in enumerate(ranges):
        if which is None or r in which:
            a = int(offs[r])
            assert got[a:a + n] == data[f:f + n], ("range", r, f, n)
    return want, offs


def touched(ranges, chunk):
    s = set()
    for f, n in ranges:
        if n:
            s.update(range(f // chunk, (f + n - 1) // chunk + 1))
    return len(s)


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


def _codec_data(name, d, es, seed):
    if name in ("cascaded_char", "cascaded_short"):
        runs = np.repeat(np.arange(d // es // 5 + 1), 5)[: d // es]
        return (runs % (251 if es == 1 else 60013)).astype("<u%d" % es).tobytes()
    return _data({"lz4_char": "text", "snappy": "text"}.get(name, "runs"), d, seed)


def _flip(c, at):
    b = bytearray(c)
    b[at] ^= 0x5A
    return bytes(b)


def _ranges(c, es, d):
    """the ranges of one call on a buffer of nine chunks and a short tenth (d bytes), whole elements"""
    assert 9 * c < d < 10 * c and c >= 600 * es
    r = [(c, 0),                                         # empty
         (0, es), (d - es, es),                          # one element
         (2 * c + 8 * es, 40 * es),                      # inside a chunk
         (3 * c, c),                                     # exactly a chunk
         (4 * c - es, 2 * es),                           # two elements across a boundary
         (c + c // 2, 4 * c - c // 4),                   # mid-chunk to mid-chunk over five chunks
         (0, d),                                         # the whole buffer
         (9 * c, d - 9 * c),                             # the short last chunk
         (5 * c + es, 3 * es), (5 * c + es, 3 * es),     # the same range twice
         (6 * c, c), (6 * c + c // 2, c),                # two overlapping ranges
         (8 * c, 3 * es), (7 * c, 5 * es), (c, 7 * es),  # in descending order
         (d, 0)]                                         # empty, at the end
    r += [(2 * c + 3 * es * k, es) for k in range(200)]  # 200 one-element ranges inside one chunk: more than a wave
    r += [(3 * c + 40 * es * k, es * k) for k in range(1, 34)]   # odd lengths: later ranges land at every residue mod 16
    return r


@pytest.mark.parametrize("name", sorted(CODECS))
def test_ranges_return_the_slices_of_the_input(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 9 * chunk + chunk // 3 // es * es
    data = _codec_data(name, d, es, 31)
    ranges = _ranges(chunk, es, d)
    want, offs = expected(data, ranges)
    if es == 1:
        assert {int(o) % 16 for o in offs} == set(range(16))
    for policy in (NO_COMPUTE_NO_VERIFY, COMPUTE_AND_VERIFY):
        c = compress(driver, tmp_path, codec, policy, data)
        (tmp_path / "c_keep.bin").write_bytes(c)
        keep = tmp_path / "c_keep.bin"
        cases = [Read(keep, ranges, "cmp"), Read(keep, ranges, 1), Read(keep, ranges, 7, "nooffs"), Read(keep, ranges, 13),
                 Read(keep, ranges, "nooffs")]
        for case, (st, got, got_offs, w) in zip(cases, read_many(driver, tmp_path, codec, policy, cases)):
            assert st == 0, (name, policy, case.extra, st)
            check_exact(data, ranges, got)
            assert got == want
            assert got_offs is None or np.array_equal(got_offs, offs), (name, policy, case.extra)
            assert "cmp" not in case.extra or w["same_as_range"] == "1"
            # each chunk once
            assert int(w["touched"]) == touched(ranges, chunk) == 10 and int(w["ranges"]) == len(ranges)
            assert int(w["total"]) == len(want) and int(w["passes"]) == 1


@pytest.mark.parametrize("name", ["lz4_char", "snappy", "cascaded_rle_delta_bp", "cascaded_short"])
def test_each_chunk_once_for_five_thousand_ranges(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 9 * chunk + chunk // 3 // es * es
    data = _codec_data(name, d, es, 32)
    rng = np.random.default_rng(5000)
    c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    # over the ten chunks, and over three of them
    for ranges in ([(int(e) * es, es) for e in rng.integers(0, d // es, 5000)],
                   [(int(e) * es, es) for e in rng.integers(0, chunk // es, 5000) + rng.choice([1, 4, 9], 5000) * (chunk // es)
                    if int(e) * es < d]):
        st, got, offs, w = read_one(driver, tmp_path, codec, COMPUTE_AND_VERIFY, c, ranges)
        want, want_offs = expected(data, ranges)
        assert st == 0 and got == want and np.array_equal(offs, want_offs)
        assert int(w["touched"]) == touched(ranges, chunk) and int(w["ranges"]) == len(ranges) and int(w["total"]) == len(ranges) * es
    assert touched(ranges, chunk) == 3


@pytest.mark.parametrize("scratch", [(), ("scratch",)], ids=["own_scratch", "callers_scratch"])
def test_several_passes(driver, tmp_path, scratch):
    """512-byte chunks, 2 * get_ranges_pass_chunks() + 3 of them: one byte of every chunk and two bytes across every
    chunk boundary -- among them every boundary between the last chunk of a pass and the first of the next,
    wherever the call's tables put it."""
    chunk = 512
    codec = "snappy:%d" % chunk
    P = int(_call([driver, "pass_chunks", codec, COMPUTE_AND_VERIFY, *scratch]).split()[1])
    assert 2 <= P <= 262144
    n = 2 * P + 3
    piece = datagen.text_like(23, 1 << 20) + bytes(np.random.default_rng(78).integers(0, 256, 1 << 19, dtype=np.uint8)) + bytes(1 << 18)
    data = (piece * (n * chunk // len(piece) + 1))[: n * chunk - 76]
    c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    assert parse(c, "snappy")["n"] == n
    k = np.arange(n, dtype=np.int64)
    first = np.concatenate([k * chunk + (k * 37) % 400, k[1:] * chunk - 1])
    num = np.concatenate([np.ones(n, np.int64), np.full(n - 1, 2, np.int64)])
    order = np.random.default_rng(3).permutation(len(first))
    ranges = list(zip(first[order].tolist(), num[order].tolist()))
    st, got, offs, w = read_one(driver, tmp_path, codec, COMPUTE_AND_VERIFY, c, ranges, *scratch)
    want, want_offs = expected(data, ranges)
    assert st == 0 and int(w["passes"]) >= 2 and int(w["touched"]) == n, w
    assert got == want and np.array_equal(offs, want_offs)


@pytest.mark.parametrize("name", sorted(CODECS))
def test_refusals(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 5 * chunk + 16 * es
    data = _codec_data(name, d, es, 33)
    c = compress(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, data)
    (tmp_path / "c_keep.bin").write_bytes(c)
    keep = tmp_path / "c_keep.bin"
    good = [(0, 8 * es), (chunk - es, 2 * es), (3 * chunk, chunk), (d - es, es)]
    total = sum(n for _, n in good)
    bad = [(d, es), (d - es, 2 * es), (0, d + es), (d + es, 0), (4 * es, 2 ** 64 - 4 * es), (2 ** 64 - es, 2 * es), (es, 2 ** 64 - es)]
    cases = [Read(keep, good[:2] + [b] + good[2:]) for b in bad]
    cases += [Read(keep, good, "out_bytes=%d" % (total - 1)), Read(keep, good + [(0, d)] * 3, "out_bytes=%d" % (total + 3 * d - 1)),
              Read(keep, good, "out_bytes=0", "nooffs")]
    if name.startswith("cascaded") and es > 1:
        cases += [Read(keep, good + [(1, es)]), Read(keep, [(0, es + 1)] + good), Read(keep, good + [(chunk + 1, chunk - 1)])]
    for case, (st, got, offs, w) in zip(cases, read_many(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, cases)):
        assert st == INVALID_VALUE, (name, case.ranges, case.extra, st)
        assert got == bytes([GUARD]) * len(got), (name, case.ranges)
        assert offs is None or offs.tobytes() == bytes([GUARD]) * (8 * len(offs)), (name, case.ranges)
        assert int(w["touched"]) == 0 and int(w["passes"]) == 0
    # the same good ranges are read where nothing is wrong, with room to the byte; no ranges at all is success
    (st, got, offs, _), (st0, got0, _, _) = read_many(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY,
                                                    [Read(keep, good, "out_bytes=%d" % total), Read(keep, [])])
    assert st == 0 and got == expected(data, good)[0] and int(offs[-1]) == total
    assert st0 == 0 and got0 == b""
    if not name.startswith("cascaded") and es > 1:      # LZ4 with 4-byte elements: the container is bytes all the same
        st, got, _, _ = read_one(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, keep, good + [(1, es + 1)])
        assert st == 0 and got == expected(data, good + [(1, es + 1)])[0]


@pytest.mark.parametrize("name", ["lz4_char", "snappy", "cascaded_rle_delta_bp"])
def test_hostile_headers(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    d = 5 * chunk + 16 * es
    data = _codec_data(name, d, es, 34)
    ranges = [(0, d), (chunk + 8 * es, 2 * chunk), (es, es)]
    for policy in (NO_COMPUTE_NO_VERIFY, COMPUTE_AND_VERIFY):
        c = compress(driver, tmp_path, codec, policy, data)
        (tmp_path / "c_keep.bin").write_bytes(c)
        # the header changes after configure_decompression: chunk count, chunk size, data offset, format
        cases = [Read(tmp_path / "c_keep.bin", ranges, poke) for poke in ("poke=24:1", "poke=49:1", "poke=56:8", "poke=6:7")]
        for case, (st, got, offs, w) in zip(cases, read_many(driver, tmp_path, codec, policy, cases)):
            assert st == CANNOT_DECOMPRESS and got == bytes([GUARD]) * len(got), (name, policy, case.extra, st)


def test_damage_in_touched_and_untouched_chunks(driver, tmp_path):
    codec, chunk, _ = CODECS["lz4_char"]
    d = 9 * chunk + 1000
    data = _data("random", d, 7)       # (random bytes: one literal run per chunk, a flipped byte decodes -- wrongly)
    summed = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    h = parse(summed, "lz4")
    assert h["flags"] == (1, 1)
    ranges = [(chunk + chunk // 2, 100), (3 * chunk - 50, 100), (5 * chunk + 5, chunk), (8 * chunk, 10), (chunk + 7, 33)]
    uses = {0: {1}, 1: {2, 3}, 2: {5, 6}, 3: {8}, 4: {1}}
    assert touched(ranges, chunk) == 6

    def comp_byte(i):
        return h["data"] + int(h["offsets"][i]) + int(h["sizes"][i]) // 2

    def avoiding(i):
        return {r for r, cs in uses.items() if i not in cs}

    verifying = (COMPUTE_AND_VERIFY, VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT)
    for policy in verifying + (NO_COMPUTE_NO_VERIFY,):
        touched_ones = (1, 3, 6)
        cases = [Read(_flip(summed, comp_byte(i)), ranges) for i in touched_ones]
        for i, (st, got, _, w) in zip(touched_ones, read_many(driver, tmp_path, codec, policy, cases)):
            assert st == (BAD_CHECKSUM if policy in verifying else 0), (i, policy, st)
            check_exact(data, ranges, got, avoiding(i))
            assert int(w["touched"]) == 6
    # damage in a chunk no range touches goes unnoticed; the full-buffer words are not checked
    places = [comp_byte(i) for i in (0, 4, 7, 9)] + [h["decomp_sums_at"] + 4 * 4, h["comp_sums_at"] + 4 * 0, 36, 40]
    for at, (st, got, _, _) in zip(places, read_many(driver, tmp_path, codec, COMPUTE_AND_VERIFY, [Read(_flip(summed, at), ranges) for at in places])):
        assert st == 0 and got == expected(data, ranges)[0], (at, st)
    # a stored checksum of a touched chunk, either side
    places = [(h["decomp_sums_at"] + 4 * 5, 5), (h["comp_sums_at"] + 4 * 3, 3), (h["decomp_sums_at"] + 4 * 1, 1)]
    for (at, i), (st, got, _, _) in zip(places, read_many(driver, tmp_path, codec, COMPUTE_AND_VERIFY,
                                                         [Read(_flip(summed, at), ranges) for at, _ in places])):
        assert st == BAD_CHECKSUM, (at, st)
        check_exact(data, ranges, got, avoiding(i))
    # a chunk that cannot be decoded at all: CannotDecompress without checksums, BadChecksum with them
    broken = bytearray(summed)
    at0 = h["data"] + int(h["offsets"][5])
    broken[at0:at0 + 8] = bytes(8)                       # (no literals, then a match at offset 0)
    for policy, status in ((NO_COMPUTE_NO_VERIFY, CANNOT_DECOMPRESS), (COMPUTE_AND_VERIFY, BAD_CHECKSUM)):
        st, got, offs, _ = read_one(driver, tmp_path, codec, policy, bytes(broken), ranges)
        assert st == status
        _, want_offs = check_exact(data, ranges, got, avoiding(5))
        assert np.array_equal(offs, want_offs)
        # the failed chunk gave nothing: its share of range 2 is as it was, the share of chunk 6 is there
        a = int(want_offs[2])
        assert got[a:a + chunk - 5] == bytes([GUARD]) * (chunk - 5) and got[a + chunk - 5:a + chunk] == data[6 * chunk:6 * chunk + 5]


def test_container_without_checksums(driver, tmp_path):
    codec, chunk, es = CODECS["snappy"]
    d = 4 * chunk + 8
    data = _data("text", d, 5)
    c = compress(driver, tmp_path, codec, "old", data)
    ranges = [(chunk // 2, 3 * chunk), (5, 1)]
    st, got, _, _ = read_one(driver, tmp_path, codec, COMPUTE_AND_VERIFY, c, ranges)
    assert st == CANNOT_VERIFY and got == expected(data, ranges)[0]
    for policy in (VERIFY_IF_PRESENT, COMPUTE_NO_VERIFY, "old"):
        st, got, _, _ = read_one(driver, tmp_path, codec, policy, c, ranges)
        assert st == 0 and got == expected(data, ranges)[0], policy


@pytest.mark.skipif(not os.path.exists(REF_TOOL), reason="reference build of the high-level interface not present")
def test_container_written_by_the_reference_manager(driver, tmp_path):
    chunk = 65536
    data = _data("text", 9 * chunk + 777, 11)
    (tmp_path / "in.bin").write_bytes(data)
    r = subprocess.run([REF_TOOL, "compress", "lz4", str(chunk), str(CHAR), str(tmp_path / "in.bin"), str(tmp_path / "ref.bin")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    codec = "lz4:%d:%d" % (chunk, CHAR)
    ranges = _ranges(chunk, 1, len(data))
    for policy in (NO_COMPUTE_NO_VERIFY, COMPUTE_VERIFY_IF_PRESENT):
        st, got, offs, w = read_one(driver, tmp_path, codec, policy, tmp_path / "ref.bin", ranges, 3)
        want, want_offs = expected(data, ranges)
        assert st == 0 and got == want and np.array_equal(offs, want_offs) and int(w["touched"]) == 10
