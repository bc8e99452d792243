"""CRC-32 checksums of the high-level managers (hipcomp/hipcompManager.hpp ChecksumPolicy; INTEGRATION.md
defines them), through tests/hlif_checksum_driver.cpp, a C++ program written against include/ and linked to
libhipcomp.so.  zlib.crc32 is the oracle: per chunk of the container (its offsets and sizes) and of the input,
the index-ordered concatenation of the compressed chunks, the whole input; silent corruption caught; containers
without checksums; the reference's manager in both directions; more chunks than one compress pass holds; a
caller-owned scratch buffer."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "hlif_ref_tool")
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

NO_COMPUTE_NO_VERIFY, COMPUTE_NO_VERIFY, VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT, COMPUTE_AND_VERIFY = range(5)
BAD_CHECKSUM, CANNOT_VERIFY = 13, 14
CHAR, INT = 0, 4
FORMAT_HEADER = {"lz4": 4, "snappy": 1, "cascaded": 24}

# (codec spec, chunk bytes, element bytes)
CODECS = {
    "lz4_char": ("lz4:65536:%d" % CHAR, 65536, 1),
    "lz4_int": ("lz4:16384:%d" % INT, 16384, 4),
    "snappy": ("snappy:32768", 32768, 1),
    "cascaded_rle_delta_bp": ("cascaded:4096:%d:1:1:1" % INT, 4096, 4),
    "cascaded_rle2": ("cascaded:8192:%d:2:0:0" % INT, 8192, 4),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("hlif_crc") / "hlif_checksum_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "hlif_checksum_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _call(args, timeout=300):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout


def compress(driver, tmp_path, codec, policy, data, scratch=False):
    (tmp_path / "in.bin").write_bytes(data)
    out = _call([driver, "compress", codec, policy, tmp_path / "in.bin", tmp_path / "c.bin"] + (["scratch"] if scratch else []))
    words = out.split()
    assert words[0] == "status" and words[1] == "0", out
    return (tmp_path / "c.bin").read_bytes()


def decompress(driver, tmp_path, policy, container, scratch=False):
    (tmp_path / "c_in.bin").write_bytes(container)
    out = _call([driver, "decompress", policy, tmp_path / "c_in.bin", tmp_path / "d.bin"] + (["scratch"] if scratch else []))
    words = out.split()
    assert words[0] == "status", out
    return int(words[1]), (tmp_path / "d.bin").read_bytes()


def parse(c, fmt):
    comp_size, decomp_size, n = struct.unpack_from("<QQQ", c, 8)
    full_comp, full_decomp = struct.unpack_from("<II", c, 36)
    chunk, = struct.unpack_from("<Q", c, 48)
    data_off, = struct.unpack_from("<I", c, 56)
    at = (64 + FORMAT_HEADER[fmt] + 7) & ~7
    return {
        "n": n, "decomp_size": decomp_size, "chunk": chunk, "data": data_off,
        "full_comp": full_comp, "full_decomp": full_decomp, "flags": (c[44], c[45]),
        "offsets": np.frombuffer(c, "<u8", n, at), "sizes": np.frombuffer(c, "<u8", n, at + 8 * n),
        "comp_sums": np.frombuffer(c, "<u4", n, at + 16 * n), "decomp_sums": np.frombuffer(c, "<u4", n, at + 20 * n),
        "comp_sums_at": at + 16 * n, "decomp_sums_at": at + 20 * n,
    }


def check_checksums(c, fmt, data, chunk):
    h = parse(c, fmt)
    n = h["n"]
    assert n == (len(data) + chunk - 1) // chunk and h["decomp_size"] == len(data)
    assert h["flags"] == (1, 1)
    full = 0
    for i in range(n):
        o, s = int(h["offsets"][i]), int(h["sizes"][i])
        piece = c[h["data"] + o: h["data"] + o + s]
        assert len(piece) == s
        assert int(h["comp_sums"][i]) == zlib.crc32(piece), i
        assert int(h["decomp_sums"][i]) == zlib.crc32(data[i * chunk: (i + 1) * chunk]), i
        full = zlib.crc32(piece, full)
    assert h["full_comp"] == full
    assert h["full_decomp"] == zlib.crc32(data)
    return h


def _data(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "text":
        return datagen.text_like(seed, n)[:n]
    return datagen.random_runs_int32(seed, (n + 3) // 4).tobytes()[:n]


@pytest.mark.parametrize("name", sorted(CODECS))
def test_compute_and_verify_round_trip_matches_zlib(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    fmt = codec.split(":")[0]
    sizes = [0, 1, chunk - 1, chunk, chunk + 1, 37 * chunk + chunk // 3]
    if fmt == "cascaded":
        sizes = [0, es, chunk - es, chunk, chunk + es, 37 * chunk + chunk // 3 // es * es]
    for k, n in enumerate(sizes):
        kind = ("random", "text", "runs")[k % 3]
        data = _data(kind, n, k + 10)
        c = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
        check_checksums(c, fmt, data, chunk)
        st, back = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, c)
        assert st == 0 and back == data, (name, n, kind, st)


@pytest.mark.parametrize("name", sorted(CODECS))
def test_default_policy_writes_the_reference_header(driver, tmp_path, name):
    codec, chunk, es = CODECS[name]
    fmt = codec.split(":")[0]
    data = _data("text", 3 * chunk + 4 * es, 3)
    for policy in ("old", NO_COMPUTE_NO_VERIFY):
        h = parse(compress(driver, tmp_path, codec, policy, data), fmt)
        assert (h["full_comp"], h["full_decomp"], h["flags"]) == (0, 0, (0, 0)), policy
        # (what the checksum arrays hold is not written by anyone: not looked at)


def _flip(c, at):
    b = bytearray(c)
    b[at] ^= 0x5A
    return bytes(b)


def test_silent_corruption_is_caught(driver, tmp_path):
    codec, chunk, _ = CODECS["lz4_char"]
    data = _data("random", 5 * chunk + 1000, 7)
    plain = compress(driver, tmp_path, codec, NO_COMPUTE_NO_VERIFY, data)
    summed = compress(driver, tmp_path, codec, COMPUTE_AND_VERIFY, data)
    for c, fmt_policy in ((plain, None), (summed, None)):
        h = parse(c, "lz4")
        i = int(np.argmax(h["offsets"]))  # a chunk of random bytes: one long literal run
        at = h["data"] + int(h["offsets"][i]) + int(h["sizes"][i]) // 2
        bad = _flip(c, at)
        if c is plain:
            # today's behaviour without checksums: the decoder succeeds and the bytes are wrong
            st, back = decompress(driver, tmp_path, NO_COMPUTE_NO_VERIFY, bad)
            assert st == 0 and back != data and len(back) == len(data)
        else:
            for policy in (COMPUTE_AND_VERIFY, VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT):
                st, _ = decompress(driver, tmp_path, policy, bad)
                assert st == BAD_CHECKSUM, policy
            st, _ = decompress(driver, tmp_path, NO_COMPUTE_NO_VERIFY, bad)
            assert st == 0
    h = parse(summed, "lz4")
    for at in (h["comp_sums_at"] + 4 * 2, h["decomp_sums_at"] + 4 * 4, 36, 40):
        st, _ = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, _flip(summed, at))
        assert st == BAD_CHECKSUM, at
        st, back = decompress(driver, tmp_path, NO_COMPUTE_NO_VERIFY, _flip(summed, at))
        assert st == 0 and back == data, at


def test_container_without_checksums(driver, tmp_path):
    for name in ("lz4_int", "snappy", "cascaded_rle_delta_bp"):
        codec, chunk, es = CODECS[name]
        data = _data("runs", 4 * chunk + 8 * es, 5)
        c = compress(driver, tmp_path, codec, "old", data)
        st, back = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, c)
        assert st == CANNOT_VERIFY and back == data, name
        for policy in (VERIFY_IF_PRESENT, COMPUTE_VERIFY_IF_PRESENT, "old"):
            st, back = decompress(driver, tmp_path, policy, c)
            assert st == 0 and back == data, (name, policy)
        # ComputeAndNoVerify writes checksums but never checks them
        st, back = decompress(driver, tmp_path, COMPUTE_NO_VERIFY, c)
        assert st == 0 and back == data


@pytest.mark.skipif(not os.path.exists(REF_TOOL), reason="reference build of the high-level interface not present")
def test_interop_with_the_reference_manager(driver, tmp_path):
    chunk = 65536
    data = _data("text", 9 * chunk + 777, 11)
    c = compress(driver, tmp_path, "lz4:%d:%d" % (chunk, CHAR), COMPUTE_AND_VERIFY, data)
    (tmp_path / "ours.bin").write_bytes(c)
    r = subprocess.run([REF_TOOL, "decompress", str(tmp_path / "ours.bin"), str(tmp_path / "ours.out")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "ours.out").read_bytes() == data
    (tmp_path / "in.bin").write_bytes(data)
    r = subprocess.run([REF_TOOL, "compress", "lz4", str(chunk), str(CHAR), str(tmp_path / "in.bin"), str(tmp_path / "ref.bin")],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    ref = (tmp_path / "ref.bin").read_bytes()
    assert parse(ref, "lz4")["flags"] == (0, 0)
    st, back = decompress(driver, tmp_path, COMPUTE_VERIFY_IF_PRESENT, ref)
    assert st == 0 and back == data


def test_more_chunks_than_one_pass(driver, tmp_path):
    chunk, n = 256, 300000
    rng = np.random.default_rng(3)
    data = rng.integers(0, 16, chunk * n - 100, dtype=np.uint8).tobytes()
    c = compress(driver, tmp_path, "lz4:%d:%d" % (chunk, CHAR), COMPUTE_AND_VERIFY, data)
    h = check_checksums(c, "lz4", data, chunk)
    assert h["n"] == n
    st, back = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, c)
    assert st == 0 and back == data
    # a flipped stored value in the second decompress pass
    st, _ = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, _flip(c, h["decomp_sums_at"] + 4 * 280000))
    assert st == BAD_CHECKSUM


def test_caller_owned_scratch(driver, tmp_path):
    codec, chunk, _ = CODECS["lz4_char"]
    data = _data("text", 20 * chunk + 5, 13)
    out = _call([driver, "compress", codec, NO_COMPUTE_NO_VERIFY, "/dev/null", tmp_path / "x.bin"])
    plain_scratch = int(out.split()[3])
    (tmp_path / "in.bin").write_bytes(data)
    out = _call([driver, "compress", codec, COMPUTE_AND_VERIFY, tmp_path / "in.bin", tmp_path / "c.bin", "scratch"])
    assert out.split()[1] == "0" and int(out.split()[3]) >= plain_scratch
    c = (tmp_path / "c.bin").read_bytes()
    check_checksums(c, "lz4", data, chunk)
    st, back = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, c, scratch=True)
    assert st == 0 and back == data
    st, _ = decompress(driver, tmp_path, COMPUTE_AND_VERIFY, _flip(c, 40), scratch=True)
    assert st == BAD_CHECKSUM
