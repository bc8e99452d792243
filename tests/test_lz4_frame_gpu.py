"""LZ4 frames on the device (hipcomp/lz4.hpp: compress_frame / decompress_frame of the LZ4 manager; INTEGRATION.md,
"LZ4 frames", has the contract), through tests/lz4_frame_driver.cpp, a C++ program written against include/ and
linked to libhipcomp.so.  The driver works through a list of cases per process, each process under a timeout; it
puts guard bytes on both sides of every output and behind a caller-owned scratch buffer.

Writing: every frame must equal, byte for byte, the frame tests/lz4_framegen.py assembles from the streams the
batched API writes for the same chunks; it must decode to the input with the Python parser and the oracle's LZ4
decoder, be accepted by liblz4's LZ4F_decompress, come back through decompress_frame, and be read by the host helper
hipcompLZ4FrameToBlocks.  Reading: every fixture of tests/golden/lz4_frame/ (liblz4's own frames) and every planned
frame of lz4_framegen, legal and hostile, gives the planned status, size and bytes under each ChecksumPolicy."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import datagen
import lz4_framegen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lz4_frame")
CHAR, INT = 0, 4
POLICIES = range(5)
COMPUTES = (1, 3, 4)
INVALID_VALUE = 10


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("lz4_frame") / "lz4_frame_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "lz4_frame_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, cmd, tmp, lines, timeout=300):
    (tmp / (cmd + ".list")).write_text("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    r = subprocess.run([driver, cmd, str(tmp / (cmd + ".list"))], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in r.stdout.splitlines())]
    assert len(out) == len(lines), r.stdout[-500:]
    return out


# ---- writing ---------------------------------------------------------------------------------------------------
def _mixed(n):
    """chunks of 65536 that alternate text / random / zeros: compressed and stored blocks interleave"""
    parts, k = [], 0
    while sum(map(len, parts)) < n:
        parts.append((datagen.text_like(k, 65536)[:65536], np.random.default_rng(k).integers(0, 256, 65536, dtype=np.uint8).tobytes(),
                      bytes(65536))[k % 3])
        k += 1
    return b"".join(parts)[:n]


def _write_specs():
    """name -> (chunk, type, policy, what the input is, scratch, offset); _write_input makes the bytes"""
    specs = {}
    for t in (CHAR, INT):
        for policy in POLICIES:
            for n in (0, 1, 65535, 65536, 65537):
                specs["c65536_t%d_p%d_n%d" % (t, policy, n)] = (65536, t, policy, ("slice", n), "own", (n + policy) % 8)
            specs["c65536_t%d_p%d_mixed" % (t, policy)] = (65536, t, policy, ("mixed",), "scratch" if policy in (0, 4) else "own", policy)
    for chunk, policy in ((4096, 4), (262144, 0), (4 << 20, 0)):
        specs["c%d_p%d" % (chunk, policy)] = (chunk, CHAR, policy, ("two_and_a_half", chunk), "own", 3)
    specs["c1024_many_passes"] = (1024, CHAR, 0, ("many",), "scratch", 5)
    return specs


def _write_input(what, cache={}):
    if not cache:
        cache["mixed"] = _mixed(5 * 65536 + 123)
        cache["text"] = datagen.text_like(3, 1 << 20)[:1 << 20]
        cache["noise"] = np.random.default_rng(9).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    mixed, text, noise = cache["mixed"], cache["text"], cache["noise"]
    if what[0] == "slice":
        return mixed[70000:70000 + what[1]]
    if what[0] == "mixed":
        return mixed
    if what[0] == "two_and_a_half":   # text, random, text
        chunk = what[1]
        return (text * 5)[:chunk] + (noise * 5)[:chunk] + (text * 5)[:chunk // 2]
    # more blocks than one pass of the write path holds (its slots are a chunk's bound each, inside the scratch space
    # of a manager of 1024-byte chunks: by the sizes' arithmetic about 20 000 of these 40 960 chunks on an MI355X);
    # every seventh chunk does not compress
    big = bytearray(text * 40)
    view = np.frombuffer(big, dtype=np.uint8).reshape(-1, 1024)
    view[::7] = np.random.default_rng(1).integers(0, 256, view[::7].shape, dtype=np.uint8)
    return bytes(big) + b"tail" * 30


@pytest.fixture(scope="module")
def written(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frame_write")
    cases = {name: spec[:3] + (_write_input(spec[3]),) + spec[4:] for name, spec in _write_specs().items()}
    lines = []
    for name, (chunk, t, policy, data, scratch, off) in cases.items():
        (tmp / (name + ".in")).write_bytes(data)
        lines.append((chunk, t, policy, tmp / (name + ".in"), tmp / (name + ".lz4"), tmp / (name + ".streams"), scratch, off))
    # also: a manager of 16 MiB chunks, which no block maximum of the format holds
    (tmp / "too_large.in").write_bytes(b"x" * 1000)
    lines.append((16 << 20, CHAR, 1, tmp / "too_large.in", tmp / "too_large.lz4", tmp / "too_large.streams", "own", 1))
    words = _run(driver, "write", tmp, lines, timeout=600)
    return tmp, cases, dict(zip(list(cases) + ["too_large"], words))


def _streams(path):
    blob, out, at = path.read_bytes(), [], 0
    while at < len(blob):
        n, = struct.unpack_from("<Q", blob, at)
        out.append(blob[at + 8:at + 8 + n])
        at += 8 + n
    return out


@pytest.mark.parametrize("name", list(_write_specs()))
def test_written_frame(written, oracle, name):
    tmp, cases, words = written
    chunk, t, policy, data, _, _ = cases[name]
    w = words[name]
    sums = policy in COMPUTES
    n = (len(data) + chunk - 1) // chunk
    assert w["status"] == 0 and w["guards"] == 1 and w["scratch_guard"] == 1, w
    assert w["bound"] == 15 + n * (chunk + 4 + 4 * sums) + 4
    frame = (tmp / (name + ".lz4")).read_bytes()
    assert w["frame_bytes"] == len(frame) <= w["bound"]
    chunks = [data[i:i + chunk] for i in range(0, len(data), chunk)]
    streams = _streams(tmp / (name + ".streams"))
    assert len(streams) == n
    want = G.written_frame(chunks, streams, chunk, sums)
    assert len(frame) == len(want) and frame == want, "the frame is not the one the batched API's streams make"
    if name.endswith("mixed") or name == "c1024_many_passes":
        kinds = {len(s) >= len(c) for c, s in zip(chunks, streams)}
        assert kinds == {False, True}, "stored and compressed blocks were to interleave"

    def block(payload, cap):
        st, out = oracle.lz4_decompress(payload, cap)
        assert st == 0
        return out
    assert G.decode(frame, block) == data
    L = G.load_lz4f()
    if L is None:
        print("liblz4.so.1 absent: the frame was not given to LZ4F_decompress")
    else:
        ok, out = G.lz4f_decompress(L, frame)
        assert ok and out == data
    assert w["roundtrip"] == 1, "decompress_frame did not give the input back"
    assert w["interop_blocks"] == n, "hipcompLZ4FrameToBlocks does not read the frame"


def test_chunks_larger_than_any_block_maximum_are_refused(written):
    tmp, _, words = written
    w = words["too_large"]
    assert w["status"] == INVALID_VALUE and w["frame_bytes"] == 0 and w["bound"] == 0 and w["guards"] == 1, w
    assert not (tmp / "too_large.lz4").exists() or (tmp / "too_large.lz4").read_bytes() == b""


# ---- reading ---------------------------------------------------------------------------------------------------
def _many_blocks():
    """More data blocks than one pass of the read path lists (262 144): an independent-block frame of one-byte stored
    blocks, then a linked-block frame that begins in the first pass and ends in the second, with its size and a
    content checksum; its blocks reach back into the blocks before them."""
    first = bytes(i % 251 for i in range(262100))
    a = G.frame([(first[i:i + 1], True) for i in range(len(first))], 4, content_size=len(first))
    content, blocks = bytearray(b"0123456789abcdef"), [(b"0123456789abcdef", True)]
    for k in range(199):
        b = G.sequence(bytes([65 + k % 26]), 9 + k % 7, 6) + G.sequence(b"<%03d>" % k)
        content += G.decode_block(b, bytes(content))
        blocks.append((b, False))
    return G.Plan("many_blocks", a + G.frame(blocks, 4, True, False, True, len(content), bytes(content)),
                  content=first + bytes(content), blocks=len(first) + 200, bare=True)


def _read_cases():
    """name -> (plan, policy, scratch, offset in, offset out)"""
    cases = {}
    for p in G.all_plans():
        for policy in POLICIES:
            cases["%s/p%d" % (p.name, policy)] = (p, policy, "own", (policy * 3 + len(p.data)) % 8, (policy + len(p.data)) % 5)
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    for name, m in manifest.items():
        if name == "liblz4":
            continue
        frame = open(os.path.join(GOLDEN, name + ".lz4"), "rb").read()
        assert hashlib.sha256(frame).hexdigest() == m["frame_sha256"], name
        p = G.Plan("golden_" + name, frame, content=m, blocks=m["blocks"], bare=m["bare"])
        for policy in POLICIES:
            cases["golden_%s/p%d" % (name, policy)] = (p, policy, "scratch" if policy == 0 else "own", 0, 0)
        for off in (1, 3, 7):   # frames and decomp_buffer at odd addresses
            cases["golden_%s/odd%d" % (name, off)] = (p, 3, "own", off, 8 - off)
    cases["many_blocks/p3"] = (G.Plan("many_blocks", b""), 3, "own", 1, 1)   # (made by the fixture: _many_blocks)
    return cases


@pytest.fixture(scope="module")
def read_back(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frame_read")
    cases = _read_cases()
    cases["many_blocks/p3"] = (_many_blocks(),) + cases["many_blocks/p3"][1:]
    lines, files = [], {}
    for k, (name, (p, policy, scratch, off_in, off_out)) in enumerate(cases.items()):
        if p.name not in files:
            files[p.name] = tmp / ("%d.lz4" % len(files))
            files[p.name].write_bytes(p.data)
        lines.append((policy, files[p.name], tmp / ("%d.out" % k), scratch, off_in, off_out))
    words = _run(driver, "read", tmp, lines, timeout=600)
    return tmp, cases, {name: (w, tmp / ("%d.out" % k)) for k, (name, w) in enumerate(zip(cases, words))}


@pytest.mark.parametrize("name", list(_read_cases()))
def test_read_frame(read_back, name):
    _, cases, results = read_back
    p, policy, _, _, _ = cases[name]
    w, out = results[name]
    assert w["guards"] == 1, ("bytes outside decomp_buffer[0, decomp_data_size) were written", w)
    assert w["scratch_guard"] == 1, ("bytes behind the scratch buffer were written", w)
    want = p.status(policy)
    assert w["status"] == want, (w, p.reason, p.flipped)
    if want in (G.SUCCESS, G.CANNOT_VERIFY) or (p.flipped and p.reason == "ok"):
        got = out.read_bytes()
        assert w["blocks"] == p.blocks
        if isinstance(p.content, dict):   # a fixture: the manifest's word on its content
            assert w["size"] == p.content["content_bytes"] == len(got)
            assert hashlib.sha256(got).hexdigest() == p.content["content_sha256"]
        else:
            assert w["size"] == len(p.content)
            # (a content checksum that does not fit says nothing about the bytes; a block's says they are damaged)
            if want != G.BAD_CHECKSUM or p.flipped == "content":
                assert got == p.content
    if w["configured"] != 0:
        assert w["configured"] == w["status"] == want and w["size"] == 0 and w["blocks"] == 0, w
