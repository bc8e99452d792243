"""Seekable LZ4 frames on the device (hipcomp/lz4.hpp: compress_frame with LZ4FrameIndex::Leading, the indexed read
inside configure_frame_decompression / decompress_frame; INTEGRATION.md, "Seekable LZ4 frames", has the contract),
through tests/lz4_frame_index_driver.cpp, a C++ program written against include/ and linked to libhipcomp.so.  The
driver works through a list of cases per process, each process under a timeout; it puts guard bytes on both sides of
every output and behind a caller-owned scratch buffer.

Writing: every indexed frame must equal, byte for byte, the index tests/lz4_frame_indexgen.py writes for the frame
the unindexed call wrote in the same process, followed by that frame; liblz4's LZ4F_decompress must give the input
back.  Reading: every planned input of lz4_frame_indexgen gives the status, size and bytes of the same input without
its index frames, and those the generator planned from liblz4's verdict; a device counter of the blocks the chain's
walk stepped over says whether the index served (0) or the call fell back (all of them).  Every planned input is read
twice: configured just before (configure_frame_decompression then tells decompress_frame whether to try the index at
all) and with another buffer configured in between, so that decompress_frame launches its indexed passes on every
forged index and these refuse on the device -- in the hop, in the listing of a pass, after the decode, and in a later
pass than the first, behind blocks the indexed passes have already written.  Ranged reads
(decompress_frame_range): byte ranges of a frame of seven 4 KiB blocks and of two frames, with and without block
checksums, against slices of the content; damage inside and outside the range; every input whose index does not
apply."""
import os
import struct
import subprocess

import numpy as np
import pytest

import datagen
import lz4_frame_indexgen as I
import lz4_framegen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
CHAR, INT = 0, 4
POLICIES = range(5)
COMPUTES = (1, 3, 4)
CHUNK = 4096


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("lz4_frame_index") / "lz4_frame_index_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "lz4_frame_index_driver.cpp"), "-L", LIB, "-lhipcomp",
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
def _mixed(chunk, n):
    """chunks that alternate text / random / zeros: compressed and stored blocks interleave"""
    parts = [(datagen.text_like(k, chunk)[:chunk], np.random.default_rng(k).integers(0, 256, chunk, dtype=np.uint8).tobytes(),
              bytes(chunk))[k % 3] for k in range(-(-n // chunk))]
    return b"".join(parts)[:n]


def _write_specs():
    """name -> (chunk, type, policy, what the input is, scratch, offset)"""
    specs = {}
    for t in (CHAR, INT):
        for policy in POLICIES:
            for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1):
                specs["c%d_t%d_p%d_n%d" % (CHUNK, t, policy, n)] = (CHUNK, t, policy, ("slice", n), "own", (n + policy) % 8)
            specs["c%d_t%d_p%d_mixed" % (CHUNK, t, policy)] = (CHUNK, t, policy, ("mixed", CHUNK), "scratch" if policy in (0, 4) else "own", policy)
    specs["c1024_p3_mixed"] = (1024, CHAR, 3, ("mixed", 1024), "own", 3)
    specs["c1024_many_passes"] = (1024, CHAR, 0, ("many",), "scratch", 5)
    return specs


def _write_input(what, cache={}):
    if what[0] == "slice":
        if "slice" not in cache:
            cache["slice"] = _mixed(CHUNK, 4 * CHUNK)
        return cache["slice"][CHUNK + 100:CHUNK + 100 + what[1]]
    if what[0] == "mixed":
        return _mixed(what[1], 11 * what[1] + 123)
    # more chunks than one pass of the write path holds (its slots are a chunk's bound each, inside the scratch space
    # of a manager of 1024-byte chunks: by the sizes' arithmetic about 20 000 of these 40 960 chunks on an MI355X);
    # every seventh chunk does not compress
    text = datagen.text_like(3, 1 << 20)[:1 << 20]
    big = bytearray(text * 40)
    view = np.frombuffer(big, dtype=np.uint8).reshape(-1, 1024)
    view[::7] = np.random.default_rng(1).integers(0, 256, view[::7].shape, dtype=np.uint8)
    return bytes(big) + b"tail" * 30


@pytest.fixture(scope="module")
def written(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frame_index_write")
    cases = {name: spec[:3] + (_write_input(spec[3]),) + spec[4:] for name, spec in _write_specs().items()}
    lines = []
    for name, (chunk, t, policy, data, scratch, off) in cases.items():
        (tmp / (name + ".in")).write_bytes(data)
        lines.append((chunk, t, policy, tmp / (name + ".in"), tmp / (name + ".lz4"), tmp / (name + ".plain"), scratch, off))
    words = _run(driver, "write", tmp, lines, timeout=600)
    return tmp, cases, dict(zip(cases, words))


@pytest.mark.parametrize("name", list(_write_specs()))
def test_written_indexed_frame(written, name):
    tmp, cases, words = written
    chunk, t, policy, data, _, _ = cases[name]
    w = words[name]
    sums = policy in COMPUTES
    n = -(-len(data) // chunk)
    assert w["status"] == 0 and w["guards"] == 1 and w["scratch_guard"] == 1, w
    assert w["plain_bound"] == 15 + n * (chunk + 4 + 4 * sums) + 4
    assert w["bound"] == w["plain_bound"] + 44 + 4 * n
    plain = (tmp / (name + ".plain")).read_bytes()
    frame = (tmp / (name + ".lz4")).read_bytes()
    assert w["plain_bytes"] == len(plain), "compress_frame(..., None) did not write what compress_frame writes"
    assert w["frame_bytes"] == len(frame) == len(plain) + 44 + 4 * n <= w["bound"]
    size_words = I.size_words(plain)
    assert len(size_words) == n
    want = I.index_frame(size_words, chunk, len(data), sums) + plain
    assert frame[:44 + 4 * n] == want[:44 + 4 * n], "the index is not the generator's"
    assert frame == want, "the bytes behind the index are not the unindexed frame"
    assert I.input_is_indexed(frame) == ("ok", 1, n, len(data))
    if "mixed" in name or name == "c1024_many_passes":
        assert {bool(x & I.STORED) for x in size_words} == {False, True}, "stored and compressed blocks were to interleave"
    L = G.load_lz4f()
    if L is None:
        print("liblz4.so.1 absent: the frame was not given to LZ4F_decompress")
    else:
        ok, out = G.lz4f_decompress(L, frame)
        assert ok and out == data
    assert w["roundtrip"] == 1, "decompress_frame did not give the input back"
    assert w["walked"] == 0, "decompress_frame followed the chain of a frame this manager indexed"


# ---- the indexed read ------------------------------------------------------------------------------------------
def _many_blocks():
    """More data blocks than one pass of the read path lists (at most 262 144): one-byte stored blocks behind their
    index, read by a manager of one-byte chunks -- the smallest there is -- in a caller-owned scratch buffer."""
    content = bytes(i % 251 for i in range(262200))
    frame = G.frame([(content[i:i + 1], True) for i in range(len(content))], 4, content_size=len(content))
    return I.IndexPlan("many_blocks", I.index_frame([I.STORED | 1] * len(content), 1, len(content), False) + frame, "ok",
                       "more blocks than a pass lists", content=content, blocks=len(content))


def _read_cases():
    """name -> (plan name, with its index frames, policy, chunk, scratch, offset in, offset out)"""
    cases = {}
    for p in I.plans():
        for policy in POLICIES:
            for indexed in (True, False):
                cases["%s/%s/p%d" % (p.name, "indexed" if indexed else "bare", policy)] = (
                    p.name, indexed, policy, CHUNK if policy % 2 else 1024, "scratch" if policy == 2 else "own",
                    (policy * 3 + len(p.data)) % 8, (policy + len(p.data)) % 5)
    for indexed in (True, False):
        cases["many_blocks/%s/p3" % ("indexed" if indexed else "bare")] = ("many_blocks", indexed, 3, 1, "scratch", 1, 1)
    return cases


@pytest.fixture(scope="module")
def read_back(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frame_index_read")
    plans = {p.name: p for p in I.plans() + [_many_blocks()]}
    cases = _read_cases()
    lines, files = [], {}
    for k, (name, (plan, indexed, policy, chunk, scratch, off_in, off_out)) in enumerate(cases.items()):
        if (plan, indexed) not in files:
            files[plan, indexed] = tmp / ("%d.lz4" % len(files))
            files[plan, indexed].write_bytes(plans[plan].data if indexed else plans[plan].bare)
        lines.append((chunk, policy, files[plan, indexed], tmp / ("%d.out" % k), scratch, off_in, off_out))
    words = _run(driver, "read", tmp, lines, timeout=600)
    return plans, cases, {name: (w, tmp / ("%d.out" % k)) for k, (name, w) in enumerate(zip(cases, words))}


@pytest.mark.parametrize("name", [n for n in _read_cases() if "/indexed/" in n])
def test_indexed_read(read_back, name):
    plans, cases, results = read_back
    plan, _, policy, _, _, _, _ = cases[name]
    p = plans[plan]
    w, out = results[name]
    b, bare_out = results[name.replace("/indexed/", "/bare/")]
    for x in (w, b):
        assert x["guards"] == 1, ("bytes outside decomp_buffer[0, decomp_data_size) were written", x)
        assert x["scratch_guard"] == 1, ("bytes behind the scratch buffer were written", x)
    # what the same input gives without its index frames
    for key in ("configured", "status", "size", "blocks"):
        assert w[key] == b[key], (key, w, b)
    got = out.read_bytes()
    if w["status"] in (G.SUCCESS, G.CANNOT_VERIFY):
        assert got == bare_out.read_bytes()
    # what the generator planned from liblz4's verdict
    assert w["status"] == p.status(policy), (w, p.why)
    if p.sound:
        assert w["size"] == len(p.content) and w["blocks"] == p.blocks and got == p.content
    # whether the index served
    assert b["walked"] == b["blocks"], b
    assert w["walked"] == (0 if p.applies else p.blocks if p.sound else w["walked"]), (w, p.reason, p.why)
    if not p.sound:
        assert w["walked"] == b["walked"]


# ---- the indexed read without the host's word on the index ------------------------------------------------------
LATE = 262190   # (a block of the second pass: a pass lists at most 262 144)


def _late_refusal():
    """_many_blocks, but index word LATE says "compressed, 1 byte" where the frame says "stored, 1 byte": the fields,
    the hash, the sum of the lengths and the EndMark behind them hold, the first pass lists, decodes and writes its
    blocks, and the listing of the second pass finds another word in the frame than in the index."""
    good = _many_blocks()
    words = [I.STORED | 1] * good.blocks
    words[LATE] = 1
    data = I.index_frame(words, 1, good.blocks, False) + good.bare
    reason = I.input_is_indexed(data)[0]
    assert reason != "ok"
    return I.IndexPlan("late_refusal", data, reason, "the stored bit of index word %d cleared" % LATE, content=good.content,
                       blocks=good.blocks)


def _displaced_cases():
    """name -> (the case of _read_cases() with the same input and manager, plan name): every indexed read of
    _read_cases() again, and the refusal in a later pass"""
    cases = {name: (name, spec[0]) for name, spec in _read_cases().items() if "/indexed/" in name}
    cases["late_refusal/indexed/p3"] = ("many_blocks/indexed/p3", "late_refusal")
    return cases


@pytest.fixture(scope="module")
def displaced(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frame_index_displaced")
    plans = {p.name: p for p in I.plans() + [_many_blocks(), _late_refusal()]}
    specs = _read_cases()
    lines, files = [], {}
    for k, (name, (like, plan)) in enumerate(_displaced_cases().items()):
        _, _, policy, chunk, scratch, off_in, off_out = specs[like]
        if plan not in files:
            files[plan] = tmp / ("%d.lz4" % len(files))
            files[plan].write_bytes(plans[plan].data)
        lines.append((chunk, policy, files[plan], tmp / ("%d.out" % k), scratch, off_in, off_out))
    words = _run(driver, "read_displaced", tmp, lines, timeout=600)
    return plans, {name: (w, tmp / ("%d.out" % k)) for k, (name, w) in enumerate(zip(_displaced_cases(), words))}


@pytest.mark.parametrize("name", list(_displaced_cases()))
def test_indexed_read_decided_on_the_device(read_back, displaced, name):
    """The expectations of test_indexed_read, on reads that launch the indexed passes whatever the index is worth."""
    _, cases, bare_results = read_back
    plans, results = displaced
    like, plan = _displaced_cases()[name]
    policy = cases[like][2]
    p = plans[plan]
    w, out = results[name]
    b, bare_out = bare_results[like.replace("/indexed/", "/bare/")]   # (late_refusal without its index is many_blocks')
    assert w["guards"] == 1, ("bytes outside decomp_buffer[0, decomp_data_size) were written", w)
    assert w["scratch_guard"] == 1, ("bytes behind the scratch buffer were written", w)
    for key in ("configured", "status", "size", "blocks"):
        assert w[key] == b[key], (key, w, b)
    got = out.read_bytes()
    if w["status"] in (G.SUCCESS, G.CANNOT_VERIFY):
        assert got == bare_out.read_bytes()
    assert w["status"] == p.status(policy), (w, p.why)
    if p.sound:
        assert w["size"] == len(p.content) and w["blocks"] == p.blocks and got == p.content
        assert w["walked"] == (0 if p.applies else p.blocks), (w, p.reason, p.why)
    else:
        assert w["walked"] == b["walked"], (w, b)


# ---- ranged reads ----------------------------------------------------------------------------------------------
NOT_SUPPORTED, INVALID_VALUE = 11, 10
RB = 4096


def _range_inputs():
    """name -> (input, content, block checksums): seven 4 KiB blocks (compressed, stored, compressed, ..., a short
    last one), and two such frames with a foreign skippable frame between them"""
    out = {}
    for sums in (False, True):
        frame, content = I.written_form(RB, "cscscsc", 1000, sums, 5)
        second, second_content = I.written_form(RB, "scc", 33, sums, 50)
        tag = "_sums" if sums else ""
        out["seven" + tag] = (I.indexed(frame, RB, sums), content, sums)
        out["two_frames" + tag] = (I.indexed(frame, RB, sums) + G.skippable(b"foreign", 9) + I.indexed(second, RB, sums),
                                   content + second_content, sums)
    return out


def _ranges(total, first_frame):
    r = {"empty": (1234, 0), "one_byte": (5000, 1), "inside_one_block": (4200, 300), "across_one_boundary": (4000, 200),
         "across_stored_and_compressed": (8000, 500), "from_0": (0, 6000), "to_the_last_byte": (20000, total - 20000),
         "whole": (0, total), "one_byte_beyond": (total - 10, 11)}
    if total > first_frame:
        r["across_the_frames"] = (first_frame - 100, 300)
        r["inside_the_second_frame"] = (first_frame + 4096 + 7, 4096)
    return r


def _range_cases():
    """name -> (input name or plan name, policy, scratch, first, count, what is done to the input)"""
    cases = {}
    seven = 6 * RB + 1000
    for name in ("seven", "seven_sums", "two_frames", "two_frames_sums"):
        total = seven if name.startswith("seven") else seven + 2 * RB + 33
        for rname, (first, count) in _ranges(total, seven).items():
            for policy in (0, 3):
                cases["%s/%s/p%d" % (name, rname, policy)] = (name, policy, "scratch" if policy == 3 and rname == "whole" else "own",
                                                             first, count, "")
    cases["seven/whole/p4"] = ("seven", 4, "own", 0, seven, "")
    cases["seven_sums/whole/p4"] = ("seven_sums", 4, "own", 0, seven, "")
    # a flipped byte in the middle of the stored block 1 (inside the range read), and of the compressed block 4
    for policy in (0, 3):
        cases["seven_sums/flip_touched_stored/p%d" % policy] = ("seven_sums", policy, "own", RB + RB // 2 - 8, 20, "flip1")
        cases["seven_sums/flip_touched_compressed/p%d" % policy] = ("seven_sums", policy, "own", 4 * RB + 10, 20, "flip4")
        cases["seven_sums/flip_untouched/p%d" % policy] = ("seven_sums", policy, "own", 4 * RB + 10, 20, "flip1")
    for p in I.plans():
        if p.reason != "ok" and len(p.content) > 0:
            cases["plan_%s/p3" % p.name] = ("plan:" + p.name, 3, "own", 0, min(10, len(p.content)), "")
    cases["plan_short_interior_blocks/first_block"] = ("plan:short_interior_blocks", 0, "own", 5, 10, "")
    cases["plan_short_interior_blocks/short_block"] = ("plan:short_interior_blocks", 0, "own", 1000, 10, "")
    return cases


def _flip(data, block):
    """one bit in the middle of data block `block` of the (single) indexed frame"""
    reason, _, h = I.index_applies(data, 0)
    assert reason == "ok"
    pos = I.index_bytes(h["blocks"]) + 15
    for w in h["words"][:block]:
        pos += 4 + (w & ~I.STORED) + (4 if h["flags"] & 1 else 0)
    at = pos + 4 + (h["words"][block] & ~I.STORED) // 2
    return data[:at] + bytes([data[at] ^ 0x20]) + data[at + 1:]


@pytest.fixture(scope="module")
def ranged(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frame_index_range")
    inputs = _range_inputs()
    plans = {p.name: p for p in I.plans()}
    cases = _range_cases()
    lines, files, content = [], {}, {}
    for k, (name, (src, policy, scratch, first, count, damage)) in enumerate(cases.items()):
        if (src, damage) not in files:
            data, want = (plans[src[5:]].data, plans[src[5:]].content) if src.startswith("plan:") else inputs[src][:2]
            if damage:
                data = _flip(data, int(damage[4:]))
            files[src, damage] = tmp / ("%d.lz4" % len(files))
            files[src, damage].write_bytes(data)
            content[src] = want
        lines.append((RB, policy, files[src, damage], tmp / ("%d.out" % k), scratch, (k * 3) % 8, (k * 5) % 7, first, count))
    words = _run(driver, "range", tmp, lines, timeout=600)
    return cases, content, plans, {name: (w, tmp / ("%d.out" % k)) for k, (name, w) in enumerate(zip(cases, words))}


@pytest.mark.parametrize("name", list(_range_cases()))
def test_ranged_read(ranged, name):
    cases, content, plans, results = ranged
    src, policy, _, first, count, damage = cases[name]
    w, out = results[name]
    want = content[src][first:first + count]
    got = out.read_bytes()
    assert w["guards"] == 1, ("bytes outside out[0, num_bytes) were written", w)
    assert w["scratch_guard"] == 1, ("bytes behind the scratch buffer were written", w)
    assert w["walked"] == 0, "a ranged read followed the chain"
    if src.startswith("plan:") and plans[src[5:]].reason != "ok":
        p = plans[src[5:]]
        assert w["untouched"] == 1, w
        assert w["status"] == (NOT_SUPPORTED if p.sound else G.CANNOT_DECOMPRESS), (w, p.why)
        assert w["configured"] == (0 if p.sound else G.CANNOT_DECOMPRESS)
        return
    if name.endswith("one_byte_beyond/p0") or name.endswith("one_byte_beyond/p3"):
        assert w["status"] == INVALID_VALUE and w["untouched"] == 1, w
        return
    if name == "plan_short_interior_blocks/short_block":   # the block holds 500 bytes where the index promises 1000
        assert w["status"] == G.CANNOT_DECOMPRESS, w
        return
    sums = src.endswith("_sums")
    touched = {"flip1": 1, "flip4": 4}.get(damage, -1) in range(first // RB, (first + count - 1) // RB + 1) if count else False
    if touched and sums and policy == 3:
        assert w["status"] == G.BAD_CHECKSUM, w
        return
    if touched and damage == "flip4":
        return   # (a damaged LZ4 stream read without its checksum: any status, any bytes, inside the guards)
    assert w["status"] == (G.CANNOT_VERIFY if policy == 4 and not sums else G.SUCCESS), w
    if touched:
        assert got != want and len(got) == len(want)   # (a damaged stored block read without its checksum)
    else:
        assert got == want
