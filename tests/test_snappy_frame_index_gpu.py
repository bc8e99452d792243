"""Seekable Snappy framed streams on the device (hipcomp/snappy.hpp: compress_frame with SnappyFrameIndex::Leading, the
indexed read inside configure_frame_decompression / decompress_frame, decompress_frame_range; INTEGRATION.md,
"Seekable Snappy framed streams", has the contract), through tests/snappy_frame_index_driver.cpp, a C++ program written
against include/ and linked to libhipcomp.so.  The driver works through a list of cases per process, each process
under a timeout; it puts guard bytes on both sides of every output and behind a caller-owned scratch buffer.

Writing: every indexed stream must equal, byte for byte, the identifier, the index tests/snappy_frame_indexgen.py
writes for the stream the unindexed call wrote in the same process, and that stream's data chunks; the Python parser
and pyarrow's Snappy codec must give the input back.  Reading: every planned input of snappy_frame_indexgen gives the
status, size and bytes snappy_framegen's parser and decoder plan for the same bytes -- they step over the index like
over any skippable chunk; a device counter of the data chunks the chain's walk stepped over says whether the index
served (0) or the call fell back (all of them).  Every planned input is read twice: configured just before
(configure_frame_decompression then tells decompress_frame whether to try the index at all) and with another buffer
configured in between, so that decompress_frame launches its indexed passes on every forged index and these refuse on
the device -- in the hop, in the listing of a pass, after the decode, and in a later pass than the first, behind
chunks the indexed passes have already written.  Ranged reads (decompress_frame_range): byte ranges of a unit of seven
4 KiB chunks and of two units against slices of the content; damage inside and outside the range; every input whose
index does not apply."""
import os
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import datagen
import snappy_frame_indexgen as I
import snappy_framegen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
POLICIES = range(5)
VERIFIES = (2, 3, 4)
CHUNK = 4096
NOT_SUPPORTED, INVALID_VALUE = 11, 10


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("snappy_frame_index") / "snappy_frame_index_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "snappy_frame_index_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


def _run(driver, cmd, tmp, lines, timeout=300):
    (tmp / (cmd + ".list")).write_text("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    r = subprocess.run([driver, cmd, str(tmp / (cmd + ".list"))], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    out = _words(r.stdout)
    assert len(out) == len(lines), r.stdout[-500:]
    return out


def _pyarrow_block(payload: bytes) -> bytes:
    pre = G.read_varint(payload, 0, len(payload))
    assert pre is not None
    return pa.Codec("snappy").decompress(payload, pre[0]).to_pybytes()


# ---- writing ---------------------------------------------------------------------------------------------------
def _mixed(chunk, n):
    """chunks that alternate text / random / zeros: compressed and stored chunks interleave"""
    parts = [(datagen.text_like(k, chunk)[:chunk], np.random.default_rng(k).integers(0, 256, chunk, dtype=np.uint8).tobytes(),
              bytes(chunk))[k % 3] for k in range(-(-n // chunk))]
    return b"".join(parts)[:n]


def _write_specs():
    """name -> (chunk, policy, what the input is, scratch, offset)"""
    specs = {}
    for policy in POLICIES:
        for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1):
            specs["c%d_p%d_n%d" % (CHUNK, policy, n)] = (CHUNK, policy, ("slice", n), "own", 1 + 2 * ((n + policy) % 4))
        specs["c%d_p%d_mixed" % (CHUNK, policy)] = (CHUNK, policy, ("mixed", CHUNK, 11), "scratch" if policy in (0, 4) else "own",
                                                    2 * policy + 1)
    specs["c1024_p3_mixed"] = (1024, 3, ("mixed", 1024, 11), "own", 3)
    specs["c65536_p4_three_chunks"] = (65536, 4, ("mixed", 65536, 2), "own", 7)
    specs["c1024_many_passes"] = (1024, 0, ("many",), "scratch", 5)
    return specs


def _write_input(what, cache={}):
    if what[0] == "slice":
        if "slice" not in cache:
            cache["slice"] = _mixed(CHUNK, 4 * CHUNK)
        return cache["slice"][CHUNK + 100:CHUNK + 100 + what[1]]
    if what[0] == "mixed":
        return _mixed(what[1], what[2] * what[1] + 123)
    # 40 960 chunks of 1024 bytes, every seventh incompressible: more than one pass of the write path, whose slots are
    # a chunk's bound each inside the scratch space of a manager of 1024-byte chunks (test_snappy_frame_gpu.py has the
    # arithmetic), so the words of several passes land in one index
    text = datagen.text_like(3, 1 << 20)[:1 << 20]
    big = bytearray(text * 40)
    view = np.frombuffer(big, dtype=np.uint8).reshape(-1, 1024)
    view[::7] = np.random.default_rng(1).integers(0, 256, view[::7].shape, dtype=np.uint8)
    return bytes(big)


@pytest.fixture(scope="module")
def written(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("snappy_frame_index_write")
    cases = {name: spec[:2] + (_write_input(spec[2]),) + spec[3:] for name, spec in _write_specs().items()}
    lines = []
    for name, (chunk, policy, data, scratch, off) in cases.items():
        (tmp / (name + ".in")).write_bytes(data)
        lines.append((chunk, policy, tmp / (name + ".in"), tmp / (name + ".sz"), tmp / (name + ".plain"), scratch, off))
    words = _run(driver, "write", tmp, lines, timeout=600)
    return tmp, cases, dict(zip(cases, words))


@pytest.mark.parametrize("name", list(_write_specs()))
def test_written_indexed_stream(written, name):
    tmp, cases, words = written
    chunk, policy, data, _, _ = cases[name]
    w = words[name]
    n = -(-len(data) // chunk)
    assert w["status"] == 0 and w["guards"] == 1 and w["scratch_guard"] == 1, w
    assert w["plain_bound"] == 10 + n * (chunk + 8)
    assert w["bound"] == w["plain_bound"] + 40 + 4 * n
    plain = (tmp / (name + ".plain")).read_bytes()
    frame = (tmp / (name + ".sz")).read_bytes()
    assert w["plain_bytes"] == len(plain), "compress_frame(..., None) did not write what compress_frame writes"
    assert w["frame_bytes"] == len(frame) == len(plain) + 40 + 4 * n <= w["bound"]
    assert plain[:10] == G.IDENTIFIER
    data_words = I.data_words(plain)
    assert len(data_words) == n
    want = G.IDENTIFIER + I.index_chunk(data_words, chunk, len(data)) + plain[10:]
    assert frame[:50 + 4 * n] == want[:50 + 4 * n], "the index is not the generator's"
    assert frame == want, "the bytes behind the index are not the unindexed stream's data chunks"
    assert I.input_is_indexed(frame) == ("ok", 1, n, len(data))
    if "mixed" in name or name == "c1024_many_passes":
        assert {x & 0xFF for x in data_words} == {0, 1}, "stored and compressed chunks were to interleave"
    if n == 0:
        assert len(frame) == 50
    assert G.decode(frame, True, _pyarrow_block) == ("ok", data)
    if len(data) <= 1 << 20:
        assert G.decode(frame, True) == ("ok", data)
    assert w["roundtrip"] == 1, "decompress_frame did not give the input back"
    assert w["walked"] == 0, "decompress_frame followed the chain of a stream this manager indexed"


def test_more_chunks_than_the_length_field_holds(driver):
    r = subprocess.run([driver, "limits"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    most, over, plain = _words(r.stdout)
    assert most == {"chunks": I.MAX_CHUNKS, "status": 0, "bound": 10 + 9 * I.MAX_CHUNKS + 40 + 4 * I.MAX_CHUNKS,
                    "chunks_configured": I.MAX_CHUNKS}
    assert over == {"chunks": I.MAX_CHUNKS + 1, "status": INVALID_VALUE, "bound": 0, "chunks_configured": 0}
    assert plain == {"chunks": I.MAX_CHUNKS + 1, "status": 0, "bound": 10 + 9 * (I.MAX_CHUNKS + 1), "chunks_configured": I.MAX_CHUNKS + 1}


# ---- the indexed read ------------------------------------------------------------------------------------------
MANY = 262200   # more data chunks than one pass of the read path lists (at most 262 144)
LATE = 262190   # (a chunk of the second pass)


def _many_stream(cache={}):
    """(content, the data chunks' bytes): MANY one-byte stored chunks"""
    if not cache:
        content = bytes(i % 251 for i in range(MANY))
        by_byte = [G.stored_chunk(bytes([b])) for b in range(251)]
        cache["x"] = content, b"".join(by_byte[b] for b in content)
    return cache["x"]


def _many_chunks():
    """One-byte stored chunks behind their index, read by a manager of one-byte chunks -- the smallest there is -- in a
    caller-owned scratch buffer."""
    content, body = _many_stream()
    data = G.IDENTIFIER + I.index_chunk([0x00000501] * MANY, 1, MANY) + body
    return I.IndexPlan("many_chunks", data, "ok", "more chunks than a pass lists", content=content, chunks=MANY, declared=MANY)


def _late_refusal():
    """_many_chunks, but index word LATE says "compressed" where the stream says "stored": the fields, the CRC, the
    sum of the lengths and the end of the input behind them hold, the first pass lists, copies and checks its chunks,
    and the listing of the second pass finds another word in the stream than in the index."""
    content, body = _many_stream()
    words = [0x00000501] * MANY
    words[LATE] = 0x00000500
    data = G.IDENTIFIER + I.index_chunk(words, 1, MANY) + body
    return I.IndexPlan("late_refusal", data, "word", "the type of index word %d cleared" % LATE, content=content, chunks=MANY,
                       declared=MANY)


def _read_cases():
    """name -> (plan name, policy, chunk, scratch, offset in, offset out)"""
    cases = {}
    for p in I.plans():
        for policy in (POLICIES if p.name.startswith("wrong_data_crc") else (0, 3, 4)):
            cases["%s/p%d" % (p.name, policy)] = (p.name, policy, CHUNK if policy % 2 else 1024, "scratch" if policy == 4 else "own",
                                                  (policy * 3 + len(p.data)) % 8, (policy + len(p.data)) % 5)
    cases["many_chunks/p3"] = ("many_chunks", 3, 1, "scratch", 1, 1)
    return cases


def _displaced_cases():
    cases = dict(_read_cases())
    cases["late_refusal/p3"] = ("late_refusal", 3, 1, "scratch", 1, 1)
    return cases


def _read(driver, tmp, cmd, cases):
    plans = {p.name: p for p in I.plans() + [_many_chunks(), _late_refusal()]}
    lines, files = [], {}
    for k, (name, (plan, policy, chunk, scratch, off_in, off_out)) in enumerate(cases.items()):
        if plan not in files:
            files[plan] = tmp / ("%d.sz" % len(files))
            files[plan].write_bytes(plans[plan].data)
        lines.append((chunk, policy, files[plan], tmp / ("%d.out" % k), scratch, off_in, off_out))
    words = _run(driver, cmd, tmp, lines, timeout=600)
    return plans, {name: (w, tmp / ("%d.out" % k)) for k, (name, w) in enumerate(zip(cases, words))}


@pytest.fixture(scope="module")
def read_back(driver, tmp_path_factory):
    return _read(driver, tmp_path_factory.mktemp("snappy_frame_index_read"), "read", _read_cases())


@pytest.fixture(scope="module")
def displaced(driver, tmp_path_factory):
    return _read(driver, tmp_path_factory.mktemp("snappy_frame_index_displaced"), "read_displaced", _displaced_cases())


def _check_read(p, policy, w, out):
    assert w["guards"] == 1, ("bytes outside decomp_buffer[0, decomp_data_size) were written", w)
    assert w["scratch_guard"] == 1, ("bytes behind the scratch buffer were written", w)
    # what snappy_framegen plans for the same bytes
    assert w["configured"] == (G.SUCCESS if p.configures else G.CANNOT_DECOMPRESS), (w, p.why)
    assert w["status"] == p.status(policy), (w, p.why)
    assert w["size"] == p.declared and w["chunks"] == p.chunks, (w, p.why)
    if w["status"] == G.SUCCESS:
        assert out.read_bytes() == p.content
    # whether the index served
    assert w["walked"] == (0 if p.applies or not p.configures else p.chunks), (w, p.reason, p.why)


@pytest.mark.parametrize("name", list(_read_cases()))
def test_indexed_read(read_back, name):
    plans, results = read_back
    plan, policy = _read_cases()[name][:2]
    _check_read(plans[plan], policy, *results[name])


@pytest.mark.parametrize("name", list(_displaced_cases()))
def test_indexed_read_decided_on_the_device(displaced, name):
    """The expectations of test_indexed_read, on reads that launch the indexed passes whatever the index is worth."""
    plans, results = displaced
    plan, policy = _displaced_cases()[name][:2]
    _check_read(plans[plan], policy, *results[name])


def test_the_planned_reads_cover_both_ends(read_back, displaced):
    plans, results = displaced
    served = {n for n, (w, _) in results.items() if w["walked"] == 0 and w["chunks"] > 0}
    fell_back = {n for n, (w, _) in results.items() if w["walked"] > 0}
    assert "many_chunks/p3" in served and "late_refusal/p3" in fell_back
    assert {"good/p0", "units_32/p3", "wrong_data_crc_stored/p2", "chunk_bytes_65536/p4"} <= served
    assert {"units_33/p0", "damaged_block/p3", "block_decodes_short/p4", "word_length_plus_1/p0", "wrong_crc/p3"} <= fell_back


# ---- ranged reads ----------------------------------------------------------------------------------------------
RB = 4096
SEVEN = 6 * RB + 1000


def _range_inputs(cache={}):
    """name -> (input, content): seven 4 KiB chunks (compressed, stored, compressed, ..., a short last one), and two
    units with a padding chunk between them"""
    if not cache:
        content = I.mixed(SEVEN, 20, 1024)
        second_content = G.text(2 * RB + 33, 21)
        seven = I.written_form(content, RB, "cscscsc")
        cache["seven"] = (seven, content)
        cache["two_units"] = (seven + G.padding(7) + I.written_form(second_content, RB, "scc"), content + second_content)
    return cache


def _ranges(total, first_unit):
    r = {"empty": (1234, 0), "one_byte": (5000, 1), "first_byte": (0, 1), "last_byte": (total - 1, 1), "inside_one_chunk": (4200, 300),
         "across_one_boundary": (4000, 200), "across_stored_and_compressed": (8000, 500), "from_0": (0, 6000),
         "to_the_last_byte": (20000, total - 20000), "whole": (0, total), "one_byte_beyond": (total - 10, 11)}
    if total > first_unit:
        r["across_the_units"] = (first_unit - 100, 300)
        r["inside_the_second_unit"] = (first_unit + 4096 + 7, 4096)
    return r


def _flip(data, chunk):
    """(the input with one bit in the middle of data chunk `chunk` of the single unit flipped, what snappy_framegen
    says of the chunk then: "ok" -- other bytes of the same number -- or the reason its block does not decode)"""
    reason, _, h = I.index_applies(data, 0)
    assert reason == "ok"
    pos = 10 + I.index_bytes(h["chunks"]) + sum(4 + (w >> 8) for w in h["words"][:chunk])
    word = h["words"][chunk]
    at = pos + 8 + ((word >> 8) - 4) // 2
    out = data[:at] + bytes([data[at] ^ 0x20]) + data[at + 1:]
    verdict = "ok"
    if not word & 0xFF:
        try:
            G.decode_block(out[pos + 8:pos + 4 + (word >> 8)])
        except G.Refused as r:
            verdict = r.reason
    return out, verdict


def _range_cases():
    """name -> (input name or plan name, policy, scratch, first, count, what is done to the input)"""
    cases = {}
    for name in ("seven", "two_units"):
        total = SEVEN if name == "seven" else SEVEN + 2 * RB + 33
        for rname, (first, count) in _ranges(total, SEVEN).items():
            for policy in (0, 3):
                cases["%s/%s/p%d" % (name, rname, policy)] = (name, policy, "scratch" if policy == 3 and rname == "whole" else "own",
                                                             first, count, "")
    cases["seven/whole/p4"] = ("seven", 4, "own", 0, SEVEN, "")
    # a flipped bit in the middle of the stored chunk 1 (inside the range read), and of the compressed chunk 4
    for policy in (0, 3):
        cases["seven/flip_touched_stored/p%d" % policy] = ("seven", policy, "own", RB + RB // 2 - 8, 20, "flip1")
        cases["seven/flip_touched_compressed/p%d" % policy] = ("seven", policy, "own", 4 * RB + 10, 20, "flip4")
        cases["seven/flip_untouched/p%d" % policy] = ("seven", policy, "own", 4 * RB + 10, 20, "flip1")
    for p in I.plans():
        if not p.applies and p.configures and p.declared > 0 and p.device_refuses != "decode":
            cases["plan_%s/p3" % p.name] = ("plan:" + p.name, 3, "own", 0, min(10, p.declared), "")
    # chunk 2 of the planned unit does not decode, chunk 4 decodes short: seen where the range touches them
    cases["plan_damaged_block/untouched"] = ("plan:damaged_block", 3, "own", 5, 300, "")
    cases["plan_damaged_block/touched"] = ("plan:damaged_block", 3, "own", 2 * I.CB + 5, 10, "")
    cases["plan_block_decodes_short/untouched"] = ("plan:block_decodes_short", 0, "own", 5 * I.CB + 1, 300, "")
    cases["plan_block_decodes_short/touched"] = ("plan:block_decodes_short", 0, "own", 4 * I.CB + 250, 10, "")
    return cases


@pytest.fixture(scope="module")
def ranged(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("snappy_frame_index_range")
    inputs = _range_inputs()
    plans = {p.name: p for p in I.plans()}
    cases = _range_cases()
    lines, files, content, verdicts = [], {}, {}, {}
    for k, (name, (src, policy, scratch, first, count, damage)) in enumerate(cases.items()):
        if (src, damage) not in files:
            if src.startswith("plan:"):
                p = plans[src[5:]]
                data, want = p.data, (p.content if p.plain_reason == "ok" else I.plans()[0].content)
            else:
                data, want = inputs[src]
            if damage:
                data, verdicts[src, damage] = _flip(data, int(damage[4:]))
            files[src, damage] = tmp / ("%d.sz" % len(files))
            files[src, damage].write_bytes(data)
            content[src] = want
        lines.append((RB, policy, files[src, damage], tmp / ("%d.out" % k), scratch, (k * 3) % 8, (k * 5) % 7, first, count))
    words = _run(driver, "range", tmp, lines, timeout=600)
    return cases, content, verdicts, plans, {name: (w, tmp / ("%d.out" % k)) for k, (name, w) in enumerate(zip(cases, words))}


@pytest.mark.parametrize("name", list(_range_cases()))
def test_ranged_read(ranged, name):
    cases, content, verdicts, plans, results = ranged
    src, policy, _, first, count, damage = cases[name]
    w, out = results[name]
    want = content[src][first:first + count]
    got = out.read_bytes()
    assert w["guards"] == 1, ("bytes outside out[0, num_bytes) were written", w)
    assert w["scratch_guard"] == 1, ("bytes behind the scratch buffer were written", w)
    assert w["walked"] == 0, "a ranged read followed the chain"
    assert w["configured"] == 0, w
    if src.startswith("plan:") and not plans[src[5:]].applies and plans[src[5:]].device_refuses != "decode":
        assert w["untouched"] == 1 and w["status"] == NOT_SUPPORTED, (w, plans[src[5:]].why)
        return
    if "/one_byte_beyond/" in name:
        assert w["status"] == INVALID_VALUE and w["untouched"] == 1, w
        return
    if name.endswith("/touched"):   # (a block that does not decode to its share, the planned unit's other chunks sound)
        assert w["status"] == G.CANNOT_DECOMPRESS, w
        return
    touched = {"flip1": 1, "flip4": 4}.get(damage, -1) in range(first // RB, (first + count - 1) // RB + 1) if count else False
    if touched:
        verdict = verdicts[src, damage]
        if verdict != "ok":
            assert w["status"] == G.CANNOT_DECOMPRESS, (w, verdict)
        elif policy == 3:
            assert w["status"] == G.BAD_CHECKSUM, w
        else:
            assert w["status"] == G.SUCCESS and len(got) == len(want), w
            if damage == "flip1":
                assert got != want   # (a damaged stored chunk read without its CRC)
        return
    assert w["status"] == G.SUCCESS, w
    assert got == want
    if count == 0:
        assert w["untouched"] == 1
