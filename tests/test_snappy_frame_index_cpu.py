"""The host logic of seekable Snappy framed streams (csrc/snappy_frame_index.hpp: the index writer, the parser with a
reason per refusal, the tests an index has to pass before it is used) through
tests/snappy_frame_index_driver_cpu.cpp, a plain C++ program -- built once as it is and once with
-fsanitize=address,undefined and run as a program -- against tests/snappy_frame_indexgen.py, the same said in Python,
and against pyarrow's Snappy codec, which decodes every legal planned stream chunk by chunk."""
import os
import struct
import subprocess

import pyarrow as pa
import pytest

import snappy_frame_indexgen as I
import snappy_framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "snappy_frame_index_driver_cpu.cpp")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, r = _build(tmp_path_factory.mktemp("snappy_frame_index_cpu"), "driver")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def plans():
    return I.plans()


def _records(plans):
    """(name, input): the planned inputs; the good one cut at every length of its identifier and index and a little
    beyond, and with every byte of them changed; the two-unit one cut inside its second identifier and index"""
    out = [(p.name, p.data) for p in plans]
    good = next(p for p in plans if p.name == "good").data
    head = 10 + I.index_bytes(7)
    for cut in range(head + 24):
        out.append(("good cut at %d" % cut, good[:cut]))
    for at in range(head + 15):
        out.append(("good byte %d" % at, good[:at] + bytes([good[at] ^ 0x41]) + good[at + 1:]))
    two = next(p for p in plans if p.name == "two_units").data
    for cut in range(len(good), len(good) + 10 + 40 + 30):
        out.append(("two_units cut at %d" % cut, two[:cut]))
    return out


def _check(exe, tmp_path, records):
    (tmp_path / "records.bin").write_bytes(b"".join(struct.pack("<I", len(d)) + d for _, d in records))
    r = subprocess.run([exe, "check", str(tmp_path / "records.bin")], capture_output=True, text=True)
    return r, [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def _model(data):
    reason, units, chunks, content = I.input_is_indexed(data)
    first, end, _ = I.index_applies(data, 0)
    return (I.REASONS[reason], units, chunks, content, I.REASONS[first], end if first == "ok" else 0)


def test_every_planned_reason_is_met_and_nothing_else(plans):
    names = [p.name for p in plans]
    assert len(set(names)) == len(names)
    assert {p.reason for p in plans} == set(I.REASONS) - set(I.DEVICE_REASONS)
    assert {p.device_refuses for p in plans if p.device_refuses} == set(I.DEVICE_REASONS)
    for p in plans:
        reason, units, chunks, content = I.input_is_indexed(p.data)
        assert reason == p.reason, p.name
        if reason == "ok":
            # an index that applies says what the chain says
            assert p.configures and chunks == p.chunks and content == p.declared, p.name
            assert units <= I.MAX_UNITS or p.device_refuses == "too_many_units"
        if p.applies:
            assert p.plain_reason == "ok" and len(p.content) == p.declared, p.name
        if p.device_refuses == "decode":
            assert p.plain_reason in ("bad_block", "size_mismatch"), p.name
    # the forms the issue names
    by = {p.name: p for p in plans}
    assert by["good_empty"].data == G.IDENTIFIER + I.index_chunk([], I.CB, 0) and len(by["good_empty"].data) == 50
    assert [by["chunk_bytes_%d" % n].applies for n in (1, 1000, 65536)] == [True] * 3
    assert by["units_32"].applies and not by["units_33"].applies
    for name in ("wrong_data_crc_stored", "wrong_data_crc_compressed"):
        p = by[name]
        assert p.applies and p.bad_crc and [p.status(k) for k in range(5)] == [0, 0, 13, 13, 13]


def test_driver_gives_the_generators_reasons(driver, plans, tmp_path):
    records = _records(plans)
    r, got = _check(driver, tmp_path, records)
    assert r.returncode == 0 and len(got) == len(records), r.stderr
    seen = set()
    for (name, data), g in zip(records, got):
        assert g == _model(data), name
        seen.add(g[0])
    assert seen == {I.REASONS[k] for k in I.REASONS if k not in I.DEVICE_REASONS}
    planned = {p.name: p for p in plans}
    for (name, _), g in zip(records, got):
        if name in planned:
            assert g[0] == I.REASONS[planned[name].reason], name


def test_writer_writes_the_generators_indexes(driver, tmp_path):
    cases = [([], 65536, 0), ([0x00000501], 1, 1), ([0x00010401, 0x00001100, 0x00006801], 256, 612),
             ([(i * 2654435761) & 0xFFFFFFFF for i in range(300)], 65536, (299 << 16) + 1),
             # a body of more than one 64 KiB piece
             ([(i * 40503) & 0xFFFFFFFF for i in range(40000)], 3, 3 * 40000 - 1)]
    blob = b"".join(struct.pack("<IIQ", len(w), cb, content) + struct.pack("<%dI" % len(w), *w) for w, cb, content in cases)
    (tmp_path / "indexes.bin").write_bytes(blob)
    r = subprocess.run([driver, "write", str(tmp_path / "indexes.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    assert len(lines) == len(cases)
    for (w, cb, content), line in zip(cases, lines):
        want = I.index_chunk(w, cb, content)
        assert bytes.fromhex(line) == want and len(want) == 40 + 4 * len(w)
        assert I.parse_index(want, 0)[0] == "ok"
        # for a reader that knows nothing of it: one reserved skippable chunk
        assert G.parse_chunk(G.IDENTIFIER + want, 10, False) == ("skipped", len(want), 0, 0, 0)


def test_size_and_offset_arithmetic(driver):
    out = subprocess.run([driver, "arith"], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [tuple(int(x) for x in line.split()) for line in out]
    assert len(rows) == 36
    for c, b, n, index, first, last, stored_chunk, bound in rows:
        assert n == -(-c // b)
        fits = 0 < n <= 0xFFFFFFFF
        assert index == 40 + 4 * n
        assert first == ((b if n > 1 else c) if fits else 0)
        assert last == (c - b * (n - 1) if fits else 0)
        assert stored_chunk == 4 + 4 + b
        assert bound == 10 + 7 * (b + 8) + 40 + 4 * 7
    assert I.MAX_CHUNKS == 4194294 and 36 + 4 * I.MAX_CHUNKS <= 0xFFFFFF < 36 + 4 * (I.MAX_CHUNKS + 1)


def _pyarrow_block(payload: bytes) -> bytes:
    pre = G.read_varint(payload, 0, len(payload))
    if pre is None:
        raise G.Refused("bad_block")
    try:
        return pa.Codec("snappy").decompress(payload, pre[0]).to_pybytes()
    except Exception:   # (pyarrow.lib.ArrowIOError: "Corrupt snappy compressed data.")
        raise G.Refused("bad_block")


@pytest.mark.parametrize("plan", [p for p in I.plans() if p.plain_reason == "ok"], ids=lambda p: p.name)
def test_legal_planned_streams_decode_with_pyarrow(plan):
    """Every planned stream that is a sound .sz stream, index or forged index and all, chunk by chunk."""
    chunks = G.parse(plan.data)
    assert len(chunks) == plan.chunks and sum(c[2] for c in chunks) == plan.declared == len(plan.content)
    assert G.decode(plan.data, False, _pyarrow_block) == ("ok", plan.content)
    assert G.decode(plan.data, True, _pyarrow_block) == (("bad_checksum", None) if plan.bad_crc else ("ok", plan.content))
    if plan.applies:
        # the index says where every chunk stands and what it holds
        pos = 0
        at = 0
        for _ in range(I.input_is_indexed(plan.data)[1]):
            reason, end, h = I.index_applies(plan.data, at)
            assert reason == "ok"
            at_chunk = at + 10 + I.index_bytes(h["chunks"])
            for i, word in enumerate(h["words"]):
                share = min(h["chunk_bytes"], h["content_bytes"] - i * h["chunk_bytes"])
                body = plan.data[at_chunk + 8:at_chunk + 4 + (word >> 8)]
                got = body if word & 0xFF else _pyarrow_block(body)
                assert got == plan.content[pos:pos + share], (plan.name, i)
                pos += share
                at_chunk += 4 + (word >> 8)
            assert at_chunk == end
            _, at, _ = I.step_behind(plan.data, end)
        assert pos == len(plan.content)


def test_sanitized_driver_runs_clean_over_every_record(plans, tmp_path):
    exe, r = _build(tmp_path, "driver_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert r.returncode == 0, "the sanitizer runtime does not link here:\n" + r.stderr
    records = _records(plans)
    run, got = _check(exe, tmp_path, records)
    assert run.returncode == 0 and len(got) == len(records), run.stderr[-2000:]
    assert got == [_model(d) for _, d in records]
    for cmd in (["arith"],):
        x = subprocess.run([exe, *cmd], capture_output=True, text=True)
        assert x.returncode == 0, x.stderr[-2000:]
