"""The host logic of the Snappy framed-stream path (csrc/snappy_frame.hpp: the chunk parse with a reason per refusal,
the varint, mask and unmask, the bound; csrc/crc32c_math.hpp: tables, slice-by-16, the shift algebra) through
tests/snappy_frame_driver_cpu.cpp, a plain C++ program -- built once as it is and once with
-fsanitize=address,undefined and run as a program -- held to tests/snappy_framegen.py."""
import os
import struct
import subprocess

import pytest

import snappy_framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "snappy_frame_driver_cpu.cpp")
KINDS = {"skipped": 0, "compressed": 1, "stored": 2}


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, r = _build(tmp_path_factory.mktemp("snappy_frame_cpu"), "driver")
    assert r.returncode == 0, r.stderr
    return exe


def _model(data: bytes, first: bool):
    """(reason, kind, bytes, payload, content, crc) by the generator's parser; the fields of a refused chunk are not
    compared"""
    try:
        kind, n, payload, content, crc = G.parse_chunk(data, 0, first)
    except G.Refused as r:
        return (G.REASONS[r.reason],)
    return G.REASONS["ok"], KINDS[kind], n, payload, content, crc


def _chunk_records():
    """(name, first, bytes from a chunk's first byte to the input's end): every plan's front; every chunk of every plan
    the walk accepts; every type byte with length fields 0 - 8, the body there, one byte short, and followed by more"""
    out = []
    for p in G.all_plans():
        if p.data:
            out.append((p.name, True, p.data))
        at = 0
        while at < len(p.data):   # (up to and with the chunk the walk refuses)
            out.append(("%s @%d" % (p.name, at), at == 0, p.data[at:at + 70]))
            if 70 < len(p.data) - at < 150000:   # (the parse looks at 13 bytes and at the length: the rest whole as well)
                out.append(("%s @%d whole" % (p.name, at), at == 0, p.data[at:]))
            try:
                at += G.parse_chunk(p.data, at, at == 0)[1]
            except G.Refused:
                break
    body = b"sNaPpY\x85\x80"
    for kind in range(256):
        for n in range(9):
            head = bytes([kind]) + n.to_bytes(3, "little")
            for first in (False, True):
                out.append(("type %02x length %d" % (kind, n), first, head + body[:n]))
            out.append(("type %02x length %d more" % (kind, n), False, head + body[:n] + b"\x01\x02\x03"))
            if n:
                out.append(("type %02x length %d short" % (kind, n), False, head + body[:n - 1]))
            for cut in range(4):
                out.append(("type %02x header cut %d" % (kind, cut), kind == 0xff, head[:cut]))
    # preambles of every length around the limits
    for pre in (b"\x00", b"\x7f", b"\x80\x01", b"\x80\x80\x04", b"\x81\x80\x04", b"\xff\xff\x03", b"\x80\x80\x80\x01",
                b"\x80\x80\x80\x80\x00", b"\x80\x80\x80\x80\x10", b"\xff\xff\xff\xff\x7f", b"\x80\x80\x80\x80\x80", b"\x80\x80"):
        out.append(("preamble %s" % pre.hex(), False, G.compressed_chunk(pre, b"")))
        out.append(("preamble %s and more" % pre.hex(), False, G.compressed_chunk(pre + b"\x00\x00", b"")))
    return out


def _run_records(exe, tmp_path, cmd, records):
    blob = b"".join((bytes([first]) if cmd == "parse" else b"") + struct.pack("<I", len(d)) + d for _, first, d in records)
    (tmp_path / (cmd + ".bin")).write_bytes(blob)
    r = subprocess.run([exe, cmd, str(tmp_path / (cmd + ".bin"))], capture_output=True, text=True)
    return r, [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def _check_parse(exe, tmp_path):
    records = [r for r in _chunk_records() if r[2]]
    run, got = _run_records(exe, tmp_path, "parse", records)
    assert run.returncode == 0 and len(got) == len(records), run.stderr[-2000:]
    seen = set()
    for (name, first, data), g in zip(records, got):
        want = _model(data, first)
        assert g[:len(want)] == want, (name, g, want)
        seen.add(want[0])
    assert seen == {G.REASONS[r] for r in ("ok",) + G.WALK_REASONS}


def _check_walk(exe, tmp_path):
    plans = G.all_plans()
    run, got = _run_records(exe, tmp_path, "walk", [(p.name, True, p.data) for p in plans])
    assert run.returncode == 0 and len(got) == len(plans), run.stderr[-2000:]
    for p, g in zip(plans, got):
        if p.configures:
            assert g == (0, p.chunks, p.declared, len(p.data)), p.name
        else:
            assert g[0] == G.REASONS[p.reason], (p.name, g)


def test_chunk_parse_gives_the_generators_reason_and_fields(driver, tmp_path):
    _check_parse(driver, tmp_path)


def test_the_chain_walk_gives_every_plans_verdict(driver, tmp_path):
    _check_walk(driver, tmp_path)


def _check_crc(exe, tmp_path):
    data = bytes((i * 131 + 7) & 0xFF for i in range(100))
    (tmp_path / "d.bin").write_bytes(data)
    x = subprocess.run([exe, "crc", str(tmp_path / "d.bin")], capture_output=True, text=True)
    assert x.returncode == 0, (x.returncode, x.stderr[-2000:])   # (5: slice-by-16 and bytewise differ)
    assert [int(v) for v in x.stdout.split()] == [G.crc32c(data[:n]) for n in range(101)]
    big = G.noise(4096, 2)
    (tmp_path / "big.bin").write_bytes(big)
    j = subprocess.run([exe, "join", str(tmp_path / "big.bin")], capture_output=True, text=True)
    assert j.returncode == 0, j.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in j.stdout.splitlines()]
    assert len(rows) == 9 and all(r == (G.crc32c(big), G.crc32c(big)) for r in rows), rows


def test_slice_by_16_and_the_shift_identity(driver, tmp_path):
    _check_crc(driver, tmp_path)


def test_crc_vectors_through_the_header(driver, tmp_path):
    for data, want in ((b"123456789", 0xE3069283), (bytes(32), 0x8A9136AA), (b"\xff" * 32, 0x62A8AB43),
                       (bytes(range(32)), 0x46DD794E), (bytes(range(31, -1, -1)), 0x113FDB5C)):
        (tmp_path / "v.bin").write_bytes(data)
        out = subprocess.run([driver, "crc", str(tmp_path / "v.bin")], capture_output=True, text=True, check=True).stdout.split()
        assert int(out[-1]) == want


def test_mask_and_unmask(driver):
    for c in (0, 1, 0xE3069283, 0xFFFFFFFF, 0x80000000, 0x7FFF, 0x8000, 0x5D7D1528):
        out = subprocess.run([driver, "mask", str(c)], capture_output=True, text=True, check=True).stdout.split()
        assert [int(x) for x in out] == [G.mask(c), c]
    assert G.mask(0xE3069283) == 0xC78AB0E5


def test_written_chunk_arithmetic_and_bound(driver):
    for chunk in (1, 1024, 65535, 65536):
        for block in (1, chunk - 1, chunk, chunk + 1, chunk + 20):
            if block < 1:
                continue
            n = 7
            out = subprocess.run([driver, "arith", str(chunk), str(block), str(n)], capture_output=True, text=True,
                                 check=True).stdout.split()
            stored = block >= chunk
            body = chunk if stored else block
            head, = struct.unpack("<I", bytes([1 if stored else 0]) + (body + 4).to_bytes(3, "little"))
            assert [int(x) for x in out] == [int(stored), 8 + body, head, 10 + n * (chunk + 8)], (chunk, block)
    # the bound holds: a written stream of n chunks, the last one short, every chunk stored at worst
    for n, last in ((1, 1), (3, 65536), (5, 123)):
        chunks = [bytes(65536)] * (n - 1) + [bytes(last)]
        worst = G.written_stream(chunks, [c + b"x" for c in chunks])
        assert len(worst) <= 10 + n * (65536 + 8)
    assert G.written_stream([], []) == G.IDENTIFIER


def test_sanitized_driver_runs_clean_over_all_plans_and_chunks(tmp_path):
    exe, r = _build(tmp_path, "driver_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert r.returncode == 0, "the sanitizer runtime does not link here:\n" + r.stderr
    _check_parse(exe, tmp_path)
    _check_walk(exe, tmp_path)
    _check_crc(exe, tmp_path)
