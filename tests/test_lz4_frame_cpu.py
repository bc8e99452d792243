"""The host logic of the LZ4 frame path (csrc/lz4_frame.hpp: the descriptor parse with a reason per refusal, the
descriptor writer, the size-word / block-maximum arithmetic, the frame bound) through tests/lz4_frame_driver_cpu.cpp,
a plain C++ program -- built once as it is and once with -fsanitize=address,undefined and run as a program."""
import os
import struct
import subprocess

import pytest

import lz4_framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lz4_frame_driver_cpu.cpp")
HEADER_REASONS = ("unknown_magic", "legacy_magic", "bad_version", "reserved_bit", "block_max_code", "header_checksum", "dict_id")
HEADER_CUTS = ("after_magic", "after_flg", "after_bd", "inside_content_size", "before_hc")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, r = _build(tmp_path_factory.mktemp("lz4_frame_cpu"), "driver")
    assert r.returncode == 0, r.stderr
    return exe


def model_parse(p: bytes):
    """csrc/lz4_frame.hpp, parse_descriptor, said again: (reason, header_bytes) -- the order of LZ4F_decodeHeader's tests"""
    if len(p) < 4:
        return "truncated", 0
    magic, = struct.unpack_from("<I", p)
    if magic == G.LEGACY_MAGIC:
        return "legacy_magic", 0
    if magic != G.MAGIC:
        return "unknown_magic", 0
    if len(p) < 5:
        return "truncated", 0
    flg = p[4]
    if flg & 2:
        return "reserved_bit", 0
    if flg >> 6 != 1:
        return "bad_version", 0
    n = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if len(p) < n:
        return "truncated", n
    bd = p[5]
    if bd & 0x80:
        return "reserved_bit", n
    if (bd >> 4) & 7 < 4:
        return "block_max_code", n
    if bd & 15:
        return "reserved_bit", n
    if p[n - 1] != (G.xxh32(p[4:n - 1]) >> 8) & 0xFF:
        return "header_checksum", n
    if flg & 1:
        return "dict_id", n
    return "ok", n


def _records():
    """(name, the front of an input, the planned reason): the planner's inputs that start with a frame, and every FLG
    byte with BD bytes of every kind, sound and with a wrong HC, cut at every length"""
    out = []
    for p in G.all_plans():
        if p.name in ("no_bytes", "only_skippable", "two_frames_skippable"):
            continue
        want = "ok"
        if p.reason in HEADER_REASONS and p.name != "unknown_magic_behind_a_frame":
            want = p.reason
        if p.truncated_at in HEADER_CUTS:
            want = "truncated"
        out.append((p.name, p.data, want))
    for flg in range(256):
        for bd in (0x40, 0x50, 0x60, 0x70, 0x30, 0x00, 0xC0, 0x41, 0x78):
            d = bytes([flg, bd]) + (struct.pack("<Q", 0x0102030405060708) if flg & 8 else b"") + (b"\x11\x22\x33\x44" if flg & 1 else b"")
            h = struct.pack("<I", G.MAGIC) + d + bytes([(G.xxh32(d) >> 8) & 0xFF])
            out.append(("flg %02x bd %02x" % (flg, bd), h + b"\0\0\0\0", None))
            if bd == 0x40:
                out.append(("flg %02x bad hc" % flg, h[:-1] + bytes([h[-1] ^ 0xFF]), None))
                for cut in range(len(h)):
                    out.append(("flg %02x cut %d" % (flg, cut), h[:cut], None))
    return out


def _parse_all(exe, tmp_path, records):
    blob = b"".join(struct.pack("<I", len(d)) + d for _, d, _ in records)
    (tmp_path / "records.bin").write_bytes(blob)
    r = subprocess.run([exe, "parse", str(tmp_path / "records.bin")], capture_output=True, text=True)
    return r, [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_descriptor_parse_gives_the_planned_reason(driver, tmp_path):
    records = _records()
    r, got = _parse_all(driver, tmp_path, records)
    assert r.returncode == 0 and len(got) == len(records), r.stderr
    seen = set()
    for (name, data, want), g in zip(records, got):
        reason, n = model_parse(data)
        assert want is None or want == reason, name
        assert g[0] == G.REASONS[reason], (name, g, reason)
        seen.add(reason)
        if reason == "ok":
            flg, bd = data[4], data[5]
            size = struct.unpack_from("<Q", data, 6)[0] if flg & 8 else 0
            assert g[1:] == (n, G.BLOCK_MAX[bd >> 4], int(not flg & 0x20), (flg >> 4) & 1, (flg >> 2) & 1, (flg >> 3) & 1, size), name
    assert seen == {"ok", "truncated"} | set(HEADER_REASONS)


def test_descriptor_writer_writes_the_generators_descriptors(driver):
    for code in (4, 5, 6, 7):
        for size in (0, 1, 65536, (1 << 40) + 12345, (1 << 64) - 1):
            for sums in (0, 1):
                out = subprocess.run([driver, "write", str(code), str(size), str(sums)], capture_output=True, text=True, check=True)
                want = G.descriptor(code, False, bool(sums), False, size)
                assert bytes.fromhex(out.stdout.strip()) == want and len(want) == 15


def test_block_arithmetic_and_bound(driver):
    for chunk, code in ((1, 4), (65536, 4), (65537, 5), (262144, 5), (262145, 6), (1 << 20, 6), ((1 << 20) + 1, 7),
                        (4 << 20, 7), ((4 << 20) + 1, 0), (16 << 20, 0)):
        for stream in (1, chunk - 1, chunk, chunk + 1, chunk + 264):
            for sums in (0, 1):
                n = 7
                out = subprocess.run([driver, "arith", str(chunk), str(stream), str(n), str(sums)], capture_output=True, text=True,
                                     check=True).stdout.split()
                stored = stream >= chunk
                body = chunk if stored else stream
                assert [int(x) for x in out] == [code, G.BLOCK_MAX.get(code, 0), int(stored), body | (0x80000000 if stored else 0),
                                                 4 + body + 4 * sums, 15 + n * (chunk + 4 + 4 * sums) + 4], (chunk, stream, sums)
    # the bound holds: a written frame of n chunks, the last one short, every block stored at worst
    for n, last in ((1, 1), (3, 65536), (5, 123)):
        for sums in (False, True):
            chunks = [bytes(65536)] * (n - 1) + [bytes(last)]
            worst = G.written_frame(chunks, [c + b"x" for c in chunks], 65536, sums)
            assert len(worst) <= 15 + n * (65536 + 4 + 4 * sums) + 4


def test_sanitized_driver_runs_clean_over_all_hostile_headers(tmp_path):
    exe, r = _build(tmp_path, "driver_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert r.returncode == 0, "the sanitizer runtime does not link here:\n" + r.stderr
    records = _records()
    run, got = _parse_all(exe, tmp_path, records)
    assert run.returncode == 0 and len(got) == len(records), run.stderr[-2000:]
    data = bytes((i * 131 + 7) & 0xFF for i in range(100))
    (tmp_path / "d.bin").write_bytes(data)
    x = subprocess.run([exe, "xxh32", str(tmp_path / "d.bin")], capture_output=True, text=True)
    assert x.returncode == 0 and [int(v) for v in x.stdout.split()] == [G.xxh32(data[:n]) for n in range(101)], x.stderr[-2000:]
