"""The host logic of seekable LZ4 frames (csrc/lz4_frame_index.hpp: the index writer, the parser with a reason per
refusal, the tests an index has to pass before it is used) through tests/lz4_frame_index_driver_cpu.cpp, a plain C++
program -- built once as it is and once with -fsanitize=address,undefined and run as a program -- against
tests/lz4_frame_indexgen.py, the same said in Python, and against liblz4, for which an index is a skippable frame."""
import os
import struct
import subprocess

import pytest

import lz4_frame_indexgen as I
import lz4_framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lz4_frame_index_driver_cpu.cpp")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, r = _build(tmp_path_factory.mktemp("lz4_frame_index_cpu"), "driver")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def plans():
    return I.plans()


def _records(plans):
    """(name, input): the planned inputs; the good one cut at every length of its index and a little beyond, and
    with every byte of its index changed; the two-frame one cut inside its second index"""
    out = [(p.name, p.data) for p in plans]
    good = next(p for p in plans if p.name == "good").data
    n_index = I.index_bytes(7)
    for cut in range(n_index + 24):
        out.append(("good cut at %d" % cut, good[:cut]))
    for at in range(n_index + 15):
        out.append(("good byte %d" % at, good[:at] + bytes([good[at] ^ 0x41]) + good[at + 1:]))
    two = next(p for p in plans if p.name == "two_frames").data
    for cut in range(len(good), len(good) + 23 + 50):
        out.append(("two_frames cut at %d" % cut, two[:cut]))
    return out


def _check(exe, tmp_path, records):
    (tmp_path / "records.bin").write_bytes(b"".join(struct.pack("<I", len(d)) + d for _, d in records))
    r = subprocess.run([exe, "check", str(tmp_path / "records.bin")], capture_output=True, text=True)
    return r, [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def _model(data):
    reason, frames, blocks, content = I.input_is_indexed(data)
    first, end, _ = I.index_applies(data, 0)
    return (I.REASONS[reason], frames, blocks, content, I.REASONS[first], end if first == "ok" else 0)


def test_every_planned_reason_is_met_and_nothing_else(plans):
    names = [p.name for p in plans]
    assert len(set(names)) == len(names)
    for p in plans:
        assert I.input_is_indexed(p.data)[0] == p.reason, p.name
    assert {p.reason for p in plans} == set(I.REASONS) - set(I.DEVICE_REASONS)
    good = [p for p in plans if p.reason == "ok"]
    assert [p.name for p in good if p.device_refuses] == ["short_interior_blocks"]
    for p in good:
        _, frames, blocks, content = I.input_is_indexed(p.data)
        assert blocks == p.blocks and content == len(p.content), p.name


def test_driver_gives_the_generators_reasons(driver, plans, tmp_path):
    records = _records(plans)
    r, got = _check(driver, tmp_path, records)
    assert r.returncode == 0 and len(got) == len(records), r.stderr
    seen = set()
    for (name, data), g in zip(records, got):
        assert g == _model(data), name
        seen.add(g[0])
    assert seen == {I.REASONS[k] for k in I.REASONS if k not in I.DEVICE_REASONS}
    for p, g in zip(plans, got):
        assert g[0] == I.REASONS[p.reason], p.name


def test_writer_writes_the_generators_indexes(driver, tmp_path):
    cases = [([], 65536, 0, 0), ([5], 1, 1, 0), ([0x80000100, 17, 0x80000064], 256, 612, 1),
             ([(i * 2654435761) & 0xFFFFFFFF for i in range(300)], 4 << 20, (299 << 22) + 1, 1)]
    blob = b"".join(struct.pack("<IIQI", len(w), bb, content, sums) + struct.pack("<%dI" % len(w), *w) for w, bb, content, sums in cases)
    (tmp_path / "indexes.bin").write_bytes(blob)
    r = subprocess.run([driver, "write", str(tmp_path / "indexes.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    assert len(lines) == len(cases)
    for (w, bb, content, sums), line in zip(cases, lines):
        want = I.index_frame(w, bb, content, bool(sums))
        assert bytes.fromhex(line) == want and len(want) == 44 + 4 * len(w)
        assert I.parse_index(want + b"\0" * 8, 0)[0] == "ok"


def test_size_and_offset_arithmetic(driver):
    out = subprocess.run([driver, "arith"], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [tuple(int(x) for x in line.split()) for line in out]
    assert len(rows) == 40
    for c, b, n, index, first, last, stored_block, bound in rows:
        assert n == -(-c // b)
        fits = 0 < n <= 0xFFFFFFFF
        assert index == 44 + 4 * (n if n <= 0xFFFFFFFF else 0)
        assert first == ((b if n > 1 else c) if fits else 0)
        assert last == (c - b * (n - 1) if fits else 0)
        assert stored_block == 4 + b + 4
        assert bound == 44 + 4 * 7 + 15 + 7 * (b + 4 + 4 * (c & 1)) + 4


def test_liblz4_reads_every_planned_input_with_and_without_its_index(plans):
    L = G.load_lz4f()
    if L is None:
        print("liblz4.so.1 absent: the planned inputs were not given to LZ4F_decompress")
        return
    for p in plans:
        with_index, without = G.lz4f_decompress(L, p.data), G.lz4f_decompress(L, p.bare)
        assert with_index[0] == without[0] == p.sound, p.name
        if p.sound:
            assert with_index[1] == without[1] == p.content, p.name
        assert I.INDEX_MAGIC.to_bytes(4, "little") not in p.bare[:4] and len(p.bare) <= len(p.data), p.name
        # the planned statuses follow that verdict: a sound input succeeds unless ComputeAndVerify finds a bare frame
        bare_frame = any(not f["block_sums"] and not f["content_sum"] for f in G.parse(p.bare)) if p.sound else False
        assert [p.status(k) for k in range(5)] == ([G.CANNOT_DECOMPRESS] * 5 if not p.sound else
                                                   [G.SUCCESS] * 4 + [G.CANNOT_VERIFY if bare_frame else G.SUCCESS]), p.name


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
