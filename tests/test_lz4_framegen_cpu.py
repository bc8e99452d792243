"""tests/lz4_framegen.py held to what it restates: its XXH32 to the known vectors, to the header checksums liblz4
writes and to csrc/xxh32_math.hpp (through tests/lz4_frame_driver_cpu.cpp); its planned frames to liblz4's
LZ4F_decompress -- every legal one accepted with the planned bytes, every hostile one refused -- and a census that
every refusal and every truncation point the reader owes a status for is planned.

The differences from LZ4F_decompress are documented ones ("LZ4 frames"): a frame with a dictionary
id is hipcompErrorNotSupported here and decoded there where it uses none of the dictionary; the legacy magic is
refused by both, here as hipcompErrorNotSupported; checksums are skipped here under a non-verifying ChecksumPolicy
and always verified there."""
import json
import os
import subprocess

import pytest

import lz4_framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lz4_frame")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lz4_frame_cpu") / "lz4_frame_driver_cpu")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                        os.path.join(ROOT, "tests", "lz4_frame_driver_cpu.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def lz4f():
    L = G.load_lz4f()
    if L is None:
        pytest.skip("liblz4.so.1 absent: the planner is not compared with LZ4F_decompress")
    return L


def test_xxh32_known_vectors():
    assert G.xxh32(b"") == 0x02CC5D05
    assert G.xxh32(b"", 1) == 0x0B2CB792
    assert G.xxh32(b"a") == 0x550D7456
    assert G.xxh32(b"abc") == 0x32D153FF
    assert G.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


def test_xxh32_is_the_header_checksum_liblz4_writes():
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    seen = 0
    for name in manifest:
        if name == "liblz4":
            continue
        frame = open(os.path.join(GOLDEN, name + ".lz4"), "rb").read()
        n = 2 + (8 if frame[4] & 8 else 0)
        assert frame[4 + n] == (G.xxh32(frame[4:4 + n]) >> 8) & 0xFF, name
        seen += 1
    assert seen >= 10


def test_xxh32_math_header_agrees_at_every_length(driver, tmp_path):
    """lengths 0 - 40 and around every multiple of 16 up to 272: every prefix of one buffer"""
    data = bytes((i * 197 + 13) & 0xFF for i in range(275))
    (tmp_path / "d.bin").write_bytes(data)
    out = subprocess.run([driver, "xxh32", str(tmp_path / "d.bin")], capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == len(data) + 1
    for n in range(len(data) + 1):
        assert int(out[n]) == G.xxh32(data[:n]), n


def test_legal_plans_are_accepted_by_liblz4_with_the_planned_bytes(lz4f):
    plans = [p for p in G.all_plans() if p.reason == "ok" and not p.flipped]
    assert len(plans) >= 20
    for p in plans:
        ok, out = G.lz4f_decompress(lz4f, p.data)
        assert ok and out == p.content, p.name
        assert G.decode(p.data) == p.content, p.name
        assert sum(len(f["blocks"]) for f in G.parse(p.data)) == p.blocks, p.name


def test_hostile_plans_are_refused_by_liblz4(lz4f):
    plans = [p for p in G.all_plans() if p.reason != "ok" or p.flipped]
    assert len(plans) >= 35
    differs = set()
    for p in plans:
        ok, _ = G.lz4f_decompress(lz4f, p.data)
        assert ok == p.liblz4_accepts, p.name
        if ok or p.liblz4_differs:
            assert p.liblz4_differs, p.name
            differs.add(p.reason if not p.flipped else "flipped")
    # the documented differences and no other
    assert differs == {"dict_id", "legacy_magic", "flipped"}


def test_statuses_the_plans_owe():
    by_name = {p.name: p for p in G.all_plans()}
    assert [by_name["dict_id"].status(k) for k in range(5)] == [G.NOT_SUPPORTED] * 5
    assert [by_name["legacy_magic"].status(k) for k in range(5)] == [G.NOT_SUPPORTED] * 5
    assert [by_name["flipped_block_checksum"].status(k) for k in range(5)] == [0, 0, G.BAD_CHECKSUM, G.BAD_CHECKSUM, G.BAD_CHECKSUM]
    assert [by_name["code_4"].status(k) for k in range(5)] == [0, 0, 0, 0, G.CANNOT_VERIFY]
    assert [by_name["linked_bsum_csum_size"].status(k) for k in range(5)] == [0] * 5
    assert [by_name["content_size_+1"].status(k) for k in range(5)] == [G.CANNOT_DECOMPRESS] * 5


def test_census_every_refusal_and_every_truncation_point_is_planned():
    plans = G.all_plans()
    assert len({p.name for p in plans}) == len(plans)
    reasons = {p.reason for p in plans}
    assert reasons == set(G.REASONS) - {"too_many_blocks"}, sorted(set(G.REASONS) - reasons)
    assert set(G.UNPLANNED_REASONS) == {"ok", "too_many_blocks"}
    assert {p.truncated_at for p in plans if p.truncated_at} == set(G.TRUNCATION_POINTS)
    assert {p.flipped for p in plans if p.flipped} == {"block", "content"}
    legal = [p for p in plans if p.reason == "ok" and not p.flipped]
    frames = [f for p in legal for f in G.parse(p.data)]
    assert {f["code"] for f in frames} == {4, 5, 6, 7}
    for key in ("linked", "block_sums", "content_sum"):
        assert {f[key] for f in frames} == {False, True}, key
    assert {f["content_size"] is None for f in frames} == {False, True}
    assert any(s for f in frames if f["linked"] for _, s, _ in f["blocks"]), "a stored block inside a linked frame"
    assert any(not f["blocks"] for f in frames), "an empty frame"
    assert any(len(G.parse(p.data)) >= 2 for p in legal), "frames back to back"
