"""The format logic of the Zstandard decoder (hipcomp-core_amd/csrc/zstd/zstd_tables.hpp, xxh64_math.hpp) on the
CPU, against libzstd.  tests/zstd_tables_driver.cpp, a scalar frame decoder composed of those headers alone (g++,
standard headers, no HIP), is built under AddressSanitizer and UBSan and runs as a process of its own: every chunk
is decoded from a heap buffer of exactly its length into one of exactly its capacity, so a read or a write outside
either ends the driver.  The kernel includes the very same headers."""
import os
import subprocess

import numpy as np
import pytest

import zstd_fixtures as F
import zstd_framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
CXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-I", os.path.join(ROOT, "include"), "-I", CSRC]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zstd_tables") / "zstd_tables_driver")
    r = subprocess.run(CXX + ["-O1", os.path.join(ROOT, "tests", "zstd_tables_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def decode_all(driver, tmp_path, cases, mode="decode"):
    """cases: [(chunk, capacity)] -> [content or None] (decode) or [size] (sizes)"""
    (tmp_path / "cases").write_bytes(F.driver_cases(cases))
    r = subprocess.run([driver, mode, str(tmp_path / "cases"), str(tmp_path / "res")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    blob = (tmp_path / "res").read_bytes()
    if mode == "sizes":
        return np.frombuffer(blob, dtype=np.uint64).tolist()
    return F.driver_results(blob, len(cases))


def libzstd_required():
    assert G.libzstd() is not None, "libzstd.so.1 does not load: it is the arbiter of these tests"


def test_every_legal_frame_decodes_to_its_bytes(driver, tmp_path):
    libzstd_required()
    cases = [(n, c, d) for n, c, d, _ in G.legal_plans()] + F.load()[0]
    for slack in (0, 100):
        got = decode_all(driver, tmp_path, [(c, len(d) + slack) for _, c, d in cases])
        for (name, chunk, want), g in zip(cases, got):
            assert g == want == G.arbiter(chunk, len(want) + slack), name
    short = [(n, c, d) for n, c, d in cases if d]
    got = decode_all(driver, tmp_path, [(c, len(d) - 1) for _, c, d in short])
    for (name, chunk, want), g in zip(short, got):
        assert g is None and G.arbiter(chunk, len(want) - 1) is None, name
    sizes = decode_all(driver, tmp_path, [(c, 0) for _, c, d in cases], mode="sizes")
    assert sizes == [len(d) for _, _, d in cases]


def test_every_illegal_planned_frame_is_refused(driver, tmp_path):
    libzstd_required()
    plans = G.illegal_plans()
    got = decode_all(driver, tmp_path, [(c, 1 << 17) for _, c in plans])
    for (name, chunk), g in zip(plans, got):
        assert g is None and G.arbiter(chunk, 1 << 17) is None, name


def test_documented_difference_sequences_bitstream_not_exactly_consumed(driver, tmp_path):
    """include/hipcomp/zstd.h, documented difference 1: libzstd 1.4.8 accepts bits that no sequence reads."""
    libzstd_required()
    (name, chunk), = [p for p in G.documented_differences() if p[0] == "sequences_bitstream_not_exactly_consumed"]
    assert G.arbiter(chunk, 1 << 17) is not None
    assert decode_all(driver, tmp_path, [(chunk, 1 << 17)]) == [None]


def test_documented_difference_fse_weights_shorter_than_their_initial_states(driver, tmp_path):
    """include/hipcomp/zstd.h, documented difference 2"""
    libzstd_required()
    (name, chunk), = [p for p in G.documented_differences() if p[0] == "fse_weights_shorter_than_their_initial_states"]
    assert G.arbiter(chunk, 1 << 17) is not None
    assert decode_all(driver, tmp_path, [(chunk, 1 << 17)]) == [None]


def test_documented_difference_huffman_stream_read_past_its_start_by_its_last_symbol(driver, tmp_path):
    """include/hipcomp/zstd.h, documented difference 3.  tests/golden/zstd/huffman_last_symbol.zst is a libzstd
    level-19 frame of 40000 skewed bytes with bit 5 of byte 346, inside its first Huffman stream, flipped: libzstd
    1.4.8 decodes 40000 (other) bytes from it, the exact walk finds a stream that is not consumed to its first bit."""
    libzstd_required()
    with open(os.path.join(F.DIR, "huffman_last_symbol.zst"), "rb") as f:
        chunk = f.read()
    cuts, heads = F.boundaries(chunk[:346] + bytes([chunk[346] ^ 0x20]) + chunk[347:])   # (the frame before the flip)
    lit, seq = [at for k, at in heads if k == "literals"][0], [at for k, at in heads if k == "sequences"][0]
    assert lit < 346 < seq
    got = G.arbiter(chunk, 40000)
    assert got is not None and len(got) == 40000
    assert decode_all(driver, tmp_path, [(chunk, 40000)]) == [None]


def test_no_legal_frame_falls_under_a_documented_difference(driver, tmp_path):
    """every frame libzstd makes itself and every legal plan decodes: the differences take nothing legal away"""
    libzstd_required()
    cases = [(c, len(d)) for _, c, d, _ in G.legal_plans()] + [(c, len(d)) for _, c, d in F.load()[0]]
    assert all(g is not None for g in decode_all(driver, tmp_path, cases))


def test_documented_difference_sequences_bitstream_read_past_its_start(driver, tmp_path):
    """include/hipcomp/zstd.h, documented difference 1, the other way round: the walk runs out of bits."""
    libzstd_required()
    frames = F.load()[0]
    good = next(c for n, c, _ in frames if n == "text_level_3")
    cuts, heads = F.boundaries(good)
    first_sequences = [at for k, at in heads if k == "sequences"][0]
    assert first_sequences < G.OVERREAD_AT < min(c for c in cuts if c > first_sequences)   # in the first block's sequences
    chunk, cap = G.libzstd_frame_with_overread(frames)
    assert G.arbiter(chunk, cap) is not None
    assert decode_all(driver, tmp_path, [(chunk, cap)]) == [None]


def test_damaged_fixture_is_what_libzstd_says_now(driver, tmp_path):
    """the fixture is recomputed where libzstd loads, and the scalar decoder is held to it"""
    libzstd_required()
    frames, damaged = F.load()
    index, blob = F.make()
    again = [(e[0], e[2], e[3], e[4]) for e in index["damaged"]]
    assert again == [(k, cap, size, md5) for k, _, cap, size, md5 in damaged]
    assert [(f"{e['input']}_level_{e['level']}", blob[e["at"][0]:e["at"][0] + e["at"][1]]) for e in index["frames"]] == \
        [(n, c) for n, c, _ in frames]
    got = decode_all(driver, tmp_path, [(c, cap) for _, c, cap, _, _ in damaged])
    import hashlib
    for (kind, chunk, cap, size, md5), g in zip(damaged, got):
        assert (None if g is None else (len(g), hashlib.md5(g).hexdigest())) == (None if size is None else (size, md5)), kind


def test_every_prefix_of_small_frames(driver, tmp_path):
    libzstd_required()
    for name in ("three_blocks_repeat_mode", "checksum", "skippable_everywhere"):
        (chunk, content), = [(c, d) for n, c, d, _ in G.legal_plans() if n == name]
        cases = [(chunk[:k], len(content)) for k in range(len(chunk) + 1)]
        got = decode_all(driver, tmp_path, cases)
        for (c, cap), g in zip(cases, got):
            assert g == G.arbiter(c, cap), (name, len(c))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 4096 + 5, 100003])
def test_xxh64(driver, tmp_path, n):
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    (tmp_path / "d").write_bytes(data)
    r = subprocess.run([driver, "xxh64", str(tmp_path / "d")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout, 16) == G.xxh64(data)
    if n == 0:
        assert G.xxh64(b"") == 0xEF46DB3751D8E999     # the published value for the empty input, seed 0


def test_temp_size_formula(driver):
    def restated(chunks, max_chunk, waves):
        per_wave = -(-min(max_chunk, 128 * 1024) // 256) * 256
        return min(chunks, waves) * per_wave
    for chunks in (0, 1, 5, 3071, 3072, 3073, 100000):
        for max_chunk in (0, 1, 255, 256, 257, 65536, 128 * 1024, 128 * 1024 + 1, 300 * 1024):
            r = subprocess.run([driver, "tempsize", str(chunks), str(max_chunk), "3072"], capture_output=True, text=True)
            assert int(r.stdout) == restated(chunks, max_chunk, 3072), (chunks, max_chunk)
