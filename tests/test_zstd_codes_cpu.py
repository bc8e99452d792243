"""The format logic of the Zstandard encoder (hipcomp-core_amd/csrc/zstd_compress/zstd_codes.hpp) on the CPU.
tests/zstd_codes_driver.cpp, a scalar encoder composed of that header alone (g++, standard headers, no HIP), is built
under AddressSanitizer and UBSan and runs as a process of its own.  Every frame it makes from a planned token list is
decoded by two judges that must both return the content: the scalar decoder of tests/zstd_tables_driver.cpp and
libzstd (G.arbiter).  Planned token lists reach every form whatever a parse would do.  The kernel includes the
very same header.

What no token list reaches, and why:
  * offsets 65534 and 65535: a match of at least 3 bytes at offset d starts at position d or later and ends inside
    the chunk, so d <= 65533 in 65536 bytes; 65533 is here.
  * RLE literals with the product's block choice: literals that are all one byte make a content that is all one
    byte, which is an RLE_Block.  The driver's flag 16 takes the RLE_Block out of the choice to reach them.
  * four Huffman streams under the 3-byte header with the product's rule (one stream wherever both sizes fit 10
    bits): the driver's flag 8 asks for four streams.
  * weights whose FSE description passes 127 bytes: none was found.  A seeded search over 4000 complete sets of code
    lengths (test_weights_descriptions prints the longest, 93 bytes) stays below: a complete code of 255
    symbols and at most 11 bits has most of its symbols at the longest lengths, so its weights have little entropy.
    The refusal itself is tested with a smaller limit.
"""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import zstd_fixtures as F
import zstd_framegen as G
import zstd_seqscan as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
CXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-I", os.path.join(ROOT, "include"), "-I", CSRC]
ENC_INCLUDES = [x for d in ("zstd", "deflate", "deflate_compress") for x in ("-I", os.path.join(CSRC, d))]
CHECKSUM, GREEDY, NO_REPEAT, FOUR_STREAMS, NO_RLE_BLOCK = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("zstd_codes")
    enc, dec = str(d / "zstd_codes_driver"), str(d / "zstd_tables_driver")
    jobs = [subprocess.Popen(CXX + ENC_INCLUDES + ["-O1", os.path.join(ROOT, "tests", "zstd_codes_driver.cpp"), "-o", enc],
                             stderr=subprocess.PIPE, text=True),
            subprocess.Popen(CXX + ["-O1", os.path.join(ROOT, "tests", "zstd_tables_driver.cpp"), "-o", dec],
                             stderr=subprocess.PIPE, text=True)]
    for j in jobs:
        err = j.communicate()[1]
        assert j.returncode == 0, err
    return enc, dec


def encode_all(drivers, tmp_path, cases):
    """cases: [(content, tokens, flags)] -> [frame]"""
    blob = b"".join(struct.pack("<III", len(c), len(t), fl) + c + b"".join(struct.pack("<III", *tok) for tok in t) for c, t, fl in cases)
    (tmp_path / "enc_cases").write_bytes(blob)
    r = subprocess.run([drivers[0], "encode", str(tmp_path / "enc_cases"), str(tmp_path / "enc_res")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    res, at, out = (tmp_path / "enc_res").read_bytes(), 0, []
    for _ in cases:
        n, = struct.unpack_from("<I", res, at)
        out.append(res[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(res)
    return out


def judged(drivers, tmp_path, named, frames):
    """both judges return the content of every frame; -> the union of the frames' forms"""
    (tmp_path / "dec_cases").write_bytes(F.driver_cases([(f, len(c)) for f, (_, c, _, _) in zip(frames, named)]))
    r = subprocess.run([drivers[1], "decode", str(tmp_path / "dec_cases"), str(tmp_path / "dec_res")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got = F.driver_results((tmp_path / "dec_res").read_bytes(), len(frames))
    forms = set()
    for (name, content, _, flags), f, g in zip(named, frames, got):
        assert g == content, name
        assert 0 < len(f) <= len(content) + 14, name
        if G.libzstd() is not None:
            assert G.arbiter(f, len(content)) == content, name
        fm = G.inspect(f)
        assert ("checksum" in fm) == bool(flags & CHECKSUM), name
        if flags & CHECKSUM:
            assert f[-4:] == struct.pack("<I", G.xxh64(content) & 0xFFFFFFFF), name
        forms |= fm
    return forms


def build(tokens, lits: bytes):
    """the content that `tokens` (ll, ml, offset) and the literal bytes mean"""
    out, at = bytearray(), 0
    for ll, ml, off in tokens:
        out += lits[at:at + ll]
        at += ll
        assert 0 < off <= len(out)
        for _ in range(ml):
            out.append(out[-off])
    out += lits[at:]
    assert len(out) <= 65536, len(out)
    return bytes(out)


def text(n, seed=1):
    rnd = random.Random(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"lorem", b"ipsum", b"0123456789", b"the", b"of", b"quick", b"Zebra"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def fibonacci_literals():
    """21 byte values with Fibonacci counts (28656 literals): Huffman's own code is 20 bits deep"""
    a, b, out = 1, 1, bytearray()
    for s in range(21):
        out += bytes([65 + s]) * a
        a, b = b, a + b
    random.Random(11).shuffle(out)
    return bytes(out)


def plans():
    """[(name, content, tokens, flags)]"""
    rnd = random.Random(8878)
    out = []

    def add(name, tokens, lits, flags=0):
        out.append((name, build(tokens, lits), tokens, flags))
    noise = rnd.randbytes(70000)
    words = text(70000)
    add("empty", [], b"")
    add("empty_checksum", [], b"", CHECKSUM)
    add("one_byte", [], b"x")
    add("raw_block_random", [], noise[:5000], CHECKSUM)
    add("raw_block_tokens_do_not_pay", [(40, 4, 17)], noise[:60])
    add("rle_block", [], bytes(1000))
    add("rle_block_with_tokens", [(1, 65535, 1)], b"\x07")
    add("content_255", [(100, 55, 10)], noise[:200])
    add("content_256", [(100, 56, 10)], noise[:200], CHECKSUM)
    # literals: raw in its three headers, RLE (flag 16), Huffman in every header and stream count
    add("raw_literals_1", [(20, 100, 5)], noise[:31])
    add("raw_literals_2", [(20, 1000, 5)], noise[:4095])
    add("raw_literals_3", [(20, 1000, 5)], noise[:4096])
    add("rle_literals_1", [(2, 100, 1)], b"aaa", NO_RLE_BLOCK)
    add("rle_literals_2", [(2, 100, 1)], b"a" * 40, NO_RLE_BLOCK)
    add("rle_literals_3", [(2, 100, 1)], b"a" * 5000, NO_RLE_BLOCK)
    add("huffman_1_stream", [(5, 40, 3)], words[:600])
    add("huffman_4_streams_header_3", [(5, 40, 3)], words[:600], FOUR_STREAMS)
    add("huffman_literals_1023", [(5, 40, 3)], words[:1023])
    add("huffman_literals_1024", [(5, 40, 3)], words[:1024])
    add("huffman_literals_16383", [(5, 40, 3)], words[:16383], CHECKSUM)
    add("huffman_literals_16384", [(5, 40, 3)], words[:16384])
    add("huffman_literals_40000", [], words[:40000])
    add("huffman_low_alphabet", [(9, 30, 2)], bytes(rnd.choice(b"\x00\x00\x00\x01\x01\x02\x03") for _ in range(3000)))
    add("huffman_fibonacci_counts", [(3, 50, 2)], fibonacci_literals())
    skew = bytes(min(255, int(rnd.expovariate(0.03))) for _ in range(30000))
    add("huffman_256_values", [], bytes(range(256)) + skew)
    add("uniform_256_values_stay_raw", [(256, 4000, 256)], bytes(range(256)) * 4)
    # sequences: counts, modes, lengths
    add("one_sequence", [(5, 10, 4)], words[:50])
    seqs = lambda n, f: [f(k) for k in range(n)]
    add("sequences_127", seqs(127, lambda k: (3, 4 + k % 9, 1 + k % 3)), words[:127 * 3 + 9])
    add("sequences_128", seqs(128, lambda k: (3, 4 + k % 9, 1 + k % 3)), words[:128 * 3 + 9], CHECKSUM)
    add("all_rle_modes", seqs(300, lambda k: (2, 7, 2 + k % 2)), words[:700])   # (offsets 2 and 3 share a code)
    add("all_predefined_modes", [(2, 3, 1), (1, 5, 2), (3, 4, 9)], b"ab" + words[:40])   # (too few for a description to pay)
    add("all_fse_modes", seqs(3000, lambda k: ((k * 7) % 3 + (17 if k % 50 == 0 else 0), 3 + (k * k) % 5 + (40 if k % 64 == 0 else 0), 1 + k % 2 + (300 if k % 90 == 89 else 0))),
        words[:9000])
    add("wide_fse_tables", seqs(1000, lambda k: (rnd.randrange(0, 40) if k % 3 or k == 0 else 0, rnd.choice((3, 4, 5, 9, 17, 33, 40, 70, 130)), 1 + rnd.randrange(0, 1 << rnd.randrange(1, 9)) if k > 100 else 1)),
        words[:20000])
    add("match_of_65532", [(4, 65532, 3)], b"abcd")
    add("literal_run_of_65532", [(65532, 4, 65532)], noise[:65532])
    add("offset_65533", [(65533, 3, 65533)], words[:65533])
    add("long_match_and_long_run", [(3, 30000, 2), (30000, 3000, 29000)], noise[:30003])
    # repeat offsets
    add("same_offset_without_literals", [(5, 4, 5), (0, 6, 5), (2, 4, 5)], words[100:140])
    add("same_offset_behind_one_literal", [(5, 4, 5), (3, 4, 3), (1, 6, 3), (1, 5, 5)], words[200:240])
    add("repeat_codes_off", [(5, 4, 5), (3, 4, 3), (1, 6, 3), (1, 5, 5)], words[200:240], NO_REPEAT)
    return out


def greedy_plans():
    rnd = random.Random(7)
    t = text(65536, 5)
    ints = np.sort(np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, 16384)).astype("<i4").tobytes()
    datas = [t, t[:1000], t[:70], ints, rnd.randbytes(3000), bytes(500), b"ab" * 700, (rnd.randbytes(255) * 300)[:65536],
             (np.arange(16384, dtype=np.int32) // 3 * 1000).astype("<i4").tobytes(), b"abc", b""]
    return [(f"greedy_{i}", d, [], GREEDY | (CHECKSUM if i % 2 else 0)) for i, d in enumerate(datas)]


def test_planned_token_lists_reach_every_form(drivers, tmp_path):
    named = plans()
    frames = encode_all(drivers, tmp_path, [(c, t, fl) for _, c, t, fl in named])
    forms = judged(drivers, tmp_path, named, frames)
    print(sorted(forms))
    want = {"raw_block", "rle_block", "compressed_block", "raw_literals_1", "raw_literals_2", "raw_literals_3",
            "rle_literals_1", "rle_literals_2", "rle_literals_3", "huffman_literals_1_stream_3", "huffman_literals_4_stream_3",
            "huffman_literals_4_stream_4", "huffman_literals_4_stream_5", "weights_direct", "weights_fse",
            "seq_count_0", "seq_count_1", "seq_count_2", "checksum", "fcs_1", "fcs_2", "single_segment"}
    want |= {f"{t}_{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse")}
    assert want <= forms, want - forms
    assert not forms & {"ll_repeat", "of_repeat", "ml_repeat", "seq_count_3", "window_descriptor", "fcs_0", "fcs_4", "fcs_8",
                        "treeless_literals_1_stream_3", "treeless_literals_4_stream_3"}
    by = {n: (c, f) for (n, c, _, _), f in zip(named, frames)}
    form = lambda n: G.inspect(by[n][1])
    # block choice
    assert by["empty"][1] == bytes.fromhex("28b52ffd2000010000")
    if G.libzstd() is not None:
        assert by["empty"][1] == G.compress(b"", 3)
    assert len(by["empty_checksum"][1]) == 13 and len(by["one_byte"][1]) == 10
    assert "raw_block" in form("raw_block_tokens_do_not_pay") and "raw_block" in form("raw_block_random")
    assert "rle_block" in form("rle_block_with_tokens") and len(by["rle_block_with_tokens"][1]) == 11
    assert "fcs_1" in form("content_255") and "fcs_2" in form("content_256")
    assert len(by["content_255"][0]) == 255 and len(by["content_256"][0]) == 256
    # literals
    assert "huffman_literals_1_stream_3" in form("huffman_literals_1023")
    assert "huffman_literals_4_stream_4" in form("huffman_literals_1024") and "huffman_literals_4_stream_4" in form("huffman_literals_16383")
    assert "huffman_literals_4_stream_5" in form("huffman_literals_16384")
    assert "weights_direct" in form("huffman_low_alphabet") and "weights_fse" in form("huffman_256_values")
    assert max(G.huf_lengths(fibonacci_literals(), 32).values()) > 11 and "huffman_literals_4_stream_5" in form("huffman_fibonacci_counts")
    assert any(f.startswith("raw_literals") for f in form("uniform_256_values_stay_raw"))   # no description of its tree fits
    # sequences
    assert "seq_count_1" in form("sequences_127") and "seq_count_2" in form("sequences_128")
    assert {"ll_rle", "of_rle", "ml_rle"} <= form("all_rle_modes")
    assert {"ll_predefined", "of_predefined", "ml_predefined"} <= form("all_predefined_modes")
    assert {"ll_fse", "of_fse", "ml_fse"} <= form("all_fse_modes")
    for (name, content, tokens, flags), f in zip(named, frames):
        seqs = S.sequences_of(f)
        if seqs is not None:
            assert [(ll, ml) for ll, ml, _ in seqs] == [(ll, ml) for ll, ml, _ in tokens], name
    assert S.sequences_of(by["match_of_65532"][1]) == [(4, 65532, 6)]
    assert S.sequences_of(by["literal_run_of_65532"][1]) is None or S.sequences_of(by["literal_run_of_65532"][1]) == [(65532, 4, 65535)]
    assert S.sequences_of(by["offset_65533"][1]) == [(65533, 3, 65536)]
    # repeat offsets: never without literals, always behind them, and always the offset of the sequence just before
    assert [ov for _, _, ov in S.sequences_of(by["same_offset_without_literals"][1])] == [8, 8, 1]
    assert [ov for _, _, ov in S.sequences_of(by["same_offset_behind_one_literal"][1])] == [8, 6, 1, 8]
    assert [ov for _, _, ov in S.sequences_of(by["repeat_codes_off"][1])] == [8, 6, 6, 8]
    assert len(by["same_offset_behind_one_literal"][1]) <= len(by["repeat_codes_off"][1])


def test_the_drivers_own_parse_round_trips(drivers, tmp_path):
    named = greedy_plans()
    frames = encode_all(drivers, tmp_path, [(c, t, fl) for _, c, t, fl in named])
    forms = judged(drivers, tmp_path, named, frames)
    assert {"compressed_block", "raw_block", "rle_block"} <= forms
    # repeat codes pay on the column whose values stand three times
    i = 8
    off = encode_all(drivers, tmp_path, [(named[i][1], [], GREEDY | NO_REPEAT)])[0]
    assert G.arbiter(off, 65536) in (None, named[i][1]) and len(frames[i]) < len(off)
    assert sum(1 for _, _, ov in S.sequences_of(frames[i]) if ov == 1) > 0


def histograms(kind, count, seed):
    """seeded histograms of `count` draws each: [(total, [64 counts])]"""
    rng = np.random.default_rng(seed)
    nsym = (36, 32, 53, 13)[kind]
    out = []
    for k in range(count):
        used = int(rng.integers(2, nsym + 1))
        syms = rng.choice(nsym, used, replace=False)
        total = int(rng.integers(used, 255 if kind == 3 else 16385))
        if k % 3 == 0:
            w = rng.random(used) ** 6     # skewed
        elif k % 3 == 1:
            w = np.ones(used)
        else:
            w = rng.random(used)
        h = np.ones(used, dtype=np.int64) + rng.multinomial(total - used, w / w.sum())
        hist = [0] * 64
        for s, c in zip(syms.tolist(), h.tolist()):
            hist[s] = c
        out.append((total, hist))
    return out


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_normalisation_and_table_description(drivers, tmp_path, kind):
    """2000 seeded histograms per table kind: the normalised counts sum to 2^log with every used symbol >= 1, the
    description is G.write_ncount's, and read_ncount (the decoder's) returns the counts from it"""
    hs = histograms(kind, 2000, 100 + kind)
    (tmp_path / "t_cases").write_bytes(b"".join(struct.pack("<II64I", kind, total, *hist) for total, hist in hs))
    r = subprocess.run([drivers[0], "tables", str(tmp_path / "t_cases"), str(tmp_path / "t_res")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res, at = (tmp_path / "t_res").read_bytes(), 0
    lo, hi = 5, (9, 8, 9, 6)[kind]
    logs = set()
    for total, hist in hs:
        log, nbytes, ok = struct.unpack_from("<III", res, at)
        norm = list(struct.unpack_from("<64h", res, at + 12))
        back = list(struct.unpack_from("<64h", res, at + 12 + 128))
        desc = res[at + 12 + 256:at + 12 + 256 + nbytes]
        at += 12 + 256 + nbytes
        assert ok == 1 and lo <= log <= hi
        assert sum(norm) == 1 << log
        assert all((c >= 1) == (h > 0) for c, h in zip(norm, hist))
        last = max(s for s, c in enumerate(norm) if c)
        assert back[:last + 1] == norm[:last + 1] and not any(back[last + 1:])
        assert desc == G.write_ncount(norm[:last + 1], log)
        logs.add(log)
    assert at == len(res)
    assert len(logs) >= 2


def log2_fix8(x: int) -> int:
    h = x.bit_length() - 1
    m = (x << 16) >> h
    r = h << 8
    for b in range(7, -1, -1):
        m = (m * m) >> 16
        if m >= 2 << 16:
            m >>= 1
            r |= 1 << b
    return r


def test_cost_estimate(drivers):
    for x in (1, 2, 3, 5, 7, 64, 100, 511, 512):
        got = int(subprocess.run([drivers[0], "log2", str(x)], capture_output=True, text=True, check=True).stdout)
        assert got == log2_fix8(x) and abs(got / 256 - np.log2(x)) < 1 / 128
    norm, log = G.LL_DEFAULT
    want = sum((s + 1) * ((log << 8) - log2_fix8(abs(c))) for s, c in enumerate(norm))
    assert int(subprocess.run([drivers[0], "cost"], capture_output=True, text=True, check=True).stdout) == want


def temp_bytes(chunks: int, max_chunk: int) -> int:
    waves = min(chunks, 256 * 12)
    return waves * (8 * ((max_chunk // 4 + 64) // 64 * 64) + (max_chunk + 256) // 256 * 256)


def test_temp_size_formula(drivers):
    for chunks, mx in ((0, 65536), (1, 0), (1, 1), (7, 1000), (3072, 65536), (3073, 65536), (100000, 65535), (5, 4095)):
        got = int(subprocess.run([drivers[0], "tempsize", str(chunks), str(mx)], capture_output=True, text=True, check=True).stdout)
        assert got == temp_bytes(chunks, mx), (chunks, mx)


def complete_lengths(rng, nsym):
    """a complete prefix code of nsym symbols, at most 11 bits: splits of random leaves"""
    lens = [1, 1]
    while len(lens) < nsym:
        can = [i for i, l in enumerate(lens) if l < 11]
        i = can[int(rng.integers(len(can)))] if rng.random() < 0.7 else min(can, key=lambda j: lens[j])
        lens[i] += 1
        lens.append(lens[i])
    return lens


def test_weights_descriptions(drivers, tmp_path):
    """the two descriptions' sizes over 4000 seeded complete codes: direct only up to symbol 127, the FSE one never
    near 127 bytes; with the limit lowered to 24 bytes the FSE description is refused wherever it is longer"""
    rng = np.random.default_rng(12)
    sets = []
    for k in range(4000):
        nsym = int(rng.integers(2, 257))
        lens = complete_lengths(rng, nsym)
        rng.shuffle(lens)
        where = np.sort(rng.choice(256, nsym, replace=False)) if k % 2 else np.arange(nsym)
        full = [0] * 256
        for s, l in zip(where.tolist(), lens):
            full[s] = l
        sets.append(full)
    (tmp_path / "w_cases").write_bytes(b"".join(bytes(s) for s in sets))
    sizes = {}
    for limit in (127, 24):
        r = subprocess.run([drivers[0], "weights", str(limit), str(tmp_path / "w_cases"), str(tmp_path / "w_res")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        sizes[limit] = list(struct.iter_unpack("<II", (tmp_path / "w_res").read_bytes()))
    longest = max(f for _, f in sizes[127])
    print("longest FSE-compressed weights description: %d bytes" % longest)
    assert 24 < longest <= 127
    for full, (direct, fse), (_, short) in zip(sets, sizes[127], sizes[24]):
        last = max(s for s, l in enumerate(full) if l)
        assert direct == (1 + (last + 1) // 2 if 1 <= last <= 127 else 0)
        assert short == (fse if fse - 1 <= 24 else 0)
        distinct = len({l for l in full[:last] if l} | ({0} if 0 in full[:last] else set()))
        assert (fse == 0) == (last < 2 or distinct < 2), (last, distinct)
