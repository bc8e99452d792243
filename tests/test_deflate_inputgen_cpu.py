"""The planned inputs of tests/deflate_inputgen.py and the stream scanner of tests/deflate_tokenscan.py on the CPU.

The scanner is held to zlib: on zlib's own streams and on deflate_streamgen's legal plans its expansion is
zlib.decompressobj(-15)'s, and where a plan's tokens are known its tokens are the plan's.  The mirror of the parse
rule returns every plan, and the records follow from the tokens.  tests/deflate_codes_driver.cpp's `encode` -- the
shipped deflate_codes.hpp, nothing else -- writes every planned chunk: zlib returns the chunk, the scanner reads the
planned tokens and the chosen kind back, the bits written are the chosen cost and the chosen cost is the smallest,
a tie going to the simpler kind.  A census asserts one by one that the inputs meet the edges they were planned for.
The driver runs once more under AddressSanitizer and UBSan, a process of its own.
tests/test_deflate_encoder_edges_gpu.py gives the same cases to the kernel.  The Zstandard cases, whose mirror this
module's shares, are unchanged: their count and a digest of their contents are asserted here."""
import hashlib
import os
import subprocess
import zlib

import pytest

import deflate_inputgen as D
import deflate_streamgen as G
import deflate_tokenscan as S
import zstd_inputgen as Z
from test_deflate_codes_cpu import CSRC, TESTS, huffman

ZSTD_CASES = (311, "f648e671fcf313c484ea7ea0bed146cd69c2f8bc4c86455de221a83b4ea00d5c")


def build_driver(directory, sanitize=False):
    exe = os.path.join(str(directory), "deflate_codes_driver" + ("_san" if sanitize else ""))
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1"] + flags + ["-I", CSRC, "-I", os.path.join(CSRC, "deflate"),
                        os.path.join(TESTS, "deflate_codes_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def encode_all(exe, directory, jobs):
    """jobs [(content, tokens)] -> [(stream, kind, bits written, dynamic, fixed, stored cost)] in one process"""
    lines = []
    for k, (content, tokens) in enumerate(jobs):
        path = os.path.join(str(directory), f"{k}.job")
        with open(path, "wb") as f:
            f.write(D.job_file(content, tokens))
        lines.append("encode @" + path)
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) == 5:          # (an empty stream cannot happen, but an empty hex field would shift the others)
            f.insert(0, "")
        out.append((bytes.fromhex(f[0]),) + tuple(int(x) for x in f[1:]))
    assert len(out) == len(jobs)
    return out


def inflate(stream):
    d = zlib.decompressobj(-15)
    got = d.decompress(stream)
    return got, d.eof, d.unused_data


def simplest_smallest(stored, fixed, dynamic):
    """the rule of DESIGN.md section 14: the smallest, a tie to the simpler kind"""
    least = min(stored, fixed, dynamic)
    return S.STORED if stored == least else S.FIXED if fixed == least else S.DYNAMIC


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("deflate_driver"))


@pytest.fixture(scope="module")
def planned(driver, tmp_path_factory):
    """-> (the cases that have tokens, the driver's output for each, its scan)"""
    cases = [c for c in D.all_cases() if c.tokens is not None]
    outs = encode_all(driver, tmp_path_factory.mktemp("planned"), [(c.content, c.tokens) for c in cases])
    return cases, outs, [S.scan(o[0]) for o in outs]


# ------------------------------------------------------------------------------------------------------ the scanner
def zlib_streams():
    text = G._text(20000, 3)
    data = {"text": text, "runs": b"ab" * 700 + bytes(900) + text[:300] * 3, "empty": b"", "one": b"x", "noise": bytes((i * 197 + (i >> 3) * 31) & 0xFF for i in range(3000))}
    out = []
    for name, d in data.items():
        for label, level, strategy in (("1", 1, zlib.Z_DEFAULT_STRATEGY), ("6", 6, zlib.Z_DEFAULT_STRATEGY), ("9", 9, zlib.Z_DEFAULT_STRATEGY),
                                       ("fixed", 6, zlib.Z_FIXED), ("0", 0, zlib.Z_DEFAULT_STRATEGY)):
            z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
            out.append((f"{name}_level_{label}", z.compress(d) + z.flush(), d))
    return out


def test_the_scanner_expands_what_zlib_expands():
    kinds = set()
    for name, stream, want in zlib_streams() + G.legal_plans():
        got, eof, unused = inflate(stream)
        assert eof and got == want, name
        s = S.scan(stream)
        assert s.output == got, name
        assert s.unused == unused or len(s.unused) >= len(unused), name
        assert (s.total_bits + 7) // 8 == len(stream) - len(unused), name
        assert sum(ll + ml for ll, ml, _ in s.tokens) + s.tail == len(got), name
        assert len(s.ranges) == len(s.tokens) and all(a <= m < e <= s.total_bits for a, m, e in s.ranges), name
        kinds |= {b.kind for b in s.blocks}
        assert s.blocks[-1].final and not any(b.final for b in s.blocks[:-1]), name
    assert kinds == {S.STORED, S.FIXED, S.DYNAMIC}


def test_the_scanner_reads_the_tokens_of_a_plan():
    """streams written by deflate_streamgen from token lists of this test: the matches come back one for one"""
    text = list(G._text(300))
    plans = {
        "every_length": text + [t for n in range(3, 259) for t in (("m", n, 1 + n % 200), 65 + n % 26)],
        "every_distance_class": list(G._text(32768, 3)) + [t for s in range(30) for d in (G.DIST_BASE[s], G.DIST_BASE[s] + (1 << G.DIST_EXTRA[s]) - 1)
                                                        for t in (("m", 3 + s, d), 48 + s)],
        "back_to_back": text + [("m", 258, 7), ("m", 258, 7), ("m", 4, 7), ("m", 3, 300)],
    }
    for name, toks in plans.items():
        for blk in (G.fixed_block, G.dynamic_block):
            w = G.BitWriter()
            blk(w, toks, True)
            bits = 8 * len(w.out) + w.bit_offset
            s = S.scan(w.done())
            want, run = [], 0
            for t in toks:
                if isinstance(t, int):
                    run += 1
                else:
                    want.append((run, t[1], t[2]))
                    run = 0
            assert s.tokens == want and s.tail == run, name
            assert s.total_bits == bits and s.output == G.expand(toks), name
            # a token's bits: its literals' codes and its match's; together with the header and the end of block, the stream
            assert all(a == (s.ranges[k - 1][2] if k else a) for k, (a, _, _) in enumerate(s.ranges)), name
            if blk is G.dynamic_block:
                b = s.blocks[0]
                assert b.kind == S.DYNAMIC and len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist and b.cl_symbols


# ------------------------------------------------------------------------------------------------------ the mirror
def test_the_zstandard_cases_are_unchanged():
    cases = Z.all_cases()
    h = hashlib.sha256()
    for c in cases:
        h.update(repr((c.name, c.content, c.tokens, sorted(c.copies.items()), sorted(c.tags.items()), c.scalar_only)).encode())
    assert (len(cases), h.hexdigest()) == ZSTD_CASES


def test_the_mirror_returns_every_plan():
    cases = D.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    planned, total = 0, 0
    for c in cases:
        assert len(c.content) <= D.MAX_CHUNK, c.name
        total += len(c.content)
        if c.family == "generic":
            continue
        assert c.tokens is not None, c.name                   # no planned case is left out
        planned += 1
        tokens, recs = D.mirror(c.content, c.copies)          # (raises PlanError where a lookup that matters is ambiguous)
        assert tokens == c.tokens, c.name
        assert D.rebuilds(c.content, c.tokens) and D.maximal(c.content, c.tokens), c.name
        assert all(D.MIN_MATCH <= ml <= D.MAX_MATCH and 1 <= d <= D.MAX_DISTANCE for _, ml, d in c.tokens), c.name
        assert not c.copies or sorted(c.copies) == Z.copy_positions(c.tokens), c.name
    print("%d cases, %d of them planned, %d bytes" % (len(cases), planned, total))
    assert planned >= 150
    again = D.FAMILIES["trip_edges"]()
    assert [(c.name, c.content, c.tokens) for c in again] == [(c.name, c.content, c.tokens) for c in D.family("trip_edges")]


def test_the_records_follow_from_the_tokens():
    for c in D.all_cases():
        if c.tokens is None:
            continue
        recs = D.records(c.tokens, len(c.content))
        assert D.tokens_of(recs) == (c.tokens, len(c.content) - sum(ll + ml for ll, ml, _ in c.tokens)), c.name
        assert all(ll <= 191 or (ll, ml) == (192, 0) for ll, ml, _ in recs), c.name
        assert recs[-1][1] == 0 and all(w < 1 << 32 for w in D.record_words(recs)), c.name
        assert len(recs) <= len(c.content) // 4 + 2, c.name          # the room a wave's buffer has
    # the rule trip by trip, on one case with long runs: the pending run after every trip without a hit
    c = {x.name: x for x in D.all_cases()}["runs/ll400"]
    recs, pos, pend = [], 0, 0
    for ll, ml, d in c.tokens + [(len(c.content) - sum(a + b for a, b, _ in c.tokens), 0, 1)]:
        left = ll
        while left >= 64 or (ml == 0 and left > 0):
            t = min(left, 64)
            pend, left = pend + t, left - t
            if pend > 191:
                recs.append((pend, 0, 0))
                pend = 0
        recs.append((pend + left, ml, d - 1))
        pend = 0
    assert recs == D.records(c.tokens, len(c.content))


def test_the_mirror_knows_the_two_limits():
    by = {c.name: c for c in D.family("distances")}
    c = by["dist/source0_at32768"]
    assert Z.parse(c.content, None, D.MAX_MATCH, 32768) == [(32768, 6, 32768)]
    assert Z.parse(c.content, None, D.MAX_MATCH, 32767) == []            # one further back than the limit: no hit
    assert Z.parse(by["dist/source0_at32769"].content, None, D.MAX_MATCH, 32769) == [(32769, 6, 32769)]
    c = {c.name: c for c in D.family("match_extension")}["extend/repeat600"]
    assert [ml for _, ml, _ in Z.parse(c.content, None, 258, None)[1:]] == [258, 258, 84]
    assert [ml for _, ml, _ in Z.parse(c.content, None, 196, None)[1:3]] == [196, 196]
    assert [ml for _, ml, _ in Z.parse(c.content)[1:]] == [600]          # Zstandard's form of the rule: no limit


# ------------------------------------------------------------------------------------------------------ the driver
def test_the_driver_writes_every_plan(planned):
    cases, outs, scans = planned
    for c, (stream, kind, bits, dyn, fixed, stored), s in zip(cases, outs, scans):
        got, eof, unused = inflate(stream)
        assert eof and unused == b"" and got == c.content, c.name
        assert [b.kind for b in s.blocks] == [kind] * len(s.blocks) and s.output == c.content, c.name
        assert stored == 8 * (len(c.content) + 5 * max(1, -(-len(c.content) // 65535))), c.name
        assert kind == simplest_smallest(stored, fixed, dyn), (c.name, stored, fixed, dyn)
        assert bits == (stored, fixed, dyn)[kind] == s.total_bits and len(stream) == (bits + 7) // 8, c.name
        if kind == S.STORED:
            assert s.tokens == [] and s.tail == len(c.content) and len(s.blocks) == max(1, -(-len(c.content) // 65535)), c.name
        else:
            assert len(s.blocks) == 1 and s.tokens == c.tokens, c.name


def test_census(planned):
    cases, outs, scans = planned
    by = {c.name: (c, o, s) for c, o, s in zip(cases, outs, scans)}
    plans = [c for c in cases if c.family != "generic"]
    # trips
    for k in (0, 1, 62, 63):
        assert by[f"trip/hit_lane{k}"][0].tokens[1][0] % 64 == k
    assert len(by["trip/source_in_the_same_trip"][0].tokens) == 1
    c = by["trip/source_in_the_trip_before"][0]
    assert c.tokens[1][2] == 3 + 4 and c.tokens[1][0] % 64 == 3          # lane 60 of the trip before, found on lane 3
    assert by["trip/position0_of_an_empty_slot"][0].tokens == [(4, 8, 4)]
    for t in (1, 2, 3):
        c = by[f"trip/tail{t}"][0]
        assert len(c.content) - sum(ll + ml for ll, ml, _ in c.tokens) == t
    c = by["trip/match_at_len_minus_4"][0]
    assert c.tokens[-1][1] == 4 and Z.copy_positions(c.tokens)[-1] == len(c.content) - 4
    assert [len(by[f"trip/len{n}"][0].content) for n in range(6)] == list(range(6))
    # match extension
    for L in D.MATCH_LENGTHS:
        for how in ("byte", "end"):
            c = by[f"extend/L{L}_{how}"][0]
            end = sum(ll + ml for ll, ml, _ in c.tokens)
            assert c.tokens[-1][1] == L and (end < len(c.content)) == (how == "byte"), c.name
    t = by["extend/repeat600"][0].tokens[1:]
    assert [ml for _, ml, _ in t] == [258, 258, 84] and [ll for ll, _, _ in t[1:]] == [0, 0] and len({d for _, _, d in t}) == 1
    t = by["extend/repeat262"][0].tokens[1:]
    assert [ml for _, ml, _ in t] == [258, 4] and t[1][0] == 0 and t[0][2] == t[1][2]
    assert [ml for _, ml, _ in by["extend/repeat259"][0].tokens[1:]] == [258]      # and the 259th byte is a literal
    for d in (1, 2, 3):
        for L in (4, 70, 258):
            assert by[f"extend/distance{d}_L{L}"][0].tokens[-1][1:] == (L, d)
    # distances
    found = {d for c in plans if c.family == "dist" for _, _, d in c.tokens}
    assert set(D.DISTANCES) <= found and {1, 4, 5, 32767, 32768} <= set(D.DISTANCES) and max(found) == 32768
    for s in D.EDGE_CLASSES:
        assert {G.DIST_BASE[s], G.DIST_BASE[s] + (1 << G.DIST_EXTRA[s]) - 1} <= found
    assert len(by["dist/d32769_not_found"][0].tokens) == 1 and len(by["dist/d32769_not_found"][0].content) > 32769 + 100
    assert by["dist/source0_at32768"][0].tokens == [(32768, 6, 32768)] and by["dist/source0_at32769"][0].tokens == []
    # literal runs and records
    recs = {c.name: D.records(c.tokens, len(c.content)) for c in plans}
    for ll in (0, 1, 63, 64, 65, 127, 128, 191):
        assert recs[f"runs/ll{ll}"][2] == (ll, 7, recs[f"runs/ll{ll}"][2][2]), ll
    assert recs["runs/ll192"][2:4] == [(192, 0, 0), (0, 7, recs["runs/ll192"][3][2])]
    assert recs["runs/tail0"][-1] == (0, 0, 0) and recs["runs/tail0"][-2][1] == 7
    assert recs["runs/tail192"][-2:] == [(192, 0, 0), (0, 0, 0)] and recs["runs/tail191"][-1] == (191, 0, 0)
    for n in D.RECORD_COUNTS:
        assert len(recs[f"counts/records{n}"]) == n
    c = by["counts/max_records"][0]
    assert len(recs[c.name]) >= 0.95 * len(c.content) / 4 and 15000 <= len(c.content) <= 17000
    assert sum(1 for ll, ml, _ in c.tokens if (ll, ml) == (0, 4)) >= len(c.tokens) - 1
    # alphabets
    c, o, s = by["alpha/no_match_dynamic"]
    assert o[1] == S.DYNAMIC and s.blocks[0].hdist == 1 and s.blocks[0].dist_lens == [0]
    c, o, s = by["alpha/one_distance_code"]
    assert o[1] == S.DYNAMIC and sum(1 for l in s.blocks[0].dist_lens if l) == 1
    c, o, s = by["alpha/hlit286"]
    assert o[1] == S.DYNAMIC and s.blocks[0].hlit == 286 and any(ml == 258 for _, ml, _ in c.tokens)
    assert any(o[1] == S.DYNAMIC and s.blocks[0].hdist == 30 for c, o, s in by.values())
    c, o, s = by["alpha/all_literals_of_one_frequency"]
    assert o[1] == S.DYNAMIC and c.tokens == [] and {c.content.count(bytes([v])) for v in set(c.content)} == {16} and len(set(c.content)) == 64
    deepest_cl = 0
    for v in D.FIBONACCI_VARIANTS:
        c, o, s = by[f"alpha/fibonacci_15_bit_limit_v{v}"]
        freq = [0] * 286
        freq[256] = 1
        for b in D.Z.literals_of(c.content, c.tokens):
            freq[b] += 1
        for _, ml, _ in c.tokens:
            freq[G.length_symbol(ml)] += 1
        assert sorted(f for f in freq if f) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
        assert huffman(freq)[1] == 16 and o[1] == S.DYNAMIC and max(s.blocks[0].lit_lens) == 15      # the limit binds
    cl_runs = set()
    for c, o, s in by.values():
        for b in s.blocks:
            cl_runs |= {x for x in b.cl_symbols if x[0] >= 16}
            deepest_cl = max(deepest_cl, max(b.cl_lens or [0]))
    assert {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= cl_runs
    assert {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= set(by["alpha/code_length_runs"][2].blocks[0].cl_symbols)
    print("census: the longest code of a code-length alphabet has %d bits (the limit is 7)" % deepest_cl)
    # choice
    assert by["choice/stored_below_fixed"][1][1] == S.STORED and by["choice/fixed_below_dynamic"][1][1] == S.FIXED
    assert by["choice/dynamic_smallest"][1][1] == S.DYNAMIC
    _, (_, kind, bits, dyn, fixed, stored), _ = by["choice/fixed_equals_stored"]
    assert (kind, fixed, stored) == (S.STORED, 280, 280) and dyn > 280
    assert len(D.TIES) >= 3
    for k in D.TIES:
        _, (_, kind, bits, dyn, fixed, stored), _ = by[f"choice/dynamic_equals_fixed_{k}"]
        assert kind == S.FIXED and dyn == fixed < stored, k
    assert len(by["choice/stored_65535"][2].blocks) == 1 and len(by["choice/stored_65535"][0].content) == 65535
    s = by["choice/stored_65536"][2]
    assert [(b.kind, b.final, b.stored_bytes) for b in s.blocks] == [(0, 0, 65535), (0, 1, 1)]
    # the bit stage
    residues, longest, widest, third = set(), 0, 0, 0
    for c, (stream, kind, bits, *_), s in by.values():
        if kind == S.STORED:
            continue
        residues.add(bits % 32)
        longest = max(longest, bits)
        value = int.from_bytes(stream, "little")
        for _, m, e in s.ranges:
            widest = max(widest, e - m)
            # (bits that a 64-bit shift by the alignment loses: they go to a third dword of the kernel's stage)
            if (m & 31) + e - m > 64:
                code = (value >> m) & ((1 << (e - m)) - 1)
                third += code >> (64 - (m & 31)) != 0
    print("census: %d residues, longest stream %d bits, widest match code %d bits, %d reach a third dword" % (len(residues), longest, widest, third))
    assert residues == set(range(32))
    assert longest >= 3 * 1024 + 1024 and widest >= 40 and third >= 1
    total = sum(len(o[0]) for o in outs)
    print("census: %d streams, %d bytes in all" % (len(outs), total))


def test_the_driver_under_the_sanitizers(planned, tmp_path):
    cases, outs, _ = planned
    exe = build_driver(tmp_path, sanitize=True)
    again = encode_all(exe, tmp_path, [(c.content, c.tokens) for c in cases])
    assert again == outs
    # the command line form, and what it refuses
    r = subprocess.run([exe], input="encode 5 L97 L98 L99 L100 M8,4\nstream 1 5 L97 L98 L99 L100 M8,4\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a, b = (l.split() for l in r.stdout.splitlines())
    assert a[0] == b[0] and a[1] == "1" and a[2:] == b[1:]
    for bad in ("encode 2 L97 M4,2\n", "encode 1 M2,1\n", "encode @" + os.path.join(str(tmp_path), "absent") + "\n"):
        r = subprocess.run([exe], input=bad, capture_output=True, text=True)
        assert r.returncode in (3, 5) and "Sanitizer" not in r.stderr, (bad, r.returncode, r.stderr[-500:])
