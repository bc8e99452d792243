"""The planned inputs of tests/zstd_inputgen.py on the CPU: the mirror of the parse rule returns every plan, the
scalar encoder of tests/zstd_codes_driver.cpp (built under AddressSanitizer and UBSan, a process of its own, with
tests/test_zstd_codes_cpu.py's helpers) writes a frame from every (content, tokens) that both judges decode to the
content, and a census over those frames asserts that the inputs meet the edges they were planned for: every
listed code, every table mode, every literals form, a block kept one byte below the chunk's size beside a raw
fall-back, a first field of a sequence that reaches a third dword of the kernel's bit stage, and every alignment.
tests/test_zstd_encoder_edges_gpu.py gives the same cases to the kernel."""
import pytest

import zstd_framegen as G
import zstd_inputgen as Z
import zstd_seqscan as S
from test_zstd_codes_cpu import drivers, encode_all, judged   # noqa: F401  (drivers is the fixture that builds them)


@pytest.fixture(scope="module")
def scalar(drivers, tmp_path_factory):
    """-> (cases, the scalar encoder's frame of every case)"""
    cases = Z.all_cases()
    frames = encode_all(drivers, tmp_path_factory.mktemp("inputgen"), [(c.content, c.scalar_tokens(), 0) for c in cases])
    return cases, frames


def test_the_mirror_returns_every_plan():
    cases = Z.all_cases()
    assert 250 <= len(cases) <= 400 and len({c.name for c in cases}) == len(cases)
    planned = 0
    for c in cases:
        assert len(c.content) <= Z.MAX_CHUNK, c.name
        if c.tokens is None or c.scalar_only:
            continue
        planned += 1
        got = Z.parse(c.content, c.copies)      # (raises PlanError where a lookup that matters is ambiguous)
        assert (got or []) == c.tokens, c.name
        assert Z.rebuilds(c.content, c.tokens) and Z.maximal(c.content, c.tokens), c.name
        assert not c.copies or sorted(c.copies) == Z.copy_positions(c.tokens), c.name
    print("%d cases, %d of them planned" % (len(cases), planned))
    assert planned >= len(cases) - 12
    # the same seeds give the same chunks
    again = Z.FAMILIES["trip_edges"]()
    assert [(c.name, c.content, c.tokens) for c in again] == [(c.name, c.content, c.tokens) for c in Z.family("trip_edges")]


def test_the_families_hold_what_is_listed():
    by = {c.name: c for c in Z.all_cases()}
    tag = lambda fam, key: {c.tags[key] for c in Z.family(fam) if key in c.tags}
    assert tag("trip_edges", "hit_lane") == {0, 1, 62, 63} and tag("trip_edges", "tail") >= {1, 2, 3}
    for k in (0, 1, 62, 63):                     # the planted copy is found on that lane of a trip that starts at the pool's end
        ll, ml, off = by[f"trip/hit_lane{k}"].tokens[1]
        assert ll % 64 == k and ml == 9
    last = by["trip/match_at_len_minus_4"]
    assert last.tokens[-1][1] == 4 and Z.copy_positions(last.tokens)[-1] == len(last.content) - 4
    assert len(by["trip/source_in_the_same_trip"].tokens) == 1
    assert tag("match_extension", "L") == set(Z.MATCH_LENGTHS) and tag("match_extension", "offset") == {1, 2, 3}
    for c in Z.family("match_extension"):
        if "L" in c.tags:
            assert c.tokens[-1][1] == c.tags["L"]
            end = sum(ll + ml for ll, ml, _ in c.tokens)
            assert (end < len(c.content)) == c.tags["by_byte"], c.name
    assert tag("literal_runs", "ll") == set(Z.LITERAL_RUNS)
    lls = {t[0] for c in Z.family("code_boundaries") for t in c.tokens}
    mls = {t[1] for c in Z.family("code_boundaries") for t in c.tokens}
    offs = {t[2] for c in Z.family("code_boundaries") for t in c.tokens}
    assert all({G.LL_BASE[k], G.LL_BASE[k] - 1} <= lls for k in Z.LL_CODES) and 65532 in lls
    assert all({G.ML_BASE[k], G.ML_BASE[k] - 1} <= mls for k in Z.ML_CODES) and 65534 in mls
    assert all({(1 << k) - 3, max((1 << k) - 4, 1)} <= offs for k in Z.OF_CODES) and 65532 in offs
    assert {len(c.tokens) for c in Z.family("sequence_counts")} == set(Z.SEQUENCE_COUNTS) | {Z.MANY_SEQUENCES}
    nlits = {len(Z.literals_of(c.content, c.tokens)) for c in Z.family("literal_forms") if c.tokens is not None}
    assert set(Z.LITERAL_COUNTS) <= nlits
    assert {(c.tags["n"], c.tags["idx"]) for c in Z.family("near_rle") if "n" in c.tags} >= {
        (n, i) for n in Z.NEAR_RLE_LENGTHS for i in (1, 63, 64, 65, n - 1) if i < n}
    a, b = by["repeat/same_offset_behind_literals"].tokens[-2:]
    assert a[2] == b[2] and b[0] > 0
    assert by["repeat/first_sequence_offset_1"].tokens[0][2] == 1


def test_the_mirror_refuses_what_the_hardware_decides():
    c = {x.name: x for x in Z.all_cases()}["trip/hit_lane1"]
    q, src = sorted(c.copies.items())[1]
    with pytest.raises(Z.PlanError, match="never posted|overwritten"):
        Z.parse(c.content, {q: src + 1})
    # two lanes of the first trip post the word "aaaa", and a lane of the second trip holds it
    with pytest.raises(Z.PlanError, match="two candidates"):
        Z.parse(b"ab" + b"a" * 127)
    # the planned source shares its slot with the lane behind it
    with pytest.raises(Z.PlanError, match="shared its slot"):
        Z.parse(b"ab" + b"a" * 127, {64: 2})
    # position 0 is a candidate: a source in the same trip is found there and nowhere else
    assert Z.parse(b"abcdabcdabcdXYZW") == [(4, 8, 4)]
    assert Z.parse(b"xabcdabcdabcdXYZ") == []


def test_both_judges_return_the_content(scalar, drivers, tmp_path):
    cases, frames = scalar
    judged(drivers, tmp_path, [(c.name, c.content, c.scalar_tokens(), 0) for c in cases], frames)


def test_census(scalar):
    cases, frames = scalar
    forms, pairs = set(), set()
    ll_codes, ml_codes, of_codes = set(), set(), set()
    starts, widest, third_dword = set(), 0, 0
    kept, raw_in_sweep, deep = {}, 0, 0
    compressed = 0
    for c, f in zip(cases, frames):
        fm = G.inspect(f)
        forms |= fm
        kind, payload = S.compressed_block(f)
        if c.family == "limit":
            if kind == 2:
                kept[len(c.content) - len(payload)] = kept.get(len(c.content) - len(payload), 0) + 1
            else:
                assert kind == 0
                raw_in_sweep += 1
        if kind != 2:
            continue
        compressed += 1
        assert len(payload) < len(c.content), c.name
        ranges = []
        seqs = S.sequences_of(f, ranges)
        assert S.resolve(seqs) == c.scalar_tokens(), c.name
        assert S.tokens_of(f) == c.scalar_tokens(), c.name
        for (ll, ml, ov), (low, high, na, first) in zip(seqs, ranges):
            ll_codes.add(G.ll_code(ll))
            ml_codes.add(G.ml_code(ml))
            of_codes.add(ov.bit_length() - 1)
            starts.add(low % 32)
            widest = max(widest, na)
            # (bits that a 64-bit shift by the alignment loses: they go to a third dword of the kernel's stage)
            third_dword += low % 32 + na > 64 and first >> (64 - low % 32) != 0
            assert na <= 41 and high - low - na <= 32
        for t in ("ll", "of", "ml"):
            pairs |= {(t, m) for m in ("rle", "predefined", "fse") if f"{t}_{m}" in fm}
        if c.tags.get("deep_tree"):
            lits = Z.literals_of(c.content, c.scalar_tokens())
            assert max(G.huf_lengths(lits, 32).values()) > 11      # Huffman's own code is deeper than the format allows
            assert fm & {"huffman_literals_4_stream_4", "huffman_literals_4_stream_5"}, c.name   # and the frame has a tree
            deep += 1
    print("census: %d cases, %d compressed blocks; LL codes %s; ML codes %s; OF codes %s" % (
        len(cases), compressed, sorted(ll_codes), sorted(ml_codes), sorted(of_codes)))
    print("census: forms %s" % sorted(forms))
    print("census: block limit sweep kept %s (bytes below n: count), raw %d; widest first field %d bits, %d set a bit in a third "
          "dword; %d alignments" % (dict(sorted(kept.items())), raw_in_sweep, widest, third_dword, len(starts)))
    assert set(Z.LL_CODES) <= ll_codes and set(Z.ML_CODES) <= ml_codes and set(Z.OF_CODES) <= of_codes
    assert len(pairs) == 9, pairs
    assert {"seq_count_1", "seq_count_2", "raw_literals_1", "raw_literals_2", "raw_literals_3", "huffman_literals_1_stream_3",
            "huffman_literals_4_stream_4", "huffman_literals_4_stream_5", "weights_direct", "weights_fse",
            "raw_block", "rle_block", "compressed_block"} <= forms
    assert deep >= 1
    assert kept.get(1, 0) >= 1 and raw_in_sweep >= 1, kept
    assert third_dword >= 1 and starts == set(range(32))
