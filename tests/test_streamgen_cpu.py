"""tests/streamgen.py checked without a GPU, at the seeds the GPU test uses (tests/test_decoder_token_forms_gpu.py):
every generated stream decodes with the CPU oracle to exactly the plain loop's output, the conforming LZ4 streams
with liblz4 too, and the census of the plans says that every family holds the token forms it claims."""
import ctypes

import pytest

import streamgen as SG


# (liblz4's streams are conforming: they have no reference-accepted kind)
@pytest.mark.parametrize("name, conforming", [(n, c) for n in SG.LZ4_FAMILIES for c in (True, False)
                                              if c or n != "liblz4"])
def test_lz4_family_agrees_with_oracle(oracle, name, conforming):
    cases = SG.lz4_family(name, conforming)
    if name == "liblz4" and SG.load_liblz4() is None:
        pytest.skip("liblz4.so.1 absent: no third-party LZ4 streams")
    assert cases
    for k, (stream, expected, plan) in enumerate(cases):
        if name != "liblz4":
            assert SG.encode_lz4(plan) == stream
        assert SG.expected_lz4(plan) == expected, f"{name} {k}: plan and expected output differ"
        assert all(s.off != 0 for s in plan if s.ml)
        assert oracle.lz4_decompress(stream, len(expected)) == (0, expected), f"{name} {k}"
        assert oracle.lz4_decompressed_size(stream) == (0, len(expected)), f"{name} {k}"


@pytest.mark.parametrize("name", [n for n in SG.LZ4_FAMILIES if n != "liblz4"])
def test_conforming_lz4_decodes_with_liblz4(name):
    L = SG.load_liblz4()
    if L is None:
        pytest.skip("liblz4.so.1 absent: the conforming streams are not checked against it")
    for k, (stream, expected, plan) in enumerate(SG.lz4_family(name, True)):
        buf = ctypes.create_string_buffer(max(len(expected), 1))
        n = L.LZ4_decompress_safe(stream, buf, len(stream), len(expected))
        assert n == len(expected) and buf.raw[:n] == expected, f"{name} {k}: liblz4 returned {n}"


def test_liblz4_rejects_what_only_the_reference_accepts():
    """The split between the two kinds: liblz4 refuses a stream that ends in a match and one whose last match
    starts fewer than 12 bytes before the end, and decodes the same content with conforming end tokens."""
    L = SG.load_liblz4()
    if L is None:
        pytest.skip("liblz4.so.1 absent")

    def dec(s, cap):
        buf = ctypes.create_string_buffer(max(cap, 1))
        return L.LZ4_decompress_safe(s, buf, len(s), cap)
    lit = SG.Seq(b"abcdefgh", 0, 0, -1)
    ends_in_match = [SG.Seq(b"abcdefgh", 20, 8, -1)]
    late_match = [SG.Seq(b"abcdefgh", 4, 8, -1), SG.Seq(b"XYZWV", 0, 0, -1)]       # starts 9 bytes before the end
    good = [SG.Seq(b"abcdefgh", 20, 8, -1), SG.Seq(b"XYZWV", 0, 0, -1)]
    for plan in (ends_in_match, late_match):
        assert dec(SG.encode_lz4(plan), len(SG.expected_lz4(plan))) < 0
    assert dec(SG.encode_lz4(good), 33) == 33
    assert dec(SG.encode_lz4([lit]), 8) == 8


def test_census():
    lz4 = SG.lz4_census({(name, c): SG.lz4_family(name, c) for name in SG.LZ4_FAMILIES for c in (True, False)})
    # (by family for the in-step figures: they are claims of short_steps)
    steps = SG.lz4_census({"short_steps": SG.lz4_family("short_steps", True) + SG.lz4_family("short_steps", False)})
    chain = SG.lz4_census({"chain_then": SG.lz4_family("chain_then", True) + SG.lz4_family("chain_then", False)})
    # chain_then by the loop the decoder takes for the whole chunk: each must hold every other family's forms
    tails = [c for kind in (True, False) for c in SG.lz4_family("chain_then", kind) if len(c[0]) >= 256]
    by_loop = {loop: SG.lz4_census({"chain_then": [c for c in tails if SG.chainy(c[0]) == loop]})
               for loop in (True, False)}
    sn = SG.snappy_census({name: SG.snappy_family(name) for name in SG.SNAPPY_FAMILIES})
    every = set(range(1, 65))
    print(f"\nLZ4 census: {lz4['streams']} streams, {lz4['output_bytes']} output bytes")
    print(f"  offsets with ml > offset, fast-path-(2) form: {len(lz4['fp2_offsets'] & set(range(1, 65)))} of 1..64; "
          f"general form (ml 65..300): {len(lz4['general_offsets'] & set(range(1, 65)))} of 1..64")
    print(f"  offset <= literals: offset < ml {len(lz4['in_literals_lt_ml'] & set(range(1, 65)))} of 1..64, "
          f"offset >= ml {len(lz4['in_literals_ge_ml'] & set(range(4, 65)))} of 4..64")
    print(f"  extension bytes: {len(lz4['ext_bytes'])} of 0..254; literal lengths 0..64 present: "
          f"{len(lz4['lit_lengths'] & set(range(65)))}; all-0xFF LSIC steps: {lz4['all_ff_steps']}")
    print(f"  short_steps: {steps['in_step_sources']} in-step sources, {steps['deep_chains']} chains of depth >= 6, "
          f"deepest {steps['max_depth']}")
    print(f"  chain_then: {chain['chain_prefixes']} CHAIN-loop streams, {chain['plain_prefixes']} plain-loop streams "
          f"of >= 256 bytes; far offsets: {sorted(o for o in lz4['far_offsets'] if o in SG.FAR_OFFSETS)} (and 1..64 above)")
    for loop, cc in by_loop.items():
        print(f"  chain_then, {'CHAIN' if loop else 'plain'} loop: {cc['streams']} streams, {cc['output_bytes']} "
              f"output bytes; literal-free short sequences at offsets "
              f"{sorted(o for o in cc['chain_form_offsets'] if o > 32767)} (> 32767); fast-path-(2) / general "
              f"offsets {len(cc['fp2_offsets'] & set(range(1, 65)))} / {len(cc['general_offsets'] & set(range(1, 65)))}"
              f" of 64; extension bytes {len(cc['ext_bytes'])}; all-0xFF steps {cc['all_ff_steps']}; last tokens "
              f"{sorted(b for b in cc['last_token_backs'] if b in (17, 18, 82))} bytes before the end")
    print(f"  last match-bearing tokens {sorted(b for b in lz4['last_token_backs'] if b in (17, 18, 82))} bytes "
          f"before the end; deepest in-step chain {lz4['max_depth']}")
    print(f"Snappy census: {sn['streams']} streams, {sn['output_bytes']} output bytes")
    for w in range(5):
        ls = sn["lit_lengths"][w]
        print(f"  literal, length field of {w} byte(s): {len(ls)} lengths, {min(ls)}..{max(ls)}")
    for kind in (1, 2, 4):
        ls = sn["copy_lengths"][kind]
        print(f"  copy-{kind}: lengths {min(ls)}..{max(ls)} ({len(ls)})")
    print(f"  copy-1 (length, offset) pairs: {len(sn['copy1_pairs'])}; offsets > 32768: copy-2 "
          f"{sn['far_copies'][2]}, copy-4 {sn['far_copies'][4]} (largest {sn['copy4_offset_max']}); varint widths "
          f"{sorted(sn['varint_widths'])}")

    assert lz4["fp2_offsets"] >= every and lz4["general_offsets"] >= every
    assert lz4["in_literals_lt_ml"] >= every and lz4["in_literals_ge_ml"] >= set(range(4, 65))
    assert lz4["ext_bytes"] >= set(range(255)) and lz4["lit_lengths"] >= set(range(65))
    assert lz4["all_ff_steps"] >= 1
    assert steps["in_step_sources"] >= 100 and steps["deep_chains"] >= 10
    assert chain["chain_prefixes"] >= 1 and chain["plain_prefixes"] >= 1
    assert steps["max_depth"] == 63
    assert {17, 18, 82} <= lz4["last_token_backs"]
    for loop, cc in by_loop.items():
        assert cc["streams"] >= 6 and cc["output_bytes"] > 6 * 65536, loop
        assert set(SG.FAR_OFFSETS) <= cc["chain_form_offsets"], loop    # (65535, 65534, 32768, 4096, 64, 65)
        assert cc["fp2_offsets"] >= every and cc["general_offsets"] >= every, loop
        assert cc["in_literals_lt_ml"] >= every and cc["in_literals_ge_ml"] >= set(range(4, 65)), loop
        assert cc["ext_bytes"] >= set(range(255)) and cc["lit_lengths"] >= set(range(65)), loop
        assert cc["all_ff_steps"] >= 1 and {17, 18, 82} <= cc["last_token_backs"], loop
    assert set(SG.FAR_OFFSETS) <= lz4["far_offsets"] | set(range(65))
    assert sn["lit_lengths"][0] >= set(range(1, 61)) and sn["lit_lengths"][1] >= set(range(1, 257))
    for w, ks in SG.WIDE_LIT_LENGTHS.items():
        assert sn["lit_lengths"][w] >= set(ks)
    assert sn["copy_lengths"][1] >= set(range(4, 12))
    assert sn["copy_lengths"][2] >= every and sn["copy_lengths"][4] >= every
    assert sn["copy1_pairs"] >= {(ln, o) for ln in range(4, 12) for o in range(1, 2048)}
    assert sn["far_copies"][2] > 0 and sn["far_copies"][4] > 0 and sn["copy4_offset_max"] > 65535
    assert sn["varint_widths"] >= {1, 2, 3, 4} and 0 in sn["usizes"]
    assert lz4["output_bytes"] + sn["output_bytes"] < 32 << 20


@pytest.mark.parametrize("name", list(SG.SNAPPY_FAMILIES))
def test_snappy_family_agrees_with_oracle(oracle, name):
    cases = SG.snappy_family(name)
    assert cases
    for k, (stream, expected, plan) in enumerate(cases):
        assert SG.encode_snappy(plan) == stream and SG.expected_snappy(plan) == expected
        assert oracle.snappy_decompress(stream, len(expected)) == (0, expected), f"{name} {k}"
        assert oracle.snappy_uncompressed_size(stream) == len(expected), f"{name} {k}"
