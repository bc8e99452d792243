"""The canonical-Huffman logic of the Deflate decoder (hipcomp-core_amd/csrc/deflate/deflate_tables.hpp) on the
CPU.  The header is compiled with tests/deflate_tables_driver.cpp alone (g++, standard headers, no HIP).  Every set
of code lengths is wrapped into a one-block stream by tests/deflate_streamgen.py and given both to the driver --
which decodes the block with the header's verdicts, tables and lookups -- and to zlib.decompressobj(-15): the
driver's verdict has to be zlib's accept / reject, and for an accepted set the symbols it decodes have to expand
to zlib's output.  The kernel includes the same header and fills its tables with the same walk."""
import os
import subprocess
import zlib

import pytest

import deflate_streamgen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_tables") / "deflate_tables_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC,
                        os.path.join(TESTS, "deflate_tables_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(driver, lines):
    r = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def expand(symbols):
    out = bytearray()
    for s in symbols:
        if s[0] == "L":
            out.append(int(s[1:]))
        else:
            n, d = map(int, s[1:].split(","))
            assert 1 <= d <= len(out), "the test's own payloads keep their distances inside the output"
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def payload_for(lit, dist):
    """Tokens that use every coded literal, every coded length symbol and every coded distance symbol whose
    distances the output so far can serve."""
    toks = [s for s in range(min(len(lit), 256)) if lit[s]] * 2
    if not toks:
        return []
    made = len(toks)
    dsyms = [s for s in range(min(len(dist), 30)) if dist[s]]
    usable = [s for s in dsyms if G.DIST_BASE[s] <= made]
    if not usable:
        return toks
    k = 0
    for ls in range(257, min(len(lit), 286)):
        if lit[ls]:
            for x in sorted({0, (1 << G.LENGTH_EXTRA[ls - 257]) - 1}):
                ds = usable[k % len(usable)]
                k += 1
                toks.append(("m", G.LENGTH_BASE[ls - 257] + x, G.DIST_BASE[ds], ls))
    if any(lit[257:]):
        ls = next(s for s in range(257, len(lit)) if lit[s])
        for ds in usable:
            span = min((1 << G.DIST_EXTRA[ds]) - 1, made - G.DIST_BASE[ds])
            for x in sorted({0, span}):
                toks.append(("m", G.LENGTH_BASE[ls - 257], G.DIST_BASE[ds] + x, ls))
    return toks


def lengths_of_zlib_streams():
    """The two sets of code lengths of the first dynamic block of real zlib streams (read back with the
    generator's own tables: the header is parsed here in Python)."""
    sets = []
    text = G._text(30000, 21)
    for data, level, strategy in ((text, 6, zlib.Z_DEFAULT_STRATEGY), (text, 1, zlib.Z_DEFAULT_STRATEGY),
                                  (text, 9, zlib.Z_HUFFMAN_ONLY), (bytes((i // 5) & 0xFF for i in range(20000)), 6, zlib.Z_RLE),
                                  (b"ab" * 5000 + text[:3000], 9, zlib.Z_DEFAULT_STRATEGY)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        s = c.compress(data) + c.flush()
        bits = "".join(format(b, "08b")[::-1] for b in s)

        def take(pos, n):
            return int(bits[pos:pos + n][::-1] or "0", 2), pos + n
        _, pos = take(0, 1)
        btype, pos = take(pos, 2)
        assert btype == 2
        hlit, pos = take(pos, 5)
        hdist, pos = take(pos, 5)
        hclen, pos = take(pos, 4)
        cl = [0] * 19
        for k in range(hclen + 4):
            cl[G.CL_ORDER[k]], pos = take(pos, 3)
        codes = {(c, ln): sym for sym, (c, ln) in G.canonical_codes(cl).items()}
        lens = []
        while len(lens) < hlit + 257 + hdist + 1:
            c, ln = 0, 0
            while (c, ln) not in codes:
                b, pos = take(pos, 1)
                c, ln = (c << 1) | b, ln + 1
            sym = codes[(c, ln)]
            if sym < 16:
                lens.append(sym)
            elif sym == 16:
                x, pos = take(pos, 2)
                lens += [lens[-1]] * (3 + x)
            elif sym == 17:
                x, pos = take(pos, 3)
                lens += [0] * (3 + x)
            else:
                x, pos = take(pos, 7)
                lens += [0] * (11 + x)
        sets.append((f"zlib_level{level}_strategy{strategy}_{len(sets)}", lens[:hlit + 257], lens[hlit + 257:]))
    return sets


def accepted_sets():
    sets = lengths_of_zlib_streams()
    sets.append(("single_distance_code", G.flat_lengths(set(range(97, 123)) | {256, 257, 258, 270}, 271), [1]))
    sets.append(("single_distance_code_not_the_first", G.flat_lengths(set(range(97, 123)) | {256, 257, 285}, 286),
                 [0, 0, 0, 1]))
    sets.append(("no_distance_code", G.flat_lengths(set(range(32, 127)) | {256}, 257), [0]))
    sets.append(("only_end_of_block", [0] * 256 + [1], [0]))
    sets.append(("max_alphabets_15_bits", G.max_alphabet_litlen(), G.max_alphabet_dist()))
    sets.append(("two_one_bit_codes", [1] + [0] * 255 + [1], [1, 1]))
    return sets


def test_fixed_block_codes(driver):
    """The fixed code itself (288 + 32 lengths, only a fixed block carries them): every literal, every length
    symbol with its extremes, distance symbols within reach."""
    toks = payload_for(G.FIXED_LITLEN, G.FIXED_DIST)
    w = G.BitWriter()
    G.fixed_block(w, toks, True)
    s = w.done()
    ok, want = G.zlib_verdict(s)
    assert ok and want == G.expand(toks)
    (line,) = run(driver, ["block " + s.hex()])
    assert line.split()[0] == "ok" and expand(line.split()[1:]) == want


def test_fixed_lengths_cut_to_what_a_dynamic_header_can_name_are_incomplete(driver):
    """286 + 30 of the fixed code's 288 + 32 lengths: both sets lack codes, zlib and the driver refuse them."""
    s = G.one_dynamic_block(G.FIXED_LITLEN[:286], [5] * 30, [65, 66])
    assert not G.zlib_verdict(s)[0]
    assert run(driver, ["block " + s.hex()]) == ["reject incomplete"]
    assert run(driver, ["set 2 30 " + " ".join(["5"] * 30)]) == ["verdict incomplete"]


@pytest.mark.parametrize("case", accepted_sets(), ids=lambda c: c[0])
def test_accepted_sets_decode_as_zlib_does(driver, case):
    name, lit, dist = case
    toks = payload_for(lit, dist)
    for rle in (True, False):
        s = G.one_dynamic_block(lit, dist, toks, rle=rle)
        ok, want = G.zlib_verdict(s)
        assert ok, f"{name}: zlib refuses the set"
        assert want == G.expand(toks)
        (line,) = run(driver, ["block " + s.hex()])
        w = line.split()
        assert w[0] == "ok", (name, line[:80])
        assert len(w) - 1 == len(toks) and expand(w[1:]) == want, name
    # the verdicts on the sets alone
    got = run(driver, ["set 1 %d %s" % (len(lit), " ".join(map(str, lit))), "set 2 %d %s" % (len(dist), " ".join(map(str, dist)))])
    assert got == ["verdict ok", "verdict ok"], (name, got)


EXPECTED_REASON = {
    "litlen_oversubscribed": "oversubscribed", "litlen_incomplete": "incomplete", "dist_oversubscribed": "oversubscribed",
    "dist_incomplete_two_codes": "incomplete", "dist_single_code_of_two_bits": "incomplete",
    "litlen_without_256": "no-end-of-block", "code_length_code_oversubscribed": "oversubscribed",
    "code_length_code_incomplete": "incomplete", "code_length_code_single": "incomplete",
    "hlit_287": "too-many-symbols", "hlit_288": "too-many-symbols", "hdist_31": "too-many-symbols",
    "hdist_32": "too-many-symbols", "repeat_16_first": "repeat-without-previous",
    "repeat_16_past_the_end": "repeat-past-end", "repeat_17_past_the_end": "repeat-past-end",
    "repeat_18_past_the_end": "repeat-past-end", "hclen_4_all_lengths_zero": "no-end-of-block",
}


def test_rejected_sets_are_rejected_as_zlib_does(driver):
    cases = G.rejected_sets()
    assert {n for n, _ in cases} == set(EXPECTED_REASON)   # no form left out
    got = run(driver, ["block " + s.hex() for _, s in cases])
    for (name, s), line in zip(cases, got):
        assert not G.zlib_verdict(s)[0], f"{name}: zlib accepts it"
        assert line == "reject " + EXPECTED_REASON[name], (name, line)


def test_every_planned_block_gets_zlibs_verdict(driver):
    """Every planned stream of the generator whose first block is a fixed or dynamic one that zlib's verdict
    depends on alone (one block, no match into history): the driver's verdict is zlib's."""
    n = 0
    for name, s, want in G.legal_plans():
        if (s[0] >> 1) & 3 in (1, 2) and s[0] & 1 and name != "trailing_bytes":
            (line,) = run(driver, ["block " + s.hex()])
            assert line.split()[0] == "ok" and expand(line.split()[1:]) == want, name
            n += 1
    assert n >= 10
