"""The code-building logic of the Deflate encoder (hipcomp-core_amd/csrc/deflate_compress/deflate_codes.hpp) on the
CPU.  The header is compiled with tests/deflate_codes_driver.cpp alone (g++, standard headers, no HIP); the kernel
includes the same header.  For planned and random histograms: the code lengths respect the limits (15 bits, 7 for
the code-length alphabet) and are accepted by deflate_tables.hpp's verdict_counts (through the decoder's own
driver), they cost exactly what a Huffman tree costs where the limit does not bind, and no more than a fixed-width
code where it does.  Whole one-block streams written with the header's functions decode in zlib, and the three
cost functions equal the bits written."""
import heapq
import os
import random
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
NLIT, NDIST, NCL = 286, 30, 19
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _build(tmp_path_factory, source, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, "-I", os.path.join(CSRC, "deflate"),
                        os.path.join(TESTS, source), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "deflate_codes_driver.cpp", "deflate_codes_driver")


@pytest.fixture(scope="module")
def tables_driver(tmp_path_factory):
    """the decoder's driver: `set KIND N lengths` -> deflate_tables.hpp's verdict_counts"""
    return _build(tmp_path_factory, "deflate_tables_driver.cpp", "deflate_tables_driver")


def run(exe, lines):
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


# ------------------------------------------------------------------------------------------- the test's own oracle
def huffman(freqs):
    """-> (cost, depth) of a Huffman tree of the used symbols, the shallowest of the optimal ones (ties go to the
    node of smaller height); a lone symbol costs one bit."""
    used = [f for f in freqs if f]
    if len(used) == 0:
        return 0, 0
    if len(used) == 1:
        return used[0], 1
    heap = [(f, 0) for f in used]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, ha = heapq.heappop(heap)
        b, hb = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(ha, hb) + 1))
    return cost, heap[0][1]


def package_merge(freqs, limit):
    """-> the cost of an optimal code of at most `limit` bits (boundary package-merge, the plain form)"""
    used = sorted(f for f in freqs if f)
    n = len(used)
    if n <= 1:
        return sum(used)
    leaves = [(f, (i,)) for i, f in enumerate(used)]
    packages = []
    for _ in range(limit):
        merged = sorted(leaves + packages, key=lambda p: p[0])
        packages = [(merged[k][0] + merged[k + 1][0], merged[k][1] + merged[k + 1][1]) for k in range(0, len(merged) - 1, 2)]
    lens = [0] * n
    for _, items in packages[:n - 1]:
        for i in items:
            lens[i] += 1
    return sum(f * l for f, l in zip(used, lens))


def check_alphabet(freqs, lens, limit, excess):
    """properties 1, 3 and 4 of one alphabet; -> its cost"""
    assert len(lens) == len(freqs)
    for f, l in zip(freqs, lens):
        assert (1 <= l <= limit) if f else l == 0, (f, l)
    cost = sum(f * l for f, l in zip(freqs, lens))
    best, depth = huffman(freqs)
    used = sum(1 for f in freqs if f)
    if depth <= limit:
        assert cost == best, (cost, best, depth)
    else:
        width = max(1, (used - 1).bit_length())
        assert cost <= width * sum(freqs), (cost, width * sum(freqs))
        over = cost - package_merge(freqs, limit)
        assert over >= 0
        excess.append((used, limit, cost, over))
    return cost


def run_length_histogram(lengths):
    """The code-length stream of RFC 1951 3.2.7 as the header writes it -- per run of equal lengths: a non-zero
    length once, then the longest repeats (16: 3..6, 17: 3..10 zeros, 18: 11..138 zeros), the rest plain -- as
    the histogram of its 19 symbols."""
    freq, i = [0] * NCL, 0
    while i < len(lengths):
        v, run = lengths[i], 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        i += run
        if v:
            freq[v] += 1
            run -= 1
        while run >= 3:
            take = min(run, 6 if v else 138)
            freq[16 if v else (17 if take <= 10 else 18)] += 1
            run -= take
        freq[v] += run
    return freq


def check_histogram(driver, tables_driver, lit, dist, excess):
    (line,) = run(driver, ["hist " + " ".join(map(str, lit + dist))])
    v = list(map(int, line.split()))
    lit_lens, dist_lens, cl_lens = v[:NLIT], v[NLIT:NLIT + NDIST], v[NLIT + NDIST:NLIT + NDIST + NCL]
    hlit, hdist, hclen, dyn, fixed = v[NLIT + NDIST + NCL:]
    assert lit[256] == 1 and lit_lens[256] >= 1   # symbol 256 is always coded
    lit_cost = check_alphabet(lit, lit_lens, 15, excess)
    dist_cost = check_alphabet(dist, dist_lens, 15, excess)
    assert all(1 <= l <= 7 or l == 0 for l in cl_lens)
    # 2. the decoder's verdict on each set
    got = run(tables_driver, ["set 1 %d %s" % (hlit, " ".join(map(str, lit_lens[:hlit]))),
                              "set 2 %d %s" % (hdist, " ".join(map(str, dist_lens[:hdist]))),
                              "set 0 %d %s" % (NCL, " ".join(map(str, cl_lens)))])
    assert got == ["verdict ok"] * 3, got
    # the header fields are trimmed, and to no less than the format's floors
    assert 257 <= hlit <= NLIT and all(l == 0 for l in lit_lens[hlit:]) and (hlit == 257 or lit_lens[hlit - 1])
    assert 1 <= hdist <= NDIST and all(l == 0 for l in dist_lens[hdist:]) and (hdist == 1 or dist_lens[hdist - 1])
    assert 4 <= hclen <= NCL and all(cl_lens[s] == 0 for s in CL_ORDER[hclen:]) and (hclen == 4 or cl_lens[CL_ORDER[hclen - 1]])
    # the fixed cost from the format's tables
    fixed_len = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    want_fixed = 3 + sum(f * (fixed_len[s] + (LENGTH_EXTRA[s - 257] if s > 256 else 0)) for s, f in enumerate(lit)) \
        + sum(f * (5 + DIST_EXTRA[s]) for s, f in enumerate(dist))
    assert fixed == want_fixed
    # the dynamic cost exactly: header, the symbols (checked above), and the code-length stream -- the run-length
    # symbols derived here from the returned lengths -- under the returned code-length code
    extras = sum(f * LENGTH_EXTRA[s - 257] for s, f in enumerate(lit) if s > 256) + sum(f * DIST_EXTRA[s] for s, f in enumerate(dist))
    cl_freq = run_length_histogram(lit_lens[:hlit] + dist_lens[:hdist])
    assert all(cl_lens[s] for s in range(NCL) if cl_freq[s]), "a used code-length symbol without a code"
    cl_cost = sum(cl_freq[s] * (cl_lens[s] + CL_EXTRA.get(s, 0)) for s in range(NCL))
    assert dyn == 17 + 3 * hclen + cl_cost + lit_cost + dist_cost + extras
    check_alphabet(cl_freq, cl_lens if sum(1 for f in cl_freq if f) > 1 else [l if f else 0 for l, f in zip(cl_lens, cl_freq)], 7, excess)
    return dyn, fixed


def fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def planned_histograms():
    z_lit, z_dist = [0] * NLIT, [0] * NDIST
    eob = lambda l: l[:256] + [1] + l[257:]   # noqa: E731  (256 is counted once)
    cases = {}
    cases["empty"] = (eob(z_lit), z_dist)
    one = list(z_lit); one[65] = 9
    cases["one_symbol"] = (eob(one), z_dist)
    two = list(z_lit); two[65] = 9; two[66] = 4
    cases["two_symbols"] = (eob(two), z_dist)
    cases["all_used_equal"] = (eob([7] * NLIT), [7] * NDIST)
    f = fib(40)
    geo = [f[i % 32] if i != 256 else 1 for i in range(NLIT)]
    cases["fibonacci_forces_15_bits"] = (geo, f[:NDIST])
    steep = list(z_lit)
    for k, s in enumerate(range(0, 256, 8)):
        steep[s] = f[k] if k < 32 else 1
    cases["fibonacci_32_literals"] = (eob(steep), f[5:5 + NDIST][::-1])
    text = [0] * NLIT
    for s in range(32, 127):
        text[s] = 1 + (s * 37) % 101
    cases["only_literals"] = (eob(text), z_dist)
    m = list(text); m[260] = 12; m[285] = 3
    d = list(z_dist); d[17] = 15
    cases["one_distance_symbol"] = (eob(m), d)
    return cases


@pytest.mark.parametrize("name", list(planned_histograms()))
def test_planned_histograms(driver, tables_driver, name):
    lit, dist = planned_histograms()[name]
    excess = []
    check_histogram(driver, tables_driver, lit, dist, excess)
    for used, limit, cost, over in excess:
        print(f"{name}: {used} symbols at {limit} bits: cost {cost}, {over} above package-merge ({100.0 * over / cost:.3f} %)")
    if name.startswith("fibonacci"):
        assert excess, "the planned frequencies were meant to force the limit"


def test_code_length_alphabet_at_its_7_bit_limit(driver):
    """19 Fibonacci frequencies: a Huffman tree 18 deep, cut to 7 bits"""
    excess = []
    for freqs in (fib(19), fib(19)[::-1], [3 * x for x in fib(12)] + [0] * 7, [1] * 19, [5] + [0] * 18, [0] * 19):
        (line,) = run(driver, ["alpha 7 19 " + " ".join(map(str, freqs))])
        check_alphabet(freqs, list(map(int, line.split())), 7, excess)
    assert len(excess) >= 3
    for used, limit, cost, over in excess:
        print(f"code-length alphabet: {used} symbols at {limit} bits: cost {cost}, {over} above package-merge")


def test_2000_random_histograms(driver, tables_driver):
    rnd = random.Random(1951)
    excess, n_limited = [], 0
    for k in range(2000):
        shape = k % 5
        lit, dist = [0] * NLIT, [0] * NDIST
        n_lit = rnd.choice((1, 2, 3, 17, 96, 200, NLIT))
        for s in rnd.sample(range(NLIT), n_lit):
            lit[s] = (rnd.randrange(1, 4), rnd.randrange(1, 2000), int(rnd.paretovariate(0.6)), 1 << rnd.randrange(0, 17),
                      rnd.randrange(1, 65536))[shape]
        for s in rnd.sample(range(NDIST), rnd.choice((0, 1, 2, 9, NDIST))):
            dist[s] = (rnd.randrange(1, 4), rnd.randrange(1, 500), int(rnd.paretovariate(0.6)), 1 << rnd.randrange(0, 15),
                       rnd.randrange(1, 16384))[shape]
        lit = [min(f, 65536) for f in lit]
        dist = [min(f, 16384) for f in dist]
        lit[256] = 1
        before = len(excess)
        check_histogram(driver, tables_driver, lit, dist, excess)
        n_limited += len(excess) > before
    worst = max(excess, key=lambda e: e[3] / e[2], default=None)
    print(f"{n_limited} of 2000 histograms met the 15-bit limit; largest excess over package-merge: {worst}")


# --------------------------------------------------------------------------------------------------- whole streams
def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def planned_token_lists():
    rnd = random.Random(7)
    lists = {"empty": [], "one_literal": [120], "abc": [97, 98, 99]}
    lists["every_length"] = [1, 2, 3, 4] + [(n, 1 + n % 4) for n in range(3, 259)]
    far = [rnd.randrange(256) for _ in range(33000)]
    lists["every_distance_symbol"] = far + [(3 + s, d) for s in range(30)
                                            for d in {1 << (s // 2) if s > 1 else s + 1, 32768 if s == 29 else (3 << (s // 2 - 1)) if s > 3 else s + 1}]
    text = [ord(c) for c in "the quick brown fox jumps over the lazy dog "]
    mixed = list(text)
    for k in range(400):
        mixed += [(rnd.randrange(3, 40), rnd.randrange(1, len(text)))] if k % 3 else [rnd.choice(text), rnd.choice(text)]
    lists["text_like"] = mixed
    lists["random_literals"] = [rnd.randrange(256) for _ in range(3000)]
    lists["one_run"] = [0, (258, 1), (258, 1), (100, 1)]
    return lists


@pytest.mark.parametrize("name", list(planned_token_lists()))
def test_streams_written_with_the_headers_functions_decode_in_zlib(driver, name):
    tokens = planned_token_lists()[name]
    want = expand(tokens)
    words = " ".join(f"L{t}" if isinstance(t, int) else f"M{t[0]},{t[1]}" for t in tokens)
    out = run(driver, [f"stream {kind} {len(tokens)} {words}" for kind in (0, 1, 2)])
    costs = None
    for kind, line in enumerate(out):
        hexed, bits, dyn, fixed, stored = line.split()
        stream = bytes.fromhex(hexed)
        bits, dyn, fixed, stored = int(bits), int(dyn), int(fixed), int(stored)
        d = zlib.decompressobj(-15)
        got = d.decompress(stream)
        assert d.eof and d.unused_data == b"" and got == want, (name, kind)
        assert (stream[0] >> 1) & 3 == kind and stream[0] & 1
        assert len(stream) == (bits + 7) // 8
        # 6. the cost function of this kind is the bit length of the stream written
        assert bits == (stored, fixed, dyn)[kind], (name, kind, bits, (stored, fixed, dyn))
        assert costs in (None, (dyn, fixed, stored))
        costs = (dyn, fixed, stored)
    assert costs[2] == 8 * (len(want) + 5)
