"""Planned INPUTS for the Deflate encoder (plain Python and numpy, no GPU, nothing read from the kernel sources).

The Deflate and the Zstandard encoder share the parse rule, so this module shares its mirror: zstd_inputgen.parse
with max_match 258 and max_distance 32768, and zstd_inputgen's Chunk, PlanError, rebuilds, maximal and _build by
import.  A case carries the token list [(literal run, match length, distance)] its plan intends; mirror() must
return exactly that list (tests/test_deflate_inputgen_cpu.py), and the kernel must too
(tests/test_deflate_encoder_edges_gpu.py).  There is no model of the code builder, the costs or the bit writer
here: expected bytes come from deflate_codes.hpp through tests/deflate_codes_driver.cpp's `encode`.

records() builds the kernel's record list from the tokens by the record rules as DESIGN.md section 14 and the
kernel's comments state them: {literal run, match length, distance - 1} per record; a trip without a hit adds its
positions (64, fewer at the chunk's end) to the pending run, and once the pending run passes 191 a literal-only
record is sent off; one final record always follows, possibly empty.  After a match the next trip starts at the
match's end, so a literal run of r = 64 k + t in front of a match is k trips without a hit and a hit on lane t:
a record of 192 literals for every three such trips, and (k mod 3) * 64 + t in the match's record.

Besides zstd_inputgen's Chunk there is one more builder, _unit_walk(): a pool of literals whose words all have
slots of their own, and behind it matches back to back with no literal between, each a copy of a unit (an offset
of the pool with one length) from the unit's latest occurrence.  A match ends where the unit ends because the byte
behind it -- the first byte of the next unit -- differs from the byte behind the unit's occurrence before.  It gives
the chunk with the most records, and the chunk whose literal/length histogram is a Fibonacci ladder of 17 symbols:
the rare ones literals, the frequent ones match lengths.

What no input reaches:
  * A match of fewer than 4 bytes at run 0 behind a 258-byte match: a repeat of 259 bytes is a match of 258 and
    one literal (extend/repeat259); 262 and 600 give the same distance again with literal run 0.
  * The 7-bit limit of the code-length alphabet: its tree is deeper than 7 only if nine of the code-length symbols
    occur in Fibonacci proportion (1 1 2 3 5 8 13 21 34) among at most 316 lengths, which needs a literal/length
    code with nine different lengths whose counts are those AND whose equal neighbours do not fold into symbol 16;
    no plan here does that.  The header is held to that limit on the CPU (tests/test_deflate_codes_cpu.py); the
    census prints the longest code-length code the cases meet.
  * dynamic == fixed exactly comes from a search (tie_candidates(), fixed seed): TIES lists the candidates the
    shipped header prices equal, and the census asserts the tie through the driver.
"""
from __future__ import annotations

import random
import struct

import numpy as np

import zstd_inputgen as Z
from zstd_inputgen import Case, Chunk, PlanError, rebuilds, zhash   # noqa: F401  (re-exported for the tests)

MIN_MATCH, MAX_MATCH, MAX_DISTANCE = 4, 258, 32768
MAX_CHUNK = 65536
RUN_SENT = 192          # a pending run of more than 191 literals leaves as a record of its own


def mirror(data: bytes, copies=None):
    """-> (tokens, records) of the encoder's parse of `data`; PlanError where the hardware decides"""
    tokens = Z.parse(data, copies, MAX_MATCH, MAX_DISTANCE) if len(data) >= 4 else []
    return tokens, records(tokens, len(data))


def records(tokens, n):
    """the wave's record buffer for these tokens of a chunk of n bytes: [(literal run, match length, distance - 1)]"""
    out, pos = [], 0
    for ll, ml, dist in tokens:
        out += [(RUN_SENT, 0, 0)] * (ll // RUN_SENT)
        out.append((ll % RUN_SENT, ml, dist - 1))
        pos += ll + ml
    rest = n - pos
    assert rest >= 0
    out += [(RUN_SENT, 0, 0)] * (rest // RUN_SENT)
    out.append((rest % RUN_SENT, 0, 0))
    return out


def tokens_of(recs):
    """the inverse of records(): -> (tokens, the literals behind the last match)"""
    tokens, run = [], 0
    for ll, ml, d in recs:
        run += ll
        if ml:
            tokens.append((run, ml, d + 1))
            run = 0
    return tokens, run


def record_words(recs):
    return [(ll << 24) | (ml << 15) | d for ll, ml, d in recs]


def maximal(content: bytes, tokens) -> bool:
    """each match ends at 258, at the chunk's end or at a differing byte"""
    pos = 0
    for ll, ml, dist in tokens:
        if ml < MAX_MATCH and not Z.maximal(content, [(pos + ll, ml, dist)]):
            return False
        pos += ll + ml
    return True


def _B(seed, fn, alphabet=Z.LOW, tries=60):
    return Z._build(seed, fn, alphabet, tries, max_match=MAX_MATCH, max_distance=MAX_DISTANCE)


def _fixed(name, content, **tags):
    """a chunk laid out by hand whose plan is `no match`: the mirror has to agree"""
    tokens, _ = mirror(content)
    if tokens:
        raise PlanError(f"{name}: a match was found")
    return Case(name, content, [], tags=tags)


def _unplanned(name, content, **tags):
    """a chunk without a plan: its tokens are the mirror's where no lookup of it is ambiguous, else the encoder's"""
    try:
        tokens = mirror(content)[0]
    except PlanError:
        tokens = None
    return Case(name, content, tokens, tags=tags)


# ------------------------------------------------------------------------------------------------------ the families

def _near(c, k, L, tail):
    c.head()
    s = c.pool(80)
    c.protect(s + 5)
    c.lit(k, then=s + 5)
    c.copy(L, s + 5)
    c.lit(tail)


def trip_edges(seed=1):
    out = []
    for k in (0, 1, 62, 63):
        out.append(_B([seed, 0, k], lambda c, k=k: (_near(c, k, 9, 7), c.finish(f"trip/hit_lane{k}", hit_lane=k))[1]))
    for tail in (1, 2, 3):
        out.append(_B([seed, 1, tail], lambda c, t=tail: (_near(c, 5, 6, t), c.finish(f"trip/tail{t}", tail=t))[1]))
    out.append(_B([seed, 2], lambda c: (_near(c, 5, 4, 0), c.finish("trip/match_at_len_minus_4"))[1]))

    def same_trip(c):
        c.head()
        a = len(c)
        c.lit(10)
        c.echo(6, a + 2)             # its source is posted only behind this trip's lookups
        c.lit(20)
        return c.finish("trip/source_in_the_same_trip")
    out.append(_B([seed, 3], same_trip))

    def trip_before(c):
        c.head()
        s = c.pool(64)
        c.protect(s + 60)
        c.lit(3, then=s + 60)
        c.copy(8, s + 60)
        c.lit(6)
        return c.finish("trip/source_in_the_trip_before")
    out.append(_B([seed, 4], trip_before))

    def position0(c):                # every empty slot names position 0: a source in the copy's own trip, found
        c.lit(4, then=0)
        c.copy(8, 0)
        c.lit(6)
        return c.finish("trip/position0_of_an_empty_slot")
    out.append(_B([seed, 5], position0))
    for n in range(6):
        out.append(_fixed(f"trip/len{n}", b"abcde"[:n], n=n))
    return out


MATCH_LENGTHS = (4, 5, 67, 68, 69, 131, 132, 133, 195, 196, 197, 257, 258)
REPEATS = (259, 262, 600)


def match_extension(seed=2):
    out = []

    def one(c, L, by_byte):
        c.head()
        s = c.pool(L + 16)
        for k in range(0, L, MAX_MATCH):
            c.protect(s + 2 + k)
        c.lit(5, then=s + 2)
        c.copy(L, s + 2)
        if by_byte:
            c.lit(9)
        kind = "repeat" if L > MAX_MATCH else "L"
        return c.finish(f"extend/{kind}{L}" + ("" if L > MAX_MATCH else "_byte" if by_byte else "_end"), L=L, by_byte=by_byte)
    for L in MATCH_LENGTHS:
        for by_byte in (True, False):
            out.append(_B([seed, L, by_byte], lambda c, L=L, b=by_byte: one(c, L, b)))
    for L in REPEATS:
        out.append(_B([seed, L], lambda c, L=L: one(c, L, True)))

    def overlap(c, d, L):
        c.head()
        q = len(c) + 64
        c.lit(64, then=q - d)        # a whole trip: the source is lane 64 - d of the trip before the copy's
        c.copy(L, q - d)
        c.lit(6)
        return c.finish(f"extend/distance{d}_L{L}", overlap=d)
    for d in (1, 2, 3):
        for L in (4, 70, 258):
            out.append(_B([seed, 100 + d, L], lambda c, d=d, L=L: overlap(c, d, L)))
    return out


DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
EDGE_CLASSES = (4, 5, 10, 17, 24, 29)     # distance symbols whose first and last distance are planned
DISTANCES = tuple(sorted({1, 4, 5, 32767, 32768} | {d for s in EDGE_CLASSES
                                                    for d in (DIST_BASE[s], (DIST_BASE[s + 1] if s < 29 else 32769) - 1)}))


def distances(seed=3):
    out = []

    def at(c, d):
        c.head()
        if d < 64:
            q = len(c) + 64
            c.lit(64, then=q - d)
            c.copy(6, q - d)
        else:
            s = c.pool(16)
            c.protect(s)
            c.lit(s + d - len(c), then=s)
            c.copy(6, s)
        c.lit(4)
        return c.finish(f"dist/d{d}", distance=d)
    for d in DISTANCES:
        out.append(_B([seed, 0, d], lambda c, d=d: at(c, d)))

    def too_far(c):
        c.head()
        s = c.pool(16)
        c.lit(s + 32769 - len(c))
        c.echo(6, s)
        c.lit(4)
        return c.finish("dist/d32769_not_found", distance=32769)
    out.append(_B([seed, 1], too_far))

    def from_zero(c, d):
        c.lit(4)
        c.protect(0)
        if d <= MAX_DISTANCE:
            c.lit(d - 4, then=0)
            c.copy(6, 0)
        else:
            c.lit(d - 4)
            c.echo(6, 0)
        c.lit(4)
        return c.finish(f"dist/source0_at{d}", distance=d)
    for d in (32768, 32769):
        out.append(_B([seed, 2, d], lambda c, d=d: from_zero(c, d)))
    return out


LITERAL_RUNS = (0, 1, 63, 64, 65, 127, 128, 191, 192, 193, 400)


def _two_copies(c, ll, tail=5):
    c.head()
    s = c.pool(32)
    c.protect(s)
    c.protect(s + 12)
    c.lit(5, then=s)
    c.copy(6, s)
    c.lit(ll, then=s + 12)
    c.copy(7, s + 12)
    c.lit(tail)


def literal_runs(seed=4):
    out = [_B([seed, ll], lambda c, ll=ll: (_two_copies(c, ll), c.finish(f"runs/ll{ll}", ll=ll))[1]) for ll in LITERAL_RUNS]
    for tail in (0, 191, 192, 193, 384):    # 0: a final record of 0; 192: a final record of 0 behind a just-sent 192
        out.append(_B([seed, 1, tail], lambda c, t=tail: (_two_copies(c, 3, t), c.finish(f"runs/tail{t}", tail=t))[1]))
    return out


RECORD_COUNTS = (63, 64, 65, 128, 129)


def _unit_walk(name, seed, pool_values, unit_len, lengths, far=None, **tags):
    """pool_values: the pool's bytes as a multiset (laid out here so that every word has a slot of its own);
    unit_len(offset) -> the one length of the unit at that offset of the pool, or None; lengths: the match lengths
    wanted, in order.  far: (offset, length) of one last copy from the pool's offset on, found at its first occurrence
    (no unit starts there), which ends with the chunk."""
    for salt in range(40):
        rng = random.Random(f"{seed}/{salt}")
        left = list(pool_values)
        rng.shuffle(left)
        pool, slots = bytearray(), set()
        while left:                                  # greedy: the next byte completes a word with a new slot
            for k, b in enumerate(left):
                if len(pool) < 3:
                    break
                s = zhash(int.from_bytes(bytes(pool[-3:]) + bytes([b]), "little"))
                if s not in slots:
                    slots.add(s)
                    break
            else:
                break
            pool.append(left.pop(k))
        if left:
            continue
        n0 = len(pool)
        units = {}
        for o in range(n0 - 3):
            L = unit_len(o)
            if L is not None and o + L <= n0 and (far is None or o != far[0]):
                units.setdefault(L, []).append(o)
        behind = {o: pool[o + L] if o + L < n0 else None for L, us in units.items() for o in us}   # the byte behind the latest occurrence
        last = {o: o for us in units.values() for o in us}
        posted = n0 // 64 * 64                       # the first match looks up before the pool's last trip posts
        buf, tokens, copies, prev = bytearray(pool), [], {}, None
        ok = True
        for L in lengths:
            pick = [o for o in units[L] if (prev is None or pool[o] != behind[prev]) and (tokens or o + 4 <= posted)]
            if not pick:
                ok = False
                break
            o = rng.choice(pick)
            if prev is not None:
                behind[prev] = pool[o]
            q = len(buf)
            tokens.append((n0 if not tokens else 0, L, q - last[o]))
            copies[q] = last[o]
            buf += pool[o:o + L]
            last[o], prev = q, o
        if not ok:
            continue
        if far is not None:
            o, L = far
            if buf[o] == behind[prev]:
                continue
            q = len(buf)
            tokens.append((0, L, q - o))
            copies[q] = o
            buf += buf[o:o + L]
        try:
            if mirror(bytes(buf), copies)[0] == tokens:
                return Case(name, buf, tokens, copies, tags)
        except PlanError:
            pass
    raise PlanError(f"{name}: no layout")


def _max_records(seed):
    """256 literals, then 3900 four-byte matches with no literal between"""
    values = list(range(32, 160)) * 2
    return _unit_walk("counts/max_records", seed, values, lambda o: 4, [4] * 3900)


def record_counts(seed=5):
    out = []

    def count(c, m):
        c.head()
        s = c.pool(8 * 130)
        for i in range(m):
            c.protect(s + 8 * i)
        for i in range(m):
            c.lit(1 + i % 3, then=s + 8 * i)
            c.copy(4 + i % 3, s + 8 * i)
        c.lit(3)
        return c
    probe = _B([seed, 0], lambda c: count(c, 10).finish("probe"))
    extra = len(records(probe.tokens, len(probe.content))) - 10      # the head, the pool's literal-only records, the last
    for n in RECORD_COUNTS:
        out.append(_B([seed, n], lambda c, n=n: count(c, n - extra).finish(f"counts/records{n}", records=n)))
    out.append(_max_records([seed, 1]))
    return out


FIBONACCI_LITERALS = (2, 3, 5, 8, 13, 21, 34)    # below them 1 and 1: the end-of-block symbol and one match of FAR_MATCH bytes
FIBONACCI_MATCHES = {11: 55, 10: 89, 9: 144, 8: 233, 7: 377, 6: 610, 5: 987, 4: 1597}
FAR_MATCH = 250                                 # length symbol 284 with 5 extra bits, at a distance with 13
FIBONACCI_VARIANTS = (0, 12, 17)                # orders of the matches; in 12 and 17 the far match reaches a third dword


def alphabets(seed=6):
    out = []
    out.append(_B([seed, 0], lambda c: (c.lit(600), c.finish("alpha/no_match_dynamic"))[1]))

    def one_distance(c):
        c.lit(4, then=0)
        c.copy(100, 0)
        c.lit(400)
        return c.finish("alpha/one_distance_code")
    out.append(_B([seed, 1], one_distance))

    def hlit286(c):
        c.head()
        s = c.pool(300)
        c.protect(s + 2)
        c.lit(300)
        c.lit(5, then=s + 2)
        c.copy(258, s + 2)
        c.lit(200)
        return c.finish("alpha/hlit286")
    out.append(_B([seed, 2], hlit286))
    # (HDIST 30: dist/d24577 .. dist/d32768)
    # every used literal 16 times: rank_of breaks nothing but ties
    for salt in range(40):
        rng = random.Random(f"ties/{seed}/{salt}")
        content = b"".join(bytes(rng.sample(range(40, 104), 64)) for _ in range(16))
        try:
            out.append(_fixed("alpha/all_literals_of_one_frequency", content))
            break
        except PlanError:
            pass
    # the 15-bit limit: 17 symbols in Fibonacci proportion, 1 (end of block) 1 (the far match) 2 .. 34 (literals) 55 ..
    # 1597 (match lengths).  The far match is the last token: a code of 15 + 5 bits and a rare distance code with 13,
    # the longest code a stream here holds; the variants differ in the order of the matches, which moves it through
    # the alignments of the bit stage
    values = [b for v, n in enumerate(FIBONACCI_LITERALS) for b in [97 + v] * n]
    lens = sorted(FIBONACCI_MATCHES)
    unit_len = lambda o: lens[(o * 5) % 11 % 8] if 0 < o < 75 else None     # noqa: E731
    for v in FIBONACCI_VARIANTS:
        want = [L for L, n in FIBONACCI_MATCHES.items() for _ in range(n)]
        random.Random(f"fib/{seed}/{v}").shuffle(want)
        out.append(_unit_walk(f"alpha/fibonacci_15_bit_limit_v{v}", [seed, 3, v], values, unit_len, want, far=(0, FAR_MATCH), variant=v))
    # runs of the code-length stream: 16, 17 and 18, each with its fewest and its most repeats
    used = [0, 4, 15, 27, 166] + list(range(170, 174)) + list(range(180, 187))
    for salt in range(40):
        rng = random.Random(f"runs/{seed}/{salt}")
        content = b"".join(bytes(rng.sample(used, 16)) for _ in range(16))
        try:
            out.append(_fixed("alpha/code_length_runs", content))
            break
        except PlanError:
            pass
    return out


TIE_SEED, TIE_CANDIDATES = 1951, 3000
TIES = (396, 1696, 2321)   # indices into tie_candidates() whose dynamic and fixed costs are equal (filled from the search)


def tie_candidates():
    """small random chunks around the size at which a dynamic block begins to pay (fixed seed)"""
    rng = random.Random(TIE_SEED)
    out = []
    for k in range(TIE_CANDIDATES):
        n = rng.randrange(24, 120)
        alpha = rng.sample(range(32, 127), rng.randrange(4, 20))
        b = bytearray(rng.choice(alpha) for _ in range(n))
        if k % 2:
            at = rng.randrange(4, n)
            b[at:at] = b[:rng.randrange(4, 12)]
        out.append(bytes(b))
    return out


def choice(seed=7):
    out = []
    out.append(_B([seed, 0], lambda c: (c.lit(300), c.finish("choice/stored_below_fixed"))[1], alphabet=Z.FLAT))
    out.append(_B([seed, 1], lambda c: (c.lit(4, then=0), c.copy(20, 0), c.finish("choice/fixed_below_dynamic"))[2]))
    out.append(_B([seed, 2], lambda c: (c.head(), c.lit(900), c.finish("choice/dynamic_smallest"))[2]))
    # 3 + 30 * 9 + 7 = 280 = 8 * (30 + 5); every third value, so that the lengths of a dynamic block do not fold into runs
    out.append(_fixed("choice/fixed_equals_stored", bytes(range(150, 240, 3))))
    cands = tie_candidates()
    for k in TIES:
        out.append(_unplanned(f"choice/dynamic_equals_fixed_{k}", cands[k], tie=k))
    rng = np.random.default_rng([seed, 3])
    noise = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    out.append(_unplanned("choice/stored_65535", noise[:65535], blocks=1))
    out.append(_unplanned("choice/stored_65536", noise, blocks=2))
    return out


def bit_stage(seed=8):
    out = []
    # 10 + 8 a + 9 b bits as a fixed block: every residue mod 32
    for a in (4, 5):
        for b in range(30):
            out.append(_fixed(f"bits/fixed_a{a}_b{b}", b"abcde"[:a] + bytes(range(150, 150 + b)), a=a, b=b))
    return out


def unplanned(seed=9):
    import test_deflate_compress_gpu as T
    out = []
    kinds = T.inputs()
    for name, data in kinds.items():
        for size in (257, 4096):
            cut = data[:size]
            if len(cut) == size:
                out.append(_unplanned(f"generic/{name}_{size}", cut))
    out.append(_unplanned("generic/text_65536", kinds["text"][:65536]))
    out.append(_unplanned("generic/sorted_int32_65536", kinds["sorted_int32"][:65536]))
    for name, data in T.match_edges().items():
        if len(data) <= 4096:
            out.append(_unplanned(f"generic/{name}", data))
    return out


FAMILIES = {"trip_edges": trip_edges, "match_extension": match_extension, "distances": distances,
            "literal_runs": literal_runs, "record_counts": record_counts, "alphabets": alphabets, "choice": choice,
            "bit_stage": bit_stage, "unplanned": unplanned}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def all_cases():
    """every case of every family, built once"""
    return [c for name in FAMILIES for c in family(name)]


def job_file(content: bytes, tokens) -> bytes:
    """the file of the driver's `encode @FILE`"""
    return struct.pack("<II", len(content), len(tokens)) + content + b"".join(struct.pack("<III", *t) for t in tokens)
