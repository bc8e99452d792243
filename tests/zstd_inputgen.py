"""Planned INPUTS for the Zstandard encoder (plain Python and numpy, no GPU, nothing read from the kernel sources).

tests/zstd_framegen.py writes frames for the decoders; this module writes chunks for the encoder, each from an
explicit plan of steps: k literal bytes, or a copy of L bytes from a chosen earlier position.  A case carries the
token list (literal run, match length, offset) the plan intends, and parse(), a small mirror of the parse rule as
DESIGN.md section 17 and the kernel's comments state it, must return exactly that list for every planned case
(tests/test_zstd_inputgen_cpu.py); the kernel must too (tests/test_zstd_encoder_edges_gpu.py).

The rule that parse() mirrors:
  * hash(v) = ((v * 0x9E3779B1) & 0xFFFFFFFF) >> 20; 4096 entries of 16-bit positions, cleared to 0: position 0 is a
    candidate like any other, and a candidate must lie before the looking position;
  * a trip starts at pos; lane j looks the word at pos + j up if pos + j <= len - 4.  All lookups of a trip happen
    before any post of that trip, so a source in the same trip as its copy is not seen -- unless it is position 0,
    which every empty slot names;
  * t is the first lane whose candidate's word equals its own, min(len - pos, 64) without a hit; lanes <= t that
    have a word post their position; a match is extended until a byte differs or the chunk ends, and the next trip
    starts at its end (at pos + t without a hit).
Where two posting lanes of one trip share a slot, which of them stays is the hardware's rule: parse() keeps both
and raises PlanError if that ever matters -- a planned source among them, or one of them holding the looking lane's
word.  It also raises where a planned source is not the candidate its copy reads (overwritten, or never posted).
Every other sharing is harmless: a candidate with a different word is rejected either way.

What makes the outcome known by construction: literal bytes are drawn one at a time and rejected until the word
they complete occurs nowhere earlier (also across a literal/copy boundary: the last literal in front of a copy is
drawn knowing the copy's first bytes) and does not hash to a slot that holds a source still to be used
(protect()); the literal behind a copy differs from the byte behind its source, and a copy's first byte from the
byte behind the source of a copy that ends where it starts.  Where a plan cannot be laid out, or parse() does not
return the plan, the case is built again with the next salt of its seed (deterministic).

Literal runs are drawn from a skewed alphabet of 32 values, so that Huffman literals pay and a block with a long
literal run stays compressed; small cases begin with head(): four literals and a long copy of position 0, which
pays for the block and ends on a known trip start.

What no input reaches (the scalar encoder's token lists in tests/test_zstd_codes_cpu.py do):
  * ml 65535 and nlit 1: one literal and a match at offset 1 to the end is a chunk of equal bytes, an RLE_Block.
    The longest match here is 65534 (ML code 51 with 15 extra bits), the fewest literals 2.
  * the same offset twice with no literal between: the first match would have gone on.  That case is here as a
    token list for the scalar encoder alone (scalar_only).
"""
from __future__ import annotations

import numpy as np

import zstd_framegen as G

M32 = 0xFFFFFFFF
MAX_CHUNK = 65536


def zhash(v: int) -> int:
    return ((v * 0x9E3779B1) & M32) >> 20


class PlanError(Exception):
    pass


def _alphabet(values, ratio):
    p = ratio ** np.arange(len(values), dtype=np.float64)
    return np.array(values, dtype=np.int64), p / p.sum()


LOW = _alphabet(range(1, 33), 0.88)        # skewed, 32 values below 128: Huffman pays, the tree can be described directly
HIGH = _alphabet(range(200, 232), 0.88)    # the same at values above 127: only the FSE description of the weights
WIDE = _alphabet(range(32, 96), 0.97)      # 64 values, for chunks that need many distinct words around few bytes
FLAT = _alphabet(range(256), 1.0)          # incompressible


class Case:
    """name; content; tokens [(ll, ml, offset)] the plan intends (None: not planned, the parse is the encoder's);
    copies {position: source}; scalar_only: a token list no parse gives, for the scalar encoder alone"""

    def __init__(self, name, content, tokens, copies=None, tags=None, scalar_only=False):
        self.name, self.content, self.tokens = name, bytes(content), tokens
        self.copies = dict(copies or {})
        self.tags = dict(tags or {})
        self.scalar_only = scalar_only
        self.family = name.split("/")[0]

    def scalar_tokens(self):
        return self.tokens or []


# ------------------------------------------------------------------------------------------------------ the mirror

def _words(data: bytes):
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    w = a[:-3] | (a[1:-2] << np.uint64(8)) | (a[2:-1] << np.uint64(16)) | (a[3:] << np.uint64(24))
    h = ((w * np.uint64(0x9E3779B1)) & np.uint64(M32)) >> np.uint64(20)
    return w.tolist(), h.tolist()


def _match_length(data: bytes, mp: int, dist: int, max_match=None) -> int:
    """bytes from mp on that equal those dist before them, to the chunk's end or to max_match"""
    n, done, step = len(data), 4, 64
    if max_match is not None:
        n = min(n, mp + max_match)
    while mp + done < n:
        k = min(step, n - mp - done)
        a, b = data[mp + done:mp + done + k], data[mp + done - dist:mp + done - dist + k]
        if a != b:
            d = np.flatnonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8))
            return done + int(d[0])
        done += k
        step *= 4
    return done


def parse(data: bytes, copies=None, max_match=None, max_distance=None):
    """The encoder's parse of `data`: -> [(ll, ml, offset)], None where no parse runs (fewer than 4 bytes, or all
    bytes equal: Zstandard's RLE_Block).  copies: {position: planned source}, checked as the module's docstring says.
    max_match, max_distance: the Deflate encoder's form of the rule (tests/deflate_inputgen.py) -- a candidate
    further back than max_distance is no hit, a match stops at max_match and the next trip starts at its end, so the
    same distance can follow with no literal between; all bytes equal are parsed like any others."""
    n = len(data)
    if n <= 3 or (max_match is None and data == data[:1] * n):
        return None
    copies = copies or {}
    w, h = _words(data)
    table, ever = {}, set()
    tokens, pos, pend = [], 0, 0
    while pos < n:
        in_window = min(64, n - pos)
        hit = cand = -1
        for j in range(in_window):
            my = pos + j
            if my > n - 4:
                break
            c = table.get(h[my], 0)
            want = copies.get(my)
            if type(c) is tuple:
                if want is not None:
                    raise PlanError(f"the source {want} of the copy at {my} " + (
                        "shared its slot with another posting lane of its trip" if want in c else "was overwritten"))
                if any(p < my and w[p] == w[my] and (max_distance is None or my - p <= max_distance) for p in c):
                    raise PlanError(f"the word at {my} has two candidates that the hardware chooses between")
                continue
            if want is not None and c != want:
                raise PlanError(f"the source {want} of the copy at {my} " + ("was overwritten" if want in ever else "was never posted"))
            if c < my and w[c] == w[my] and (max_distance is None or my - c <= max_distance):
                hit, cand = j, c
                break
        t = in_window if hit < 0 else hit
        posts = {}
        for j in range(min(t, 63) + 1):
            my = pos + j
            if my > n - 4:
                break
            posts[h[my]] = posts.get(h[my], ()) + (my,)
        for slot, who in posts.items():
            table[slot] = who[0] if len(who) == 1 else who
            ever.update(who)
        if hit >= 0:
            mp = pos + t
            dist = pos + hit - cand
            ml = _match_length(data, mp, dist, max_match) if mp + 4 <= n else 4
            tokens.append((pend + t, ml, dist))
            pend, pos = 0, mp + ml
        else:
            pend += t
            pos += t
    return tokens


def rebuilds(content: bytes, tokens) -> bool:
    """the tokens are this content's: every match copies what stands `offset` before it"""
    a = np.frombuffer(content, dtype=np.uint8)
    pos = 0
    for ll, ml, off in tokens:
        pos += ll
        if off < 1 or off > pos or pos + ml > len(content) or not np.array_equal(a[pos:pos + ml], a[pos - off:pos + ml - off]):
            return False
        pos += ml
    return pos <= len(content)


def maximal(content: bytes, tokens) -> bool:
    """no match could have gone on: it ends with the chunk or at a byte that differs"""
    pos = 0
    for ll, ml, off in tokens:
        pos += ll + ml
        if pos < len(content) and content[pos] == content[pos - off]:
            return False
    return True


def copy_positions(tokens):
    out, pos = [], 0
    for ll, ml, off in tokens:
        out.append(pos + ll)
        pos += ll + ml
    return out


def literals_of(content: bytes, tokens) -> bytes:
    out, pos = bytearray(), 0
    for ll, ml, off in tokens:
        out += content[pos:pos + ll]
        pos += ll + ml
    return bytes(out + content[pos:])


# ------------------------------------------------------------------------------------------------------ the builder

class Chunk:
    def __init__(self, seed, alphabet=LOW, max_match=None, max_distance=None):
        self.rng = np.random.default_rng(seed)
        self.alpha = alphabet
        self.max_match, self.max_distance = max_match, max_distance
        self.buf = bytearray()
        self.words = set()         # every 4-byte word of the chunk so far
        self.used = set()          # their slots
        self.reserved = set()      # slots that hold a source still to be used
        self.tokens, self.copies = [], {}
        self.run = 0               # literals since the last copy
        self.forbid = None         # the next byte must differ from this one
        self.trip0 = 0             # a position where a trip is known to start
        self._draws = []

    def __len__(self):
        return len(self.buf)

    def word(self, i):
        return int.from_bytes(self.buf[i:i + 4], "little")

    def _draw(self):
        if not self._draws:
            values, p = self.alpha
            self._draws = self.rng.choice(values, 4096, p=p).tolist()
        return self._draws.pop()

    def _see(self, frm):
        for s in range(max(frm, 0), len(self.buf) - 3):
            w = self.word(s)
            self.words.add(w)
            self.used.add(zhash(w))

    def _boundary_ok(self, b, src):
        """with b as the last literal in front of a copy from src: the words that start in the literals and end in
        the copy are new and leave the reserved slots alone"""
        n = len(self.buf)
        lo = max(0, n - 2)
        ext = bytearray(self.buf[lo:]) + bytes([b])
        for i in range(3):
            p = src + i
            ext.append(self.buf[p] if p < n else ext[p - lo])
        seen = set()
        for s in range(len(ext) - 3):
            w = int.from_bytes(ext[s:s + 4], "little")
            if w in self.words or w in seen or zhash(w) in self.reserved:
                return False
            seen.add(w)
        return True

    def lit(self, k, then=None, fresh=False):
        """k literal bytes.  then: the source of the copy that follows them; fresh: every word gets a slot that no
        word of the chunk has had (a pool of sources: no two of them share one)."""
        for j in range(k):
            n = len(self.buf)
            base = int.from_bytes(self.buf[n - 3:n], "little") if n >= 3 else None
            last = then is not None and j == k - 1
            for _ in range(600):
                b = self._draw()
                if b == self.forbid:
                    continue
                if base is not None:
                    w = base | (b << 24)
                    if w in self.words:
                        continue
                    s = zhash(w)
                    if s in self.reserved or (fresh and s in self.used):
                        continue
                if last and not self._boundary_ok(b, then):
                    continue
                break
            else:
                raise PlanError(f"no byte completes a new word at {n} (literal {j} of {k})")
            self.buf.append(b)
            self.forbid = None
            self._see(n - 3)
        self.run += k
        return len(self.buf) - k

    def protect(self, pos):
        """the word at pos is a source still to be used: no later literal word takes its slot"""
        assert pos + 4 <= len(self.buf)
        self.reserved.add(zhash(self.word(pos)))
        return pos

    def copy(self, L, src):
        """a copy of L >= 4 bytes from position src (it may run into itself): the token (literals so far, L, offset).
        With max_match a longer copy is as many tokens as it takes, the later ones behind no literal; fewer than 4
        bytes left over are literals of the next run."""
        q = len(self.buf)
        assert L >= 4 and 0 <= src < q and q + L <= MAX_CHUNK
        assert self.max_distance is None or q - src <= self.max_distance
        if self.forbid is not None and self.buf[src] == self.forbid:
            raise PlanError("the copy's first byte is the one that has to differ")
        for i in range(L):
            self.buf.append(self.buf[src + i])
        for s in range(max(q - 3, q - self.run, 0), q):       # the words that start in the literals in front of it
            w = self.word(s)
            if w in self.words or zhash(w) in self.reserved:
                raise PlanError("a literal word that the copy completes occurs earlier or takes a source's slot")
        self._see(q - 3)
        step = L if self.max_match is None else self.max_match
        for done in range(0, L, step):
            piece = min(step, L - done)
            if piece < 4:
                self.run = piece
                break
            self.tokens.append((self.run, piece, q - src))
            self.copies[q + done] = src + done
            self.run = 0
        self.forbid = self.buf[src + L]
        self.trip0 = q + L
        return q

    def echo(self, n, src):
        """n literal bytes equal to those at src, which the plan says the encoder does NOT find"""
        q = len(self.buf)
        if self.forbid is not None and self.buf[src] == self.forbid:
            raise PlanError("the first byte has to differ")
        for i in range(n):
            self.buf.append(self.buf[src + i])
        self._see(q - 3)
        self.run += n
        self.forbid = self.buf[src + n]
        return q

    def head(self, L=100):
        """four literals and a copy of position 0 (every empty slot names it): pays for the block, and the next trip
        starts at its end"""
        assert not self.buf
        self.lit(4, then=0)
        self.copy(L, 0)

    def lane(self):
        return (len(self.buf) - self.trip0) % 64

    def pool(self, n):
        """whole trips of literals without a hit, at least n bytes, from the next trip start on: -> where they start.
        Their words all have slots of their own, so any of them can be a source."""
        if self.lane():
            self.lit(64 - self.lane())
        at = len(self.buf)
        self.lit((n + 63) // 64 * 64, fresh=True)
        return at

    def finish(self, name, **tags):
        if len(self.buf) > MAX_CHUNK:
            raise AssertionError(f"{name}: {len(self.buf)} bytes")
        return Case(name, self.buf, list(self.tokens), self.copies, tags)


def _build(seed, fn, alphabet=LOW, tries=60, max_match=None, max_distance=None):
    """fn(Chunk) -> Case whose plan parse() confirms, with the next salt of the seed whenever it does not"""
    err = None
    for salt in range(tries):
        try:
            case = fn(Chunk(list(seed) + [salt], alphabet, max_match, max_distance))
            got = parse(case.content, case.copies, max_match, max_distance)
            if got != case.tokens and not (got is None and not case.tokens):
                raise PlanError(f"{case.name}: the parse differs from the plan")
            return case
        except PlanError as e:
            err = e
    raise PlanError(f"no layout in {tries} salts: {err}")


def _unplanned(name, content, **tags):
    """a chunk without a plan: its tokens are the mirror's where no lookup of it is ambiguous, else the encoder's"""
    try:
        tokens = parse(content)
        tokens = [] if tokens is None else tokens
    except PlanError:
        tokens = None
    return Case(name, content, tokens, tags=tags)


# ------------------------------------------------------------------------------------------------------ the families

def trip_edges(seed=1):
    out = []

    def near(c, k, L, tail):
        c.head()
        s = c.pool(80)
        c.protect(s + 5)
        c.lit(k, then=s + 5)
        c.copy(L, s + 5)
        c.lit(tail)
    for k in (0, 1, 62, 63):
        out.append(_build([seed, 0, k], lambda c, k=k: (near(c, k, 9, 7), c.finish(f"trip/hit_lane{k}", hit_lane=k))[1]))
    for tail in (1, 2, 3, 4, 10):    # 1 .. 3: positions without a word; 10: a short last window without a hit
        out.append(_build([seed, 1, tail], lambda c, t=tail: (near(c, 5, 6, t), c.finish(f"trip/tail{t}", tail=t))[1]))
    out.append(_build([seed, 2], lambda c: (near(c, 5, 4, 0), c.finish("trip/match_at_len_minus_4"))[1]))

    def same_trip(c):
        c.head()
        a = len(c)
        c.lit(10)
        c.echo(6, a + 2)             # its source is posted only behind this trip's lookups
        c.lit(20)
        return c.finish("trip/source_in_the_same_trip")
    out.append(_build([seed, 3], same_trip))

    def trip_before(c):
        c.head()
        s = c.pool(64)
        c.protect(s + 60)
        c.lit(3, then=s + 60)
        c.copy(8, s + 60)
        c.lit(6)
        return c.finish("trip/source_in_the_trip_before")
    out.append(_build([seed, 4], trip_before))
    return out


MATCH_LENGTHS = (4, 5, 67, 68, 69, 131, 132)


def match_extension(seed=2):
    out = []

    def one(c, L, by_byte):
        c.head()
        s = c.pool(L + 16)
        c.protect(s + 2)
        c.lit(5, then=s + 2)
        c.copy(L, s + 2)
        if by_byte:
            c.lit(9)
        return c.finish(f"extend/L{L}_{'byte' if by_byte else 'end'}", L=L, by_byte=by_byte)
    for L in MATCH_LENGTHS:
        for by_byte in (True, False):
            out.append(_build([seed, L, by_byte], lambda c, L=L, b=by_byte: one(c, L, b)))

    def overlap(c, d, L):
        c.head()
        q = len(c) + 64
        c.lit(64, then=q - d)        # a whole trip: the source is lane 64 - d of the trip before the copy's
        c.copy(L, q - d)
        c.lit(6)
        return c.finish(f"extend/offset{d}_L{L}", offset=d)
    for d in (1, 2, 3):
        for L in (4, 70):
            out.append(_build([seed, 100 + d, L], lambda c, d=d, L=L: overlap(c, d, L)))
    return out


LITERAL_RUNS = (0, 1, 63, 64, 65, 128, 129)


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


def literal_runs(seed=3):
    return [_build([seed, ll], lambda c, ll=ll: (_two_copies(c, ll), c.finish(f"runs/ll{ll}", ll=ll))[1]) for ll in LITERAL_RUNS]


LL_CODES, ML_CODES, OF_CODES = range(16, 35), range(32, 52), range(2, 16)


def code_boundaries(seed=4):
    out = []
    for code in LL_CODES:
        for ll in (G.LL_BASE[code], G.LL_BASE[code] - 1):
            out.append(_build([seed, 0, ll], lambda c, ll=ll: (_two_copies(c, ll, 3), c.finish(f"codes/ll{ll}", ll=ll))[1]))

    def long_match(c, ml):
        c.head()
        q = len(c) + 64
        c.lit(64, then=q - 7)
        c.copy(ml, q - 7)
        c.lit(4)
        return c.finish(f"codes/ml{ml}", ml=ml)
    for code in ML_CODES:
        for ml in (G.ML_BASE[code], G.ML_BASE[code] - 1):
            out.append(_build([seed, 1, ml], lambda c, ml=ml: long_match(c, ml)))

    def offset(c, off):
        c.head()
        if off < 64:
            q = len(c) + 64
            c.lit(64, then=q - off)
            c.copy(6, q - off)
        else:
            s = c.pool(16)
            c.protect(s)
            c.lit(s + off - len(c), then=s)
            c.copy(6, s)
        c.lit(4)
        return c.finish(f"codes/offset{off}", offset=off)
    offs = sorted({o for code in OF_CODES for o in ((1 << code) - 3, (1 << code) - 4) if o >= 1})
    for off in offs:
        out.append(_build([seed, 2, off], lambda c, off=off: offset(c, off)))

    def largest_run(c):              # ll 65532 and offset 65532 at once: a 4-byte copy of the chunk's head
        c.lit(4)
        c.protect(0)
        c.lit(65528, then=0)
        c.copy(4, 0)
        return c.finish("codes/ll65532_offset65532", ll=65532, offset=65532)
    out.append(_build([seed, 3], largest_run))
    # the longest match a parse can find: one more byte and the chunk is an RLE_Block
    out.append(Case("codes/ml65534", b"y" * 65535 + b"x", [(1, 65534, 1)], {1: 0}, {"ml": 65534}))
    return out


def _cycle(c, nseq, K, ll_of, L_of, rank_of, special=None):
    """nseq sequences over a pool of K four-byte words at the chunk's head: sequence i copies L_of(i) bytes from
    the latest occurrence -- the pool's, then the copy before -- of the word that was used rank_of(i) words ago,
    behind ll_of(i) literals: a low rank is a near offset, and every word is used about as often as any other (the
    literal in front of a word has to differ every time).  special: {i: fn(c)} lays sequence i itself, from word 0,
    which is then no one else's."""
    assert not c.buf and K % 16 == 0
    c.lit(4 * K, fresh=True)
    last = [c.protect(4 * i) for i in range(K)]
    mru = list(range(1 if special else 0, K))
    for i in range(nseq):
        if special and i in special:
            special[i](c)
            continue
        ll, L, r = ll_of(i), L_of(i), rank_of(i) % len(mru)
        if ll == 0:
            for _ in range(len(mru)):   # (the copy's first byte must differ from the byte behind the last source)
                if c.forbid is None or c.buf[last[mru[r]]] != c.forbid:
                    break
                r = (r + 1) % len(mru)
        p = mru.pop(r)
        mru.insert(0, p)
        c.lit(ll, then=last[p])
        last[p] = c.copy(L, last[p])


SEQUENCE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192)
MANY_SEQUENCES = 8200


def sequence_counts(seed=5):
    out = []

    def count(c, n):
        c.head()
        if n > 1:
            s = c.pool(8 * n)
            for i in range(n - 1):
                c.protect(s + 8 * i)
            for i in range(n - 1):
                c.lit(1 + i % 3, then=s + 8 * i)
                c.copy(4 + i % 3, s + 8 * i)
        c.lit(3)
        return c.finish(f"counts/n{n}", nseq=n)
    for n in SEQUENCE_COUNTS:
        out.append(_build([seed, n], lambda c, n=n: count(c, n)))

    def many(c):
        _cycle(c, MANY_SEQUENCES, 512, lambda i: 1, lambda i: 4, lambda i: -1)
        c.lit(2)
        return c.finish(f"counts/n{MANY_SEQUENCES}", nseq=MANY_SEQUENCES)
    out.append(_build([seed, MANY_SEQUENCES], many, alphabet=WIDE, tries=8))
    return out


def table_modes(seed=6):
    """RLE for each of the three tables (predefined and described tables come with the other families)"""
    out = []

    def ll_ml_rle(c):                # every sequence (4, 8, .): block j copies from the second literal of block j - 1
        c.lit(4, then=0)
        c.copy(8, 0)
        for j in range(1, 30):
            q = len(c) + 4
            c.lit(4, then=q - 15)
            c.copy(8, q - 15)
        return c.finish("modes/ll_rle_ml_rle")
    out.append(_build([seed, 0], ll_ml_rle))

    def of_rle(c):                   # every Offset_Value has code 9 and none repeats; every match has 5 bytes
        c.lit(640, fresh=True)
        for i in range(24):
            ll = 2 + i % 3
            src = len(c) + ll - (520 + 4 * i)
            c.lit(ll, then=src)
            c.copy(5, src)
        c.lit(3)
        return c.finish("modes/of_rle_ml_rle")
    out.append(_build([seed, 1], of_rle))
    return out


def repeat_rule(seed=7):
    out = []

    def with_literals(c):            # the same offset twice, two literals between: Offset_Value 1
        c.head()
        s = c.pool(32)
        c.protect(s)
        c.lit(3, then=s)
        c.copy(5, s)
        c.lit(2, then=s + 7)
        c.copy(5, s + 7)
        c.lit(4)
        assert c.tokens[-1][2] == c.tokens[-2][2]
        return c.finish("repeat/same_offset_behind_literals")
    out.append(_build([seed, 0], with_literals))

    def first_offset_1(c):           # the first sequence at offset 1: written as 4, not as the repeat code
        c.lit(1)
        c.copy(40, 0)
        c.lit(30)
        return c.finish("repeat/first_sequence_offset_1")
    out.append(_build([seed, 1], first_offset_1))
    # no parse gives this one: the first match would have gone on
    tokens = [(5, 4, 5), (0, 6, 5), (2, 4, 5)]
    lits = bytes(np.random.default_rng([seed, 2]).choice(LOW[0], 40).tolist())
    content, at = bytearray(), 0
    for ll, ml, off in tokens:
        content += lits[at:at + ll]
        at += ll
        for _ in range(ml):
            content.append(content[-off])
    content += lits[at:]
    out.append(Case("repeat/same_offset_without_literals", content, tokens, scalar_only=True))
    return out


LITERAL_COUNTS = (2, 31, 32, 1023, 1024, 1025, 1026, 1027, 4095, 4096, 16383, 16384)


def fibonacci_literals(seed):
    """21 byte values with Fibonacci counts (28656 bytes), shuffled: Huffman's own code is 20 bits deep"""
    a, b, out = 1, 1, []
    for s in range(21):
        out += [65 + s] * a
        a, b = b, a + b
    return bytes(np.random.default_rng(seed).permutation(np.array(out, dtype=np.uint8)).tolist())


def literal_forms(seed=8):
    out = []

    def section(c, nlit, name):
        if nlit < 4:
            c.lit(nlit, then=0)
            c.copy(100, 0)
        else:
            c.head()
            c.lit(nlit - 4)
        return c.finish(name, nlit=nlit)
    for k, (label, alpha) in enumerate((("compressible", LOW), ("incompressible", FLAT))):
        for nlit in LITERAL_COUNTS:
            out.append(_build([seed, k, nlit], lambda c, n=nlit, l=label: section(c, n, f"literals/{l}_{n}"), alphabet=alpha))
    out.append(_build([seed, 2], lambda c: section(c, 3000, "literals/high_values_3000"), alphabet=HIGH))
    out.append(_unplanned("literals/fibonacci_counts", fibonacci_literals([seed, 3]), deep_tree=True))
    return out


FAT_SEQUENCES = 2100


def fat_sequences(seed=9):
    """Chunks of 2100 varied sequences, so that the three tables are described with their largest logs, and among them
    one that carries a rare LL code with 13, 14 or 15 extra bits, the rarest offset code and a rare match length code
    at once; v varies what is written in front of it (the sequences behind it)."""
    out = []

    def fat(c, bits, v):
        rng = np.random.default_rng([seed, 77, bits, v])
        lls = rng.choice([0, 1, 2, 3, 4, 5, 7, 9, 12, 17, 19, 26, 41], FAT_SEQUENCES, p=[.1, .2, .2, .12, .1, .08, .06, .05, .03, .02, .02, .01, .01])
        Ls = rng.choice([4, 5, 6, 7, 8, 10, 13, 21, 36, 52], FAT_SEQUENCES, p=[.3, .2, .15, .1, .08, .06, .05, .03, .02, .01])
        picks = np.minimum(rng.geometric(0.04, FAT_SEQUENCES) * rng.choice([1, 1, 2, 5], FAT_SEQUENCES), 126)
        at = FAT_SEQUENCES - 2 - 7 * v - bits

        def the_fat_one(c):          # word 0 of the pool is no one else's: the farthest source and 300 bytes behind it
            c.lit((1 << bits) + (6000 if bits == 15 else 1 << (bits - 1)) + 37 * v + 1, then=0)   # (high extra bits set)
            c.copy(300 + v, 0)
        _cycle(c, FAT_SEQUENCES, 128, lambda i: int(lls[i]), lambda i: int(Ls[i]), lambda i: int(picks[i]), {at: the_fat_one})
        c.lit(5)
        return c.finish(f"fat/extra{bits}_v{v}", nseq=FAT_SEQUENCES, fat_at=at)
    for bits in (13, 14, 15):
        for v in range(6):
            out.append(_build([seed, bits, v], lambda c, b=bits, v=v: fat(c, b, v), alphabet=WIDE, tries=12))

    def hundreds(c, v):              # several hundred sequences: smaller logs
        rng = np.random.default_rng([seed, 78, v])
        n = 300 + 100 * v
        lls, Ls, picks = rng.integers(0, 24, n), rng.integers(4, 40, n), rng.integers(1, 64, n)
        _cycle(c, n, 64, lambda i: int(lls[i]), lambda i: int(Ls[i]), lambda i: int(picks[i]),
               {n - 9: lambda c: (c.lit(8192 + 17 * v, then=0), c.copy(150, 0))})
        c.lit(3)
        return c.finish(f"fat/hundreds_v{v}", nseq=n)
    for v in range(3):
        out.append(_build([seed, 100, v], lambda c, v=v: hundreds(c, v), alphabet=WIDE, tries=12))
    return out


def block_limit(seed=10):
    """About 300 near-incompressible bytes with one to five short copies, the first copy's length swept: the block
    comes out a few bytes below, at, or above the chunk's size, so some are kept and their neighbours fall back."""
    out = []

    def one(c, ncopy, L0):
        c.lit(64, fresh=True)
        c.lit(150, then=8)
        c.copy(L0, 8)
        for j in range(1, ncopy):
            c.lit(10, then=8 + 12 * j)
            c.copy(4, 8 + 12 * j)
        c.lit(300 - len(c))
        return c.finish(f"limit/copies{ncopy}_L{L0}", ncopy=ncopy, L0=L0)
    for ncopy in range(1, 6):
        for L0 in range(4, 20):
            out.append(_build([seed, ncopy, L0], lambda c, n=ncopy, L=L0: one(c, n, L), alphabet=FLAT))
    return out


NEAR_RLE_LENGTHS = (2, 3, 4, 64, 65, 129, 65536)


def near_rle(seed=11):
    """all bytes equal but one: the all-equal check must see the one wherever it lies"""
    out, seen = [], set()
    for n in NEAR_RLE_LENGTHS:
        for idx in (1, 63, 64, 65, n - 1):
            if idx < n and (n, idx) not in seen:
                seen.add((n, idx))
                b = bytearray(b"a" * n)
                b[idx] = ord("b")
                out.append(_unplanned(f"near_rle/len{n}_at{idx}", bytes(b), n=n, idx=idx))
    out.append(_unplanned("near_rle/three_unequal", b"abc"))
    out.append(_unplanned("near_rle/two_equal", b"aa"))
    return out


FAMILIES = {"trip_edges": trip_edges, "match_extension": match_extension, "literal_runs": literal_runs,
            "code_boundaries": code_boundaries, "sequence_counts": sequence_counts, "table_modes": table_modes,
            "repeat_rule": repeat_rule, "literal_forms": literal_forms, "fat_sequences": fat_sequences,
            "block_limit": block_limit, "near_rle": near_rle}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def all_cases():
    """every case of every family, built once"""
    return [c for name in FAMILIES for c in family(name)]


def kernel_cases():
    """those a parse can give (not the scalar encoder's alone)"""
    return [c for c in all_cases() if not c.scalar_only]
