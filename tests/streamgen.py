"""Seeded generator of valid LZ4 and Snappy streams in every legal token form (CPU only: plain Python and numpy).

The project's encoders emit a narrow set of token shapes; the decoders promise to decode any valid stream.  Every
stream here is written from an explicit plan -- LZ4: a list of Seq(literal bytes, match length, offset, run),
Snappy: a list of elements -- and every plan is valid by construction (nothing is drawn and then discarded).  A
family is a function of (seed, count, size) that returns [(stream, expected output, plan)]; the expected output
comes from the plan alone through the plainest loop there is (expected_lz4 / expected_snappy: matches one byte at a
time, out.append(out[-offset])), which shares no code with the oracle or the kernels.

LZ4 streams never carry offset 0 (the project rejects it).  `conforming` chooses between streams that keep the LZ4
block format's end rules (the last 5 bytes are literals, the last match starts at least 12 bytes before the end:
liblz4 decodes them) and streams that the reference decoder accepts but liblz4 does not (ending in a match or in a
literal-only token of any length, the empty one included).

Used by tests/test_streamgen_cpu.py (the generator against the oracle and liblz4, and its census),
tests/test_decoder_token_forms_gpu.py (the batched decoders against expected_*) and scripts/fuzz_decoders.py.
"""
from __future__ import annotations

import ctypes
import functools
from collections import namedtuple

import numpy as np

import datagen

# ============================================================================================== LZ4

Seq = namedtuple("Seq", "lit ml off run")   # literal bytes; match length (0: none, last sequence only); offset;
                                            # run: id of the short-sequence run it belongs to (-1: none)


def lsic(n: int) -> bytes:
    """LZ4's linear small-integer code: 255 while n >= 255, then the rest."""
    return b"\xff" * (n // 255) + bytes([n % 255])


def encode_lz4(plan) -> bytes:
    out = bytearray()
    for s in plan:
        nl = len(s.lit)
        m = s.ml - 4 if s.ml else 0
        out.append((min(nl, 15) << 4) | min(m, 15))
        if nl >= 15:
            out += lsic(nl - 15)
        out += s.lit
        if s.ml:
            out += s.off.to_bytes(2, "little")
            if m >= 15:
                out += lsic(m - 15)
    return bytes(out)


def expected_lz4(plan) -> bytes:
    """The plan's output, one byte at a time."""
    out = bytearray()
    for s in plan:
        out += s.lit
        for _ in range(s.ml):
            out.append(out[-s.off])
    return bytes(out)


class _LZ4:
    """A plan being written; every sequence is checked for validity as it is added."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.plan = []
        self.n = 0          # output bytes so far
        self.runs = 0

    def bytes(self, k):
        return bytes(self.rng.integers(0, 256, k, dtype=np.uint8))

    def r(self, lo, hi):   # inclusive
        return int(self.rng.integers(lo, hi + 1))

    def seq(self, nlit, ml, off, run=-1):
        assert ml >= 4 and 1 <= off <= min(65535, self.n + nlit), (nlit, ml, off, self.n)
        self.plan.append(Seq(self.bytes(nlit), ml, off, run))
        self.n += nlit + ml

    def need(self, k, big=False):
        """Filler sequences until at least k output bytes exist."""
        while self.n < k:
            nlit = self.r(1, 400 if big else 20)
            ml = self.r(4, 2000 if big else 40)
            self.seq(nlit, ml, self.r(1, min(65535, self.n + nlit)))

    def filler(self, k):
        for _ in range(k):
            nlit = self.r(0 if self.n else 1, 20)
            self.seq(nlit, self.r(4, 40), self.r(1, min(65535, self.n + nlit)))

    def new_run(self):
        self.runs += 1
        return self.runs - 1

    def finish(self, conforming, ending="lits", tail=None):
        """conforming: a last literal run of at least max(5, 12 - last match length) bytes (`tail` if given, raised
        to that).  Otherwise `ending`: "match" (the stream ends right after a match), "empty" (a literal-only
        token without literals), "lits" (a literal-only token of `tail` bytes, a random count if None)."""
        last_ml = self.plan[-1].ml if self.plan else 0
        if self.plan and last_ml == 0:
            return self.plan
        if conforming:
            least = max(5, 12 - last_ml) if self.plan else 0
            k = max(least, tail if tail is not None else least + self.r(0, 8))
        elif ending == "match" and self.plan:
            return self.plan
        elif ending == "empty":
            k = 0
        else:
            k = tail if tail is not None else self.r(1, 20)
        self.plan.append(Seq(self.bytes(k), 0, 0, -1))
        return self.plan


def _case_lz4(b):
    return encode_lz4(b.plan), expected_lz4(b.plan), b.plan


ENDINGS = ("match", "empty", "lits")


def _spread(items, count, seed, prefix=64, size=0, conforming=True):
    """Items (functions of a builder) dealt round robin to `count` streams, each started with a sequence of
    `prefix` literal bytes, topped up with filler to at least `size` output bytes, then finished (the
    reference-accepted ones in each of the three endings in turn)."""
    builders = [_LZ4(seed * 1000 + k) for k in range(count)]
    for b in builders:
        if prefix:
            b.seq(prefix, 4, 1)
    for k, item in enumerate(items):
        item(builders[k % count])
    for k, b in enumerate(builders):
        b.need(size)
        b.finish(conforming, ENDINGS[k % 3])
    return [_case_lz4(b) for b in builders]


# ---- families -------------------------------------------------------------------------------- LZ4

def _short_run(b, style):
    """One run of short sequences (both lengths inside the token) of at most 64 output bytes whose match sources
    lie inside the run: style 0 with literals, sources anywhere in the run in front of the match; 1 without
    literals, often the previous match's bytes (matches of matches); 2 without literals, periods 1..3 (self-
    overlap, chains of random depth); 3 every offset exactly all the output in front of the match (the
    several-sequences step's bad_mine boundary); 4 one literal, then offset 1 over the other 63 bytes (a chain of
    depth 63: the last byte is 63 hops from the literal)."""
    run = b.new_run()
    if style == 4:
        for nlit, ml in ((1, 18), (0, 18), (0, 18), (0, 9)):
            b.seq(nlit, ml, 1, run)
        return
    start = b.n
    left = 64
    while left >= 4:
        nlit = 0 if style in (1, 2) else b.r(0, min(14, left - 4))
        if style == 0 and b.n + nlit == start:
            nlit = 1
        ml = b.r(4, min(18, left - nlit))
        front = b.n + nlit - start          # bytes of the run in front of the match
        if style == 3:
            off = min(b.n + nlit, 65535)
        elif style == 2 or front == 0:
            off = min(b.r(1, 3) if front == 0 else b.r(1, min(3, front)), b.n + nlit)
        else:
            off = b.r(1, front) if b.r(0, 1) else min(front, b.r(4, 8))
        b.seq(nlit, ml, off, run)
        left -= nlit + ml


def short_steps(seed=1, count=64, size=2048, conforming=True):
    items = [lambda b, s=s: _short_run(b, s) for _ in range(40) for s in (0, 1, 2, 0, 3, 4)]
    return _spread(items, count, seed, size=size, conforming=conforming)


def _overlap_items(off):
    def fp2(b):
        # fast path (2): one extension byte (ml >= 19), lit + ml <= 64, ml > off -- and lit + ml == 64 exactly.
        # (Offset 64 cannot overlap inside 64 bytes: there ml == 64 == off, the path's one-extension-byte form.)
        b.need(off)
        top = min(14, 63 - off) if off < 64 else 0
        nlit = b.r(0, top)
        b.seq(nlit, 64 - nlit, off)
        nlit = b.r(0, top)
        b.seq(nlit, b.r(max(19, min(off + 1, 64)), 64 - nlit), off)
        if off < 18:                        # (the match length inside the token, overlapping)
            b.seq(b.r(0, 14), b.r(max(4, off + 1), 18), off)

    def general(b):                         # the general path: ml 65..300
        b.need(off)
        b.seq(b.r(0, 14), b.r(65, 300), off)

    def in_literals(b):                     # offset <= lit: the source sits in the sequence's own literals
        nlit = b.r(max(off, 15), 80)
        b.seq(nlit, b.r(off + 1, off + 70), off)                  # offset < ml
        if off >= 4:
            b.seq(nlit, b.r(4, off), off)                          # offset >= ml
    return [fp2, general, in_literals]


def overlap(seed=2, count=16, size=0, conforming=True):
    items = [it for off in range(1, 65) for it in _overlap_items(off)]
    return _spread(items, count, seed, prefix=0, size=size, conforming=conforming)


LIT_LENGTHS = tuple(range(0, 65)) + tuple(15 + 255 * k + r for k in range(4) for r in (0, 1, 254))
ALL_FF_LENGTHS = (15 + 255 * 64, 15 + 255 * 64 + 7, 15 + 255 * 130 + 254)   # read_lsic's all-0xFF step


def _lengths_items():
    items = []
    for nl in LIT_LENGTHS + ALL_FF_LENGTHS:
        items.append(lambda b, nl=nl: b.seq(nl, b.r(4, 30), b.r(1, min(65535, b.n + nl))))

    def ext(b, e):                          # one extension byte e: ml = 19 + e, apart (odd e) or overlapping
        ml = 19 + e
        b.need(ml)
        b.seq(b.r(0, 3), ml, b.r(ml, min(65535, b.n)) if e % 2 else b.r(1, min(ml - 1, b.n)))

    def apart(b, ml):
        b.need(ml)
        b.seq(b.r(0, 14), ml, b.r(ml, min(65535, b.n)))
    items += [lambda b, e=e: ext(b, e) for e in range(255)]
    # 255 then 0, 255 255 0, 255 then 1, 254; long matches that do not overlap
    items += [lambda b, ml=ml: apart(b, ml) for ml in (19 + 255, 19 + 510, 19 + 256, 19 + 254, 65, 66, 100, 127,
                                                       128, 129, 500, 1000, 4096)]
    return items


def lengths(seed=3, count=12, size=0, conforming=True):
    return _spread(_lengths_items(), count, seed, size=size, conforming=conforming)


FAR_OFFSETS = (65535, 65534, 32768, 4096, 64, 65)
FAR_SIZES = (65536, 200000, 1 << 20, 4 << 20)


def far(seed=4, count=None, size=0, conforming=True):
    """Offsets 65535, 65534, 32768, 4096, 64, 65 all through chunks of 64 KiB .. 4 MiB (conforming: one of each
    size; the reference-accepted kind: the two smaller ones, to keep the generated output small)."""
    count = (4 if conforming else 2) if count is None else count
    out = []
    for k in range(count):
        total = FAR_SIZES[k % len(FAR_SIZES)]
        b = _LZ4(seed * 1000 + k)
        b.need(65535, big=True)
        while b.n < total - 70000:
            for off in FAR_OFFSETS:
                b.seq(b.r(0, 14), (4, 18, 19, 64, 300)[b.r(0, 4)], off)
            b.seq(b.r(100, 3000), b.r(4, 3000), b.r(1, 65535))   # (moves on through the chunk)
        for off in FAR_OFFSETS:
            b.seq(b.r(0, 14), b.r(4, 18), off)
        b.finish(conforming, ENDINGS[k % 3])
        out.append(_case_lz4(b))
    return out


def _chain_prefix(b, plain_tokens):
    """The stream's first 24 tokens, in fewer than 200 stream bytes: literal-bearing short sequences, then
    `plain_tokens` short sequences without literals copying from inside their own step (8: the decoder takes its
    CHAIN loop for the whole chunk; 7: the plain one)."""
    for _ in range(24 - plain_tokens):
        nlit = b.r(1, 5)
        b.seq(nlit, b.r(4, 12), b.r(1, b.n + nlit))
    run = b.new_run()
    start = b.n
    for _ in range(plain_tokens):
        front = b.n - start
        b.seq(0, b.r(4, 8), b.r(1, front) if front else b.r(1, 3), run)


def chainy(stream: bytes) -> bool:
    """The decoder's choice of loop (lz4_decode.hiph): the stream is at least 256 bytes long and its first two
    dozen tokens (while below stream byte 200 and without a 15 nibble) end in eight without literals."""
    if len(stream) < 256:
        return False
    p = plain = 0
    for _ in range(24):
        if p >= 200:
            break
        t = stream[p]
        if (t >> 4) == 15 or (t & 15) == 15:
            break
        plain = plain + 1 if (t >> 4) == 0 else 0
        p += 3 + (t >> 4)
    return plain >= 8


def _literal_token_bytes(k):
    return 1 + k + (len(lsic(k - 15)) if k >= 15 else 0)


def _to_stream_length(b, target, conforming):
    """Finish with a last literal run that makes the stream exactly `target` bytes long."""
    have = len(encode_lz4(b.plan))
    least = max(5, 12 - b.plan[-1].ml) if conforming else 0
    for k in range(target - have, -1, -1):
        if k >= least and have + _literal_token_bytes(k) == target:
            b.plan.append(Seq(b.bytes(k), 0, 0, -1))
            return
    raise AssertionError(f"no literal tail gives {target} stream bytes from {have}")


def _end_at(b, back, lit_last, k, conforming):
    """A last match-bearing short sequence whose token lies `back` bytes before the end of the stream (a literal-
    only token of the right length behind it), or -- reference-accepted kind, every other k -- a stream that ends
    right after that match.  (Conforming: a tail too short for the end rules is raised to them.)"""
    ml = b.r(4, 18)
    b.seq(lit_last, ml, b.r(1, min(65535, b.n + lit_last)))
    if conforming or k % 2:
        # bytes from the last match's token to the end: 3 + lit_last, then the literal-only token
        want = back - (3 + lit_last)
        tail = next((t for t in range(max(want, 0), -1, -1) if _literal_token_bytes(t) == want), None)
        if tail is None or (conforming and tail < max(5, 12 - ml)):
            tail = max(5, 12 - ml) if conforming else 0
        b.finish(conforming, "lits", tail)
    else:
        b.finish(False, "match")


def _far_chain_run(b, n=40):
    """n short sequences without literals -- the form the CHAIN loop's step takes -- whose offsets are the far
    ones in turn, with offsets inside the step between them (needs 65535 bytes of output in front)."""
    for j in range(n):
        b.seq(0, b.r(4, 8), FAR_OFFSETS[(j // 2) % len(FAR_OFFSETS)] if j % 2 == 0 else b.r(1, 24))


CHAIN_BACKS = (17, 18, 82, 16, 19, 83)


def chain_then(seed=5, count=6, size=0, conforming=True):
    """The CHAIN (8) and the plain (7) prefix, each followed by every other family as its tail, dealt over `count`
    streams per prefix: more than 64 KiB of output, runs of far offsets in the chain step's own form and with
    literals, every short-run style, every overlap item (offsets 1..64), every lengths item (the all-0xFF LSIC
    steps included), and at the end the stream_ends positions (the last match-bearing token CHAIN_BACKS bytes
    before the end, behind short runs without literals).  And the prefixes alone, finished at stream lengths 255,
    256 and 257 (the CHAIN test's threshold is 256)."""
    tails = ([lambda b, s=s: _short_run(b, s) for s in range(5)] * 4
             + [it for off in range(1, 65) for it in _overlap_items(off)]
             + _lengths_items())
    out = []
    k = 0
    for plain_tokens in (8, 7):
        for group in range(count):
            b = _LZ4(seed * 1000 + k)
            _chain_prefix(b, plain_tokens)
            b.need(65535, big=True)
            _far_chain_run(b)
            for off in FAR_OFFSETS:
                b.seq(b.r(1, 14), b.r(4, 18), off)
            for it in tails[group::count]:
                it(b)
            _far_chain_run(b)
            for style in (1, 2, 1):
                _short_run(b, style)
            _end_at(b, CHAIN_BACKS[group % len(CHAIN_BACKS)], (0, 3, 14)[group % 3], k, conforming)
            out.append(_case_lz4(b))
            k += 1
        for target in (255, 256, 257):
            b = _LZ4(seed * 1000 + k)
            _chain_prefix(b, plain_tokens)
            _to_stream_length(b, target, conforming)
            out.append(_case_lz4(b))
            k += 1
    return out


def stream_ends(seed=6, count=0, size=0, conforming=True):
    """The last match-bearing token 14..90 and 100 bytes before the end (kFastSeqBytes = 18, kBatchReach = 82)
    behind runs of short sequences; single-token streams; and (reference-accepted) empty literal tails and streams
    that end right after a match, of one sequence or of many."""
    out = []
    k = 0
    for back in tuple(range(14, 91)) + (100,):
        for lit_last in (0, 3, 14):
            b = _LZ4(seed * 1000 + k)
            b.seq(b.r(20, 60), 4, 1)
            for _ in range(3):
                _short_run(b, k % 4)
            _end_at(b, back, lit_last, k, conforming)
            out.append(_case_lz4(b))
            k += 1
    for nl in (0, 1, 4, 5, 14, 15, 16, 17, 18, 63, 64, 65, 81, 82, 83, 300):   # one literal-only token
        b = _LZ4(seed * 1000 + k)
        b.plan.append(Seq(b.bytes(nl), 0, 0, -1))
        out.append(_case_lz4(b))
        k += 1
    if not conforming:
        for ending in ("match", "empty"):
            for ml in (4, 18, 19, 64, 65, 300):
                b = _LZ4(seed * 1000 + k)
                b.seq(b.r(1, 14), ml, 1)                      # one sequence only
                b.finish(False, ending)
                out.append(_case_lz4(b))
                b = _LZ4(seed * 1000 + k + 500)
                b.seq(30, 4, 3)
                b.filler(k % 7 + 1)
                b.seq(b.r(0, 14), ml, b.r(1, 30))
                b.finish(False, ending)
                out.append(_case_lz4(b))
                k += 1
    return out


# ---- liblz4: a third-party encoder's streams

def load_liblz4():
    """The system liblz4 (ctypes), or None."""
    try:
        L = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    L.LZ4_compressBound.argtypes = [ctypes.c_int]
    L.LZ4_compress_fast.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.LZ4_compress_HC.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    return L


LIBLZ4_MODES = (("fast", 1), ("fast", 8), ("fast", 65537), ("hc", 3), ("hc", 9), ("hc", 12))
LIBLZ4_SIZES = (1024, 8192, 65536, 262144, 1 << 20)
DATAGEN_KINDS = ("text", "harness", "runs", "sparse", "random")


def parse_lz4(stream: bytes):
    """A valid stream's plan (the census reads liblz4's streams through it)."""
    plan, c = [], 0

    def code(n):
        nonlocal c
        while True:
            n += stream[c]
            c += 1
            if stream[c - 1] != 255:
                return n
    while c < len(stream):
        tok = stream[c]
        c += 1
        nl = code(15) if tok >> 4 == 15 else tok >> 4
        lit = stream[c:c + nl]
        c += nl
        if c == len(stream):
            plan.append(Seq(lit, 0, 0, -1))
            break
        off = stream[c] | (stream[c + 1] << 8)
        c += 2
        ml = code(19) if tok & 15 == 15 else 4 + (tok & 15)
        plan.append(Seq(lit, ml, off, -1))
    return plan


def _datagen_kind(kind, seed, n):
    if kind == "text":
        return datagen.text_like(seed, n)
    if kind == "harness":
        return datagen.harness_like_int32(seed, n // 4).tobytes()
    if kind == "runs":
        return datagen.random_runs_int32(seed, n // 4).tobytes()
    if kind == "sparse":
        return datagen.sparse_repeats(seed, n, 90, 7)
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def liblz4(seed=7, count=0, size=0, conforming=True):
    """Every datagen kind under every liblz4 mode (LZ4_compress_fast at acceleration 1, 8, 65537, LZ4_compress_HC
    at levels 3, 9, 12); the sizes 1 KiB .. 1 MiB in turn, so that every mode and every kind meets each size but
    one.  Expected output: the source.  [] where liblz4 is absent (the tests say so)."""
    L = load_liblz4()
    if L is None:
        return []
    out = []
    for ki, kind in enumerate(DATAGEN_KINDS):
        for mi, (mode, level) in enumerate(LIBLZ4_MODES):
            n = LIBLZ4_SIZES[(ki + mi) % len(LIBLZ4_SIZES)]
            src = _datagen_kind(kind, seed * 100 + 10 * ki + mi, n)
            cap = L.LZ4_compressBound(len(src))
            buf = ctypes.create_string_buffer(cap)
            f = L.LZ4_compress_fast if mode == "fast" else L.LZ4_compress_HC
            m = f(src, buf, len(src), cap, level)
            assert m > 0, (kind, mode, level, n)
            s = buf.raw[:m]
            out.append((s, src, parse_lz4(s)))
    return out


LZ4_FAMILIES = {"short_steps": short_steps, "overlap": overlap, "lengths": lengths, "far": far,
                "chain_then": chain_then, "stream_ends": stream_ends, "liblz4": liblz4}


@functools.lru_cache(maxsize=None)
def lz4_family(name, conforming=True):
    """[(stream, expected, plan)] of one family at its default seed and counts -- the tests' inputs.  (liblz4's
    streams are conforming; they are listed under conforming=True only.)"""
    if name == "liblz4":
        return tuple(liblz4()) if conforming else ()
    return tuple(LZ4_FAMILIES[name](conforming=conforming))


# ============================================================================================== Snappy

# Elements: ("L", bytes, width) -- a literal, its length - 1 in the tag (width 0) or in `width` bytes behind tag
# 59 + width; ("C", kind, length, offset) -- a copy with a 1- (kind 1), 2- (2) or 4-byte (4) offset.


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def encode_snappy(plan) -> bytes:
    out = bytearray(varint(sum(len(e[1]) if e[0] == "L" else e[2] for e in plan)))
    for e in plan:
        if e[0] == "L":
            _, data, w = e
            n = len(data) - 1
            if w == 0:
                assert 0 <= n < 60
                out.append(n << 2)
            else:
                assert 0 <= n < 256 ** w
                out.append((59 + w) << 2)
                out += n.to_bytes(w, "little")
            out += data
        else:
            _, kind, ln, off = e
            if kind == 1:
                assert 4 <= ln <= 11 and 1 <= off < 2048
                out.append(1 | ((ln - 4) << 2) | ((off >> 8) << 5))
                out.append(off & 0xFF)
            elif kind == 2:
                assert 1 <= ln <= 64 and 1 <= off < 65536
                out.append(2 | ((ln - 1) << 2))
                out += off.to_bytes(2, "little")
            else:
                assert kind == 4 and 1 <= ln <= 64 and 1 <= off < (1 << 32)
                out.append(3 | ((ln - 1) << 2))
                out += off.to_bytes(4, "little")
    return bytes(out)


def expected_snappy(plan) -> bytes:
    """The plan's output, one byte at a time."""
    out = bytearray()
    for e in plan:
        if e[0] == "L":
            out += e[1]
        else:
            for _ in range(e[2]):
                out.append(out[-e[3]])
    return bytes(out)


class _Snappy:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.plan = []
        self.n = 0

    def r(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    def lit(self, k, w=0):
        self.plan.append(("L", bytes(self.rng.integers(0, 256, k, dtype=np.uint8)), w))
        self.n += k

    def copy(self, kind, ln, off):
        assert 1 <= off <= self.n, (kind, ln, off, self.n)
        self.plan.append(("C", kind, ln, off))
        self.n += ln

    def need(self, k):
        while self.n < k:
            self.lit(self.r(1, 60))
            self.copy(2, self.r(4, 64), self.r(1, min(self.n, 65535)))

    def fill_to(self, total):
        """Exactly `total` output bytes: literals of at most 60 and copy-2 elements, last a literal."""
        while total - self.n > 200:
            self.lit(self.r(1, 60))
            self.copy(2, self.r(1, 64), self.r(1, min(self.n, 65535)))
        while self.n < total:
            self.lit(min(60, total - self.n))

    def case(self):
        return encode_snappy(self.plan), expected_snappy(self.plan), self.plan


# literal lengths of the 2-4-byte length fields (every length of the 1-byte field is taken)
WIDE_LIT_LENGTHS = {2: (1, 5, 60, 61, 256, 257, 4096, 65536), 3: (1, 5, 61, 256, 65536, 65537, 70000),
                    4: (1, 5, 61, 257, 65537, 70000)}


def literal_forms(seed=11, count=16, size=0):
    """Lengths 1..60 in the tag (each followed by a copy-2), every length 1..256 of tag 60, lengths 1..65537 and
    70000 in the fields of tags 61-63 (short ones written in a longer field), runs of 61..70 in tag 61."""
    items = [lambda b, k=k: (b.lit(k, 0), b.copy(2, b.r(1, 64), b.r(1, b.n))) for k in range(1, 61)]
    items += [lambda b, k=k: b.lit(k, 1) for k in range(1, 257)]
    items += [lambda b, k=k, w=w: b.lit(k, w) for w, ks in WIDE_LIT_LENGTHS.items() for k in ks]
    items += [lambda b, k=k: b.lit(k, 2) for k in range(61, 71)]
    builders = [_Snappy(seed * 1000 + k) for k in range(count)]
    for k, item in enumerate(items):
        item(builders[k % count])
    return [b.case() for b in builders]


def _in_step_run(b):
    """Elements of at most 64 output bytes whose copy sources lie inside the same 64 bytes (copies of copies,
    self-overlap with periods 1..7), literals of up to 20 bytes between them."""
    start = b.n
    b.lit(b.r(1, 8))
    left = 64 - (b.n - start)
    while left >= 4:
        front = b.n - start
        ln = b.r(4, min(11, left))
        off = b.r(1, min(front, 7)) if b.r(0, 1) else b.r(1, front)
        b.copy(1 if b.r(0, 1) else 2, ln, off)
        left -= ln
        if left > 8 and b.r(0, 2) == 0:
            k = b.r(1, min(20, left - 4))
            b.lit(k)
            left -= k


COPY_OFFSETS = (1, 2, 3, 5, 6, 7, 9, 12, 63, 64, 65, 255, 256, 2047, 2048, 32767, 32768, 32769, 40000, 65534,
                65535)


def copy_forms(seed=12, count=16, size=0):
    """copy-1 of every length 4..11 at every offset 1..2047; copy-2 and copy-4 of every length 1..64 at offsets
    COPY_OFFSETS and length - 1, length, length + 1 (offset < length: periods of every kind), copy-4 also at 70000,
    100000, 150000; runs of elements whose sources lie inside the same 64-byte step."""
    items = []
    for ln in range(4, 12):
        items += [lambda b, ln=ln, o0=o0: [b.copy(1, ln, o) for o in range(o0, 2048, 64)] for o0 in range(1, 65)]
    for kind in (2, 4):
        for ln in range(1, 65):
            offs = set(COPY_OFFSETS) | {max(ln - 1, 1), ln, ln + 1}
            if kind == 4:
                offs |= {70000, 100000, 150000}
            items.append(lambda b, kind=kind, ln=ln, offs=sorted(offs): [b.copy(kind, ln, o) for o in offs])
    items += [_in_step_run] * 200
    builders = [_Snappy(seed * 1000 + k) for k in range(count)]
    for b in builders:
        b.need(150001)
    for k, item in enumerate(items):
        item(builders[k % count])
    return [b.case() for b in builders]


PREAMBLE_SIZES = (0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, (1 << 21) + 1)   # varints of 1, 2, 3, 4 bytes


def preamble(seed=13, count=0, size=0):
    out = []
    for k, n in enumerate(PREAMBLE_SIZES):
        b = _Snappy(seed * 1000 + k)
        b.fill_to(n)
        out.append(b.case())
    return out


def snappy_stream_ends(seed=14, count=0, size=0):
    """The last element 2..5 bytes before the end (a 1- or 2-byte literal, a copy-1, copy-2 or copy-4: inside
    kSnappyWindowMin = 4 or just outside), behind 0..129 stream bytes of small elements (kSnappyBatchReach = 128);
    the output always fills usize exactly."""
    out = []
    k = 0
    for last in ("lit1", "lit2", "c1", "c2", "c4"):
        for run_bytes in range(130):
            b = _Snappy(seed * 1000 + k)
            b.need(b.r(64, 300))
            while run_bytes > 0:
                if b.r(0, 1):
                    ln = b.r(1, min(8, run_bytes))
                    b.lit(ln)
                    run_bytes -= ln + 1
                else:
                    b.copy(1, b.r(4, 11), b.r(1, min(2047, b.n)))
                    run_bytes -= 2
            if last == "lit1":
                b.lit(1)
            elif last == "lit2":
                b.lit(2)
            elif last == "c1":
                b.copy(1, b.r(4, 11), b.r(1, 5))
            elif last == "c2":
                b.copy(2, b.r(1, 64), b.r(1, min(70, b.n)))
            else:
                b.copy(4, b.r(1, 64), b.r(1, b.n))
            out.append(b.case())
            k += 1
    return out


SNAPPY_FAMILIES = {"literal_forms": literal_forms, "copy_forms": copy_forms, "preamble": preamble,
                   "stream_ends": snappy_stream_ends}


@functools.lru_cache(maxsize=None)
def snappy_family(name):
    return tuple(SNAPPY_FAMILIES[name]())


# ============================================================================================== census

def lz4_census(cases_by_family):
    """What the LZ4 plans hold, computed from the plans (and for the decoder's choice of loop, from the
    streams)."""
    c = {"streams": 0, "output_bytes": 0, "fp2_offsets": set(), "general_offsets": set(),
         "in_literals_lt_ml": set(), "in_literals_ge_ml": set(), "ext_bytes": set(), "lit_lengths": set(),
         "all_ff_steps": 0, "in_step_sources": 0, "deep_chains": 0, "max_depth": 0, "chain_prefixes": 0,
         "plain_prefixes": 0, "far_offsets": set(), "chain_form_offsets": set(), "last_token_backs": set()}
    for fam, cases in cases_by_family.items():
        fam = fam[0] if isinstance(fam, tuple) else fam   # (keys: a family's name, or (name, conforming))
        for stream, expected, plan in cases:
            c["streams"] += 1
            c["output_bytes"] += len(expected)
            for s in plan:
                nl = len(s.lit)
                if nl >= 15 and (nl - 15) // 255 >= 64:
                    c["all_ff_steps"] += 1
                if not s.ml:
                    continue
                c["lit_lengths"].add(nl)
                if 19 <= s.ml < 19 + 255:   # (one extension byte)
                    c["ext_bytes"].add(s.ml - 19)
                if nl == 0 and s.ml <= 18:  # (the CHAIN step's form)
                    c["chain_form_offsets"].add(s.off)
                if s.off > 64:
                    c["far_offsets"].add(s.off)
                if nl < 15 and 19 <= s.ml and nl + s.ml <= 64 and (s.ml > s.off or s.off == 64):
                    c["fp2_offsets"].add(s.off)
                if s.ml > s.off and 65 <= s.ml <= 300:
                    c["general_offsets"].add(s.off)
                if s.off <= nl and nl >= 15:
                    c["in_literals_lt_ml" if s.off < s.ml else "in_literals_ge_ml"].add(s.off)
            last = max((i for i, s in enumerate(plan) if s.ml), default=None)
            if last is not None and fam != "liblz4":
                c["last_token_backs"].add(len(stream) - len(encode_lz4(plan[:last])))
            if fam in ("short_steps", "chain_then"):
                _runs_census(plan, c)
            if fam == "chain_then" and len(stream) >= 256:
                c["chain_prefixes" if chainy(stream) else "plain_prefixes"] += 1
    return c


def _runs_census(plan, c):
    """In-step sources: matches of a run whose source lies inside the run; a chain's depth: the hops from an
    output byte through match bytes of the run to a literal of the run (depth 0, as is a byte whose source lies in
    front of the run) -- the rounds of "take the source's source" it needs."""
    pos, cur, start, depth = 0, None, 0, {}
    for s in plan:
        if s.run != cur:
            cur, start, depth = s.run, pos, {}
        for j in range(len(s.lit)):
            depth[pos + j] = 0
        pos += len(s.lit)
        if s.ml and s.run >= 0:
            src = pos - s.off
            if src >= start:
                c["in_step_sources"] += 1
            deepest = 0
            for j in range(s.ml):
                q = src + j
                d = depth[q] + 1 if q >= start else 0
                depth[pos + j] = d
                deepest = max(deepest, d)
            if deepest >= 6:
                c["deep_chains"] += 1
            c["max_depth"] = max(c["max_depth"], deepest)
        pos += s.ml


def snappy_census(cases_by_family):
    c = {"streams": 0, "output_bytes": 0, "lit_lengths": {w: set() for w in range(5)},
         "copy_lengths": {1: set(), 2: set(), 4: set()}, "copy1_pairs": set(), "far_copies": {2: 0, 4: 0},
         "copy4_offset_max": 0, "varint_widths": set(), "usizes": set()}
    for fam, cases in cases_by_family.items():
        for stream, expected, plan in cases:
            c["streams"] += 1
            c["output_bytes"] += len(expected)
            c["usizes"].add(len(expected))
            c["varint_widths"].add(len(varint(len(expected))))
            for e in plan:
                if e[0] == "L":
                    c["lit_lengths"][e[2]].add(len(e[1]))
                    continue
                _, kind, ln, off = e
                c["copy_lengths"][kind].add(ln)
                if kind == 1:
                    c["copy1_pairs"].add((ln, off))
                elif off > 32768:
                    c["far_copies"][kind] += 1
                if kind == 4:
                    c["copy4_offset_max"] = max(c["copy4_offset_max"], off)
    return c
