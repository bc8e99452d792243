"""Planned raw-Deflate streams (RFC 1951), written bit by bit.

In the spirit of tests/streamgen.py: every form of the format that a decoder has to get right, and every
form it has to refuse, is written on purpose here instead of hoped for from a compressor.  A plan is
`(name, stream bytes, expected output or None)`; tests/test_deflate_streamgen_cpu.py proves every plan with
zlib on the CPU (legal: `zlib.decompressobj(-15)` gives exactly the planned bytes; illegal: it raises or does
not reach `eof`), the GPU tests then decode the same streams.  Standard library only.

Tokens of a block: an int 0..255 is a literal; `("m", length, distance)` is a match with the usual symbols,
`("m", length, distance, length_symbol)` forces the length symbol (258 can be written as 285 or as 284 + 31);
`("l", symbol)` / `("d", symbol, extra_value)` write a raw literal/length or distance symbol (illegal ones
included).  The end-of-block symbol is added by the block writers.
"""
from __future__ import annotations

import zlib

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
               227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value: int, count: int):
        """`count` bits of `value`, lowest first (header fields, extra bits)."""
        assert 0 <= value < (1 << count) or count == 0
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, length: int):
        """A Huffman code: its first (most significant) bit first."""
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    @property
    def bit_offset(self) -> int:
        return self.n

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data: bytes):
        assert self.n == 0
        self.out += data

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def canonical_codes(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (3.2.2); the set may be incomplete or
    over-subscribed (codes are then still handed out in order, modulo 2^length)."""
    count = [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def flat_lengths(used, n):
    """A complete code over the symbols `used` of an alphabet of n: lengths k or k + 1."""
    used = sorted(set(used))
    lens = [0] * n
    m = len(used)
    if m == 0:
        return lens
    if m == 1:
        lens[used[0]] = 1
        return lens
    k = m.bit_length() - 1
    short = (1 << (k + 1)) - m
    for i, s in enumerate(used):
        lens[s] = k if i < short else k + 1
    return lens


def length_symbol(length):
    if length == 258:
        return 285
    for i in range(27, -1, -1):
        if LENGTH_BASE[i] <= length:
            return 257 + i
    raise ValueError(length)


def dist_symbol(dist):
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= dist:
            return i
    raise ValueError(dist)


def token_symbols(tokens):
    """-> [(litlen symbol, extra value, extra bits, None | (dist symbol, extra value, extra bits))]"""
    out = []
    for t in tokens:
        if isinstance(t, int):
            out.append((t, 0, 0, None))
        elif t[0] == "l":
            out.append((t[1], 0, 0, None))
        elif t[0] == "d":   # a raw distance symbol behind length 3
            out.append((257, 0, 0, (t[1], t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0)))
        else:
            length, dist = t[1], t[2]
            ls = t[3] if len(t) > 3 else length_symbol(length)
            ds = dist_symbol(dist)
            out.append((ls, length - LENGTH_BASE[ls - 257], LENGTH_EXTRA[ls - 257],
                        (ds, dist - DIST_BASE[ds], DIST_EXTRA[ds])))
    return out


def expand(tokens, history=b""):
    """What the tokens decode to behind `history` (legal tokens only)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out[len(history):])


def write_symbols(w, tokens, lit_codes, dist_codes, lenient=False):
    """`lenient`: a symbol without a code is left out (the rejected sets, where the header decides)."""
    for ls, lx, lxb, d in token_symbols(tokens) + [(256, 0, 0, None)]:
        if lenient and (ls not in lit_codes or (d is not None and d[0] not in dist_codes)):
            continue
        w.code(*lit_codes[ls])
        w.bits(lx, lxb)
        if d is not None:
            w.code(*dist_codes[d[0]])
            w.bits(d[1], d[2])


def stored_block(w, data: bytes, final: bool, nlen=None):
    w.bits(int(final), 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.raw(data)


def fixed_block(w, tokens, final: bool):
    w.bits(int(final), 1)
    w.bits(1, 2)
    write_symbols(w, tokens, canonical_codes(FIXED_LITLEN), canonical_codes(FIXED_DIST))


def _cl_symbols(lengths, rle=True):
    """The lengths as symbols of the code-length alphabet: [(symbol, extra value)]; with `rle`, runs become
    16 / 17 / 18 (greedy), also across the border between the two sets."""
    out, i = [], 0
    n = len(lengths)
    while i < n:
        v, run = lengths[i], 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        i += run
        if not rle:
            out += [(v, 0)] * run
            continue
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
    return out


code_length_symbols = _cl_symbols

CL_EXTRA_BITS = {16: 2, 17: 3, 18: 7}


def dynamic_header(w, final, hlit, hdist, cl_syms, cl_lengths=None, hclen=None):
    """BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code and the code-length symbols `cl_syms`.
    hlit / hdist are the COUNTS (257.. / 1..) and are written as they are (also illegal ones, as far as the
    5-bit fields go); cl_lengths: the 19 lengths of the code-length code (default: a complete code over the
    symbols in use); hclen: how many of them are stored (default: as few as possible, at least 4)."""
    if cl_lengths is None:
        used = {s for s, _ in cl_syms}
        if len(used) == 1:   # the code-length code has to be complete: a second one-bit code nobody uses
            used.add(next(s for s in (0, 8, 7, 9) if s not in used))
        cl_lengths = flat_lengths(used, 19)
    if hclen is None:
        hclen = max([4] + [k + 1 for k in range(19) if cl_lengths[CL_ORDER[k]]])
    w.bits(int(final), 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lengths[CL_ORDER[k]], 3)
    codes = canonical_codes(cl_lengths)
    for s, x in cl_syms:
        if s not in codes:   # (a code-length code under test that lacks the symbol: it is refused before this)
            continue
        w.code(*codes[s])
        if s >= 16:
            w.bits(x, CL_EXTRA_BITS[s])


def dynamic_block(w, tokens, final: bool, lit_lengths=None, dist_lengths=None, rle=True, cl_lengths=None, hclen=None,
                  hlit=None, hdist=None, lenient=False):
    """A dynamic block.  lit_lengths / dist_lengths default to complete codes over the symbols the tokens use
    (the distance set is one zero length when there is no match); hlit / hdist default to the lists' sizes."""
    syms = token_symbols(tokens)
    if lit_lengths is None:
        lit_lengths = flat_lengths({s[0] for s in syms} | {256}, max(257, max(s[0] for s in syms + [(256,)]) + 1))
    if dist_lengths is None:
        used = {s[3][0] for s in syms if s[3] is not None}
        dist_lengths = flat_lengths(used, max(used) + 1) if used else [0]
        if len(used) == 1:
            dist_lengths = flat_lengths(used | {(max(used) + 1) % 30}, max(max(used) + 1, (max(used) + 1) % 30 + 1))
    hlit = len(lit_lengths) if hlit is None else hlit
    hdist = len(dist_lengths) if hdist is None else hdist
    dynamic_header(w, final, hlit, hdist, _cl_symbols(list(lit_lengths) + list(dist_lengths), rle), cl_lengths, hclen)
    write_symbols(w, tokens, canonical_codes(lit_lengths), canonical_codes(dist_lengths), lenient)


def one_dynamic_block(lit_lengths, dist_lengths, tokens=(), rle=True, **kw) -> bytes:
    """A one-block stream that carries these two sets of code lengths and `tokens` (the wrapper of
    tests/test_deflate_tables_cpu.py)."""
    w = BitWriter()
    dynamic_block(w, list(tokens), True, lit_lengths, dist_lengths, rle, **kw)
    return w.done()


def zlib_verdict(stream: bytes):
    """(accepted, output): zlib's inflate on a raw stream, all of it given at once."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return False, b""
    return (True, out) if d.eof else (False, b"")


# ---------------------------------------------------------------------------------------------------- plans
def _text(n, seed=1):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"lorem", b"ipsum", b"0123456789", b"the", b"of", b" ", b"\n"]
    out, x = bytearray(), seed * 2654435761 % (1 << 32)
    while len(out) < n:
        x = (x * 1103515245 + 12345) % (1 << 31)
        out += words[(x >> 8) % len(words)] + b" "
    return bytes(out[:n])


def legal_plans():
    """[(name, stream, expected output)]"""
    plans = []

    def add(name, w, expect):
        plans.append((name, w.done() if isinstance(w, BitWriter) else w, bytes(expect)))

    # stored blocks of 0, 1 and 65 535 bytes that start at every bit offset: k bits of fixed-block prelude in
    # front (an empty fixed block is 10 bits; k = 0: none, else literals of a dynamic block tune the offset)
    for size in (0, 1, 65535):
        data = bytes((i * 7 + size) & 0xFF for i in range(size))
        for off in range(8):
            w = BitWriter()
            lead = b""
            if off:
                # stored blocks end on a byte boundary; an empty fixed block adds 10 bits (offset 2), one with
                # an 8-bit literal 18 (offset 2 again): offsets are tuned with 7-, 8- and 9-bit symbols
                toks = []
                while (w.bit_offset + 10 + sum(8 if t < 144 else 9 for t in toks)) % 8 != off:
                    toks.append(200 if len(toks) % 2 == 0 else 65)
                    if len(toks) > 16:
                        raise AssertionError("offset not reachable")
                fixed_block(w, toks, False)
                lead = bytes(toks)
            assert w.bit_offset == off
            stored_block(w, data, True)
            add(f"stored{size}_at_bit{off}", w, lead + data)
    w = BitWriter()
    fixed_block(w, [], True)
    add("empty_fixed", w, b"")

    # every length symbol with its extra-bit extremes, 258 both ways; in a fixed and in a dynamic block
    hist = _text(300)
    ltoks = list(hist)
    for i in range(29):
        for x in sorted({0, (1 << LENGTH_EXTRA[i]) - 1}):
            ltoks.append(("m", LENGTH_BASE[i] + x, 7 + i, 257 + i))
    ltoks.append(("m", 258, 1, 285))
    ltoks.append(("m", 258, 2, 284))
    for name, blk in (("fixed", fixed_block), ("dynamic", dynamic_block)):
        w = BitWriter()
        blk(w, ltoks, True)
        add(f"all_length_symbols_{name}", w, expand(ltoks))

    # every distance symbol with its extremes, and the distances 1, 2, 3, 4, 63, 64, 65, 32 768
    hist = _text(32768, seed=3)
    dtoks = list(hist)
    dists = sorted({DIST_BASE[s] + x for s in range(30) for x in (0, (1 << DIST_EXTRA[s]) - 1)}
                   | {1, 2, 3, 4, 63, 64, 65, 32768})
    for k, d in enumerate(dists):
        dtoks.append(("m", (3, 4, 64, 65, 130, 258)[k % 6], d))
        dtoks.append(33 + k % 90)
    for name, blk in (("fixed", fixed_block), ("dynamic", dynamic_block)):
        w = BitWriter()
        blk(w, dtoks, True)
        add(f"all_distance_symbols_{name}", w, expand(dtoks))

    # overlapping matches of every short distance against every length class
    otoks = list(b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ!?#" * 2)
    for d in (1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 257):
        for ln in (3, 63, 64, 65, 129, 257, 258):
            otoks += [("m", ln, d), 48 + d % 10]
    w = BitWriter()
    dynamic_block(w, otoks, True)
    add("overlapping_matches", w, expand(otoks))

    # a match that reaches back into an earlier block, also across a stored block
    a, s, b = list(_text(500, 5)), _text(700, 6), [("m", 200, 1100), 1, ("m", 258, 1401), ("m", 30, 3)]
    w = BitWriter()
    fixed_block(w, a, False)
    stored_block(w, s, False)
    dynamic_block(w, b, True)
    add("match_across_blocks", w, bytes(a) + s + expand(b, bytes(a) + s))

    # a run of equal lengths that crosses from the literal/length set into the distance set (16, 17, 18)
    # the literal/length set ends in zeros and the distance set starts with zeros
    # (17 / 18 across the border), and it ends in ones where the distance set is two ones (16 across)
    lit = [8] * 254 + [0, 0] + [9] * 4 + [0] * 20   # 254/256 + 4/512 = 1; zeros from symbol 260 to 279
    dist = [0] * 6 + [1, 1]                         # and the zeros go on; codes 6 and 7: distances 9.. and 13..
    toks = list(range(254)) + [("m", 3, 9), ("m", 4, 16)]
    w = BitWriter()
    dynamic_block(w, toks, True, lit, dist)
    syms = _cl_symbols(lit + dist, True)
    assert any(s in (17, 18) for s, _ in syms)
    add("zero_run_across_the_two_sets", w, expand(toks))
    lit = [2, 2, 2] + [0] * 253 + [3, 3]         # 3/4 + 2/8 = 1, ends 3 3
    dist = [3] * 8                               # eight 3-bit codes: complete; 3 3 | 3 3 3 ... one run for 16
    toks = [0, 1, 2, ("m", 3, 1), ("m", 3, 4), 1]
    w = BitWriter()
    dynamic_block(w, toks, True, lit, dist)
    assert (16, 3) in _cl_symbols(lit + dist, True) or any(s == 16 for s, _ in _cl_symbols(lit + dist, True))
    add("repeat_across_the_two_sets", w, expand(toks))

    # HCLEN: 19 lengths stored, and the fewest that can be legal.  HCLEN = 4 stores lengths for 16, 17, 18 and 0
    # only: every code length is then 0, symbol 256 has no code, and the block is refused (see illegal_plans);
    # 5 adds the 8: 256 eight-bit codes -- symbols 1..256 -- and no distance code.
    lit = [0] + [8] * 256
    toks = list(range(1, 256))
    w = BitWriter()
    dynamic_block(w, toks, True, lit, [0], rle=True)
    add("hclen_5", w, bytes(toks))
    w = BitWriter()
    dynamic_block(w, toks, True, lit, [0], rle=True, cl_lengths=flat_lengths({0, 8, 16, 18, 15}, 19), hclen=19)
    add("hclen_19", w, bytes(toks))

    # no distance code in use (one zero length), and a single distance code of one bit
    w = BitWriter()
    dynamic_block(w, list(b"no match here"), True, None, [0])
    add("dynamic_without_distance_code", w, b"no match here")
    toks = list(b"xyz") + [("m", 10, 1), ("m", 3, 1)]
    w = BitWriter()
    dynamic_block(w, toks, True, None, [1])
    add("single_distance_code", w, expand(toks))
    # a literal/length set that is only the end-of-block code, one bit (zlib accepts it: an empty block)
    w = BitWriter()
    dynamic_block(w, [], True, [0] * 256 + [1], [0])
    add("only_end_of_block_code", w, b"")

    # the largest alphabets with 15-bit codes: 286 + 30 symbols
    lit = max_alphabet_litlen()
    dist = max_alphabet_dist()
    toks = list(range(256)) * 2 + [("m", LENGTH_BASE[i], DIST_BASE[i % 30] if DIST_BASE[i % 30] <= 512 else 1 + i, 257 + i)
                                   for i in range(29)]
    toks += [("m", 3, DIST_BASE[s]) for s in range(30) if DIST_BASE[s] <= 600]
    w = BitWriter()
    dynamic_block(w, toks, True, lit, dist)
    add("max_alphabets_15_bit_codes", w, expand(toks))

    # a final block that ends on the last bit of the last byte, and one with bytes behind it
    # (3 header bits, 7 for the end of block: six 9-bit literals make 64)
    w = BitWriter()
    fixed_block(w, [200] * 6, True)
    assert w.bit_offset == 0
    add("ends_on_the_last_bit", w, bytes([200] * 6))
    w = BitWriter()
    dynamic_block(w, list(b"trailing bytes follow") + [("m", 20, 5)], True)
    add("trailing_bytes", w.done() + b"\x07\xff\x00 these bytes are not the stream's",
        expand(list(b"trailing bytes follow") + [("m", 20, 5)]))

    # 200 blocks in one chunk, of all three kinds
    w, expect = BitWriter(), bytearray()
    for k in range(200):
        last = k == 199
        piece = _text(40 + k % 17, seed=k + 11)
        if k % 3 == 0:
            stored_block(w, piece, last)
            expect += piece
        else:
            toks = list(piece) + ([("m", 3 + k % 250, 1 + k % 40)] if k else [])
            (fixed_block if k % 3 == 1 else dynamic_block)(w, toks, last)
            expect += expand(toks, bytes(expect))
    add("blocks_200", w, expect)
    return plans


def max_alphabet_litlen():
    """286 lengths, complete, with 15-bit codes."""
    return _split_to(286, 15)


def max_alphabet_dist():
    return _split_to(30, 15)


def _split_to(n, maxbits):
    """A complete set of n lengths that uses `maxbits`: the chain 1, 2, ..., maxbits - 1, maxbits, maxbits
    has maxbits + 1 codes; further codes come from splitting the shortest code that can still be split."""
    lens = list(range(1, maxbits)) + [maxbits, maxbits]
    while len(lens) < n:
        lens.sort()
        k = next(i for i, v in enumerate(lens) if v < maxbits)
        v = lens.pop(k)
        lens += [v + 1, v + 1]
    assert len(lens) == n and sum(1 << (maxbits - v) for v in lens) == 1 << maxbits
    # spread: give the long codes to the low symbols too, deterministically
    return [lens[(i * 7) % n] for i in range(n)] if n % 7 else sorted(lens)


def rejected_sets():
    """[(name, stream)]: one-block dynamic streams for every rejected form of code lengths (section 2 of the
    decoder's contract).  Each carries a literal as its payload so that only the header decides."""
    out = []
    ok_lit = flat_lengths(set(range(64, 91)) | {256}, 257)
    ok_dist = [1, 1]
    pay = [65]

    def blk(name, **kw):
        w = BitWriter()
        lit = kw.pop("lit", ok_lit)
        dist = kw.pop("dist", ok_dist)
        dynamic_block(w, kw.pop("tokens", pay), True, lit, dist, lenient=True, **kw)
        w.bits(0, 16)
        out.append((name, w.done()))

    over = list(ok_lit)
    over[0] = 1
    blk("litlen_oversubscribed", lit=over)
    inc = list(ok_lit)
    inc[64] = 0
    blk("litlen_incomplete", lit=inc, tokens=[66])
    blk("dist_oversubscribed", dist=[1, 1, 1])
    blk("dist_incomplete_two_codes", dist=[2, 2])
    blk("dist_single_code_of_two_bits", dist=[2])
    no256 = flat_lengths(set(range(64, 92)), 257)
    blk("litlen_without_256", lit=no256, tokens=[65])
    blk("code_length_code_oversubscribed", cl_lengths=[1, 1, 0, 0, 0, 0, 0, 0, 1] + [0] * 10, rle=False)
    blk("code_length_code_incomplete", cl_lengths=[2, 2, 0, 0, 0, 0, 0, 0, 2] + [0] * 10, rle=False)
    blk("code_length_code_single", lit=[0] * 256 + [1], dist=[1], cl_lengths=[0, 1] + [0] * 17, rle=False, tokens=[])
    # HLIT > 286 / HDIST > 30: the fields are written as they are
    lit288 = flat_lengths(set(range(288)), 288)
    blk("hlit_287", lit=flat_lengths(set(range(287)), 287), tokens=[65])
    blk("hlit_288", lit=lit288, tokens=[65])
    blk("hdist_31", dist=flat_lengths(set(range(31)), 31))
    blk("hdist_32", dist=flat_lengths(set(range(32)), 32))
    # a repeat (16) with nothing before it; repeats that run past HLIT + HDIST
    cl = flat_lengths({16, 17, 18, 0, 1, 8}, 19)
    for name, syms in (
        ("repeat_16_first", [(16, 0)] + [(8, 0)] * 254 + [(0, 0)] * 2),
        ("repeat_16_past_the_end", [(8, 0)] * 256 + [(1, 0), (1, 0), (16, 3)]),
        ("repeat_17_past_the_end", [(8, 0)] * 256 + [(1, 0), (1, 0), (1, 0), (17, 0)][1:] + [(17, 1)]),
        ("repeat_18_past_the_end", [(8, 0)] * 250 + [(18, 127)]),
    ):
        w = BitWriter()
        dynamic_header(w, True, 257, 2, syms, cl)
        w.bits(0, 24)
        out.append((name, w.done()))
    # HCLEN = 4: only 16, 17, 18 and 0 have a code, every length is 0, 256 has none
    w = BitWriter()
    dynamic_header(w, True, 257, 1, [(18, 127), (18, 98)], [1 if s in (18, 0) else 0 for s in range(19)], hclen=4)
    w.bits(0, 24)
    out.append(("hclen_4_all_lengths_zero", w.done()))
    return out


def illegal_plans():
    """[(name, stream)]"""
    out = []

    def add(name, w):
        out.append((name, w.done() if isinstance(w, BitWriter) else bytes(w)))

    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    add("btype_3", w)
    w = BitWriter()
    stored_block(w, b"stored data", True, nlen=len(b"stored data") ^ 0xFFFE)
    add("len_nlen_mismatch", w)
    for blk, name in ((fixed_block, "fixed"), (dynamic_block, "dynamic")):
        w = BitWriter()
        blk(w, list(b"abc") + [("m", 3, 4)], True)
        add(f"distance_before_start_{name}", w)
        w = BitWriter()
        blk(w, [("m", 3, 1)], True)
        add(f"distance_with_no_output_{name}", w)
    w = BitWriter()
    stored_block(w, b"0123456789", False)
    fixed_block(w, [("m", 5, 11)], True)
    add("distance_before_start_after_stored", w)
    for s in (286, 287):
        w = BitWriter()
        fixed_block(w, [65, ("l", s), 66], True)
        add(f"fixed_litlen_symbol_{s}", w)
    for s in (30, 31):
        w = BitWriter()
        fixed_block(w, list(b"abcdefgh") + [("d", s, 0), 66], True)
        add(f"fixed_distance_symbol_{s}", w)
    # a dynamic block whose one-bit literal/length or distance code is used with the pattern that is no code
    w = BitWriter()
    dynamic_header(w, True, 257, 1, _cl_symbols([0] * 256 + [1] + [0], True))
    w.bits(1, 1)    # the code of 256 is 0; 1 is nobody's
    w.bits(0, 16)
    add("unused_pattern_of_single_litlen_code", w)
    w = BitWriter()
    lit = flat_lengths({97, 256, 257}, 258)
    dynamic_header(w, True, 258, 1, _cl_symbols(lit + [1], True))
    codes = canonical_codes(lit)
    w.code(*codes[97])
    w.code(*codes[257])
    w.bits(1, 1)    # the distance alphabet's one code is 0
    w.code(*codes[256])
    add("unused_pattern_of_single_distance_code", w)
    w = BitWriter()
    dynamic_header(w, True, 258, 1, _cl_symbols(lit + [0], True))
    w.code(*codes[97])
    w.code(*codes[257])
    w.bits(0, 5)    # whatever follows a length here is no distance code
    w.code(*codes[256])
    add("match_without_distance_code", w)
    out += rejected_sets()
    # truncation of a legal stream at every byte boundary, and a missing final block
    w = BitWriter()
    fixed_block(w, list(_text(60, 9)) + [("m", 40, 13)], False)
    stored_block(w, b"stored part", False)
    dynamic_block(w, list(_text(50, 10)) + [("m", 100, 90)], True)
    whole = w.done()
    assert zlib_verdict(whole)[0]
    for k in range(len(whole)):
        out.append((f"truncated_at_{k}", whole[:k]))
    w = BitWriter()
    fixed_block(w, list(b"no final block"), False)
    stored_block(w, b"and then nothing", False)
    add("missing_final_block", w)
    return out
