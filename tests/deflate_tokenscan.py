"""A raw Deflate stream (RFC 1951) read back into its tokens, in plain Python.

zlib says what a stream expands to; this module says HOW it is written: per block the kind, BFINAL, HLIT / HDIST /
HCLEN, the code-length symbols as they stand in the header and the three tables of lengths, and over the whole
stream the token list [(literal run, match length, distance)] in the encoder kernel's grouping -- a run of literals
and the match behind it; the literals behind the last match are `tail` -- with every token's place in the stream in
bits.  tests/test_deflate_inputgen_cpu.py holds it to zlib's own streams and to deflate_streamgen's legal plans.

Nothing here comes from the encoder: the only import is the RFC's base and extra-bit tables, and nothing is read
from csrc/.  A stream that is not legal raises ScanError.
"""
from __future__ import annotations

from deflate_streamgen import CL_ORDER, DIST_BASE, DIST_EXTRA, LENGTH_BASE, LENGTH_EXTRA

STORED, FIXED, DYNAMIC = 0, 1, 2
CL_EXTRA = {16: (2, 3), 17: (3, 3), 18: (7, 11)}   # symbol: (extra bits, base of the count)


class ScanError(Exception):
    pass


class Block:
    """kind; final; at: the bit offset of its header; for a dynamic block hlit, hdist, hclen, cl_symbols
    [(symbol, value of its extra bits)] as written, cl_lens (19), and for every coded block lit_lens and dist_lens"""

    def __init__(self, kind, final, at):
        self.kind, self.final, self.at = kind, final, at
        self.hlit = self.hdist = self.hclen = None
        self.cl_symbols, self.cl_lens, self.lit_lens, self.dist_lens = [], None, None, None
        self.stored_bytes = 0


class Scan:
    """blocks; tokens [(literal run, match length, distance)]; ranges [(bit offset of the token's first symbol, bit
    offset of its match's length code, bit offset behind it)]; tail: the literals behind the last match; total_bits:
    up to and including the last block's end-of-block code (a stored block: its last byte); output: the expansion"""

    def __init__(self):
        self.blocks, self.tokens, self.ranges = [], [], []
        self.tail, self.total_bits, self.output = 0, 0, b""

    def match_bits(self):
        return [end - at for _, at, end in self.ranges]


def _table(lengths):
    """lengths -> (lookup by the next `width` stream bits, lowest first: symbol << 4 | length, or -1; width)"""
    width = max(lengths) if lengths else 0
    if width == 0:
        return [], 0
    count = [0] * (width + 1)
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code, left = [0] * (width + 2), 0, 1
    for b in range(1, width + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
        left = (left << 1) - count[b]
        if left < 0:
            raise ScanError("over-subscribed code")
    look = [-1] * (1 << width)
    for sym, ln in enumerate(lengths):
        if ln:
            c, rev = nxt[ln], 0
            nxt[ln] += 1
            for _ in range(ln):
                rev = (rev << 1) | (c & 1)
                c >>= 1
            entry = sym << 4 | ln
            for k in range(rev, 1 << width, 1 << ln):
                look[k] = entry
    return look, width


_FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST = [5] * 32


def scan(stream: bytes) -> Scan:
    s = Scan()
    nbits = 8 * len(stream)
    pos = 0                                         # in bits
    out = bytearray()
    run, run_at = 0, 0

    def need(n):
        if pos + n > nbits:
            raise ScanError("the stream ends inside a block")

    def peek(n):                                    # n <= 16: three bytes hold them at any alignment
        b = pos >> 3
        return (int.from_bytes(stream[b:b + 3], "little") >> (pos & 7)) & ((1 << n) - 1)

    def take(n):
        nonlocal pos
        need(n)
        v = peek(n)
        pos += n
        return v

    def symbol(look, width):
        nonlocal pos
        if width == 0:
            raise ScanError("a symbol of an empty code")
        e = look[peek(width)]
        if e < 0:
            raise ScanError("no such code")
        need(e & 15)
        pos += e & 15
        return e >> 4

    while True:
        at = pos
        final, kind = take(1), take(2)
        if kind == 3:
            raise ScanError("block type 3")
        blk = Block(kind, final, at)
        s.blocks.append(blk)
        if kind == STORED:
            pos = (pos + 7) & ~7
            n, nn = take(16), take(16)
            if n ^ nn != 0xFFFF:
                raise ScanError("LEN and NLEN disagree")
            need(8 * n)
            if run == 0:
                run_at = at
            out += stream[pos >> 3:(pos >> 3) + n]
            run += n
            pos += 8 * n
            blk.stored_bytes = n
        else:
            if kind == FIXED:
                blk.lit_lens, blk.dist_lens = list(_FIXED_LIT), list(_FIXED_DIST)
            else:
                blk.hlit, blk.hdist, blk.hclen = take(5) + 257, take(5) + 1, take(4) + 4
                if blk.hlit > 286 or blk.hdist > 30:
                    raise ScanError("HLIT or HDIST beyond the alphabets")
                blk.cl_lens = [0] * 19
                for k in range(blk.hclen):
                    blk.cl_lens[CL_ORDER[k]] = take(3)
                look, width = _table(blk.cl_lens)
                lens = []
                while len(lens) < blk.hlit + blk.hdist:
                    sym = symbol(look, width)
                    if sym < 16:
                        blk.cl_symbols.append((sym, 0))
                        lens.append(sym)
                        continue
                    xb, base = CL_EXTRA[sym]
                    x = take(xb)
                    blk.cl_symbols.append((sym, x))
                    if sym == 16 and not lens:
                        raise ScanError("a repeat with nothing before it")
                    lens += [lens[-1] if sym == 16 else 0] * (base + x)
                if len(lens) != blk.hlit + blk.hdist:
                    raise ScanError("a run beyond the last length")
                blk.lit_lens, blk.dist_lens = lens[:blk.hlit], lens[blk.hlit:]
                if blk.lit_lens[256] == 0:
                    raise ScanError("no end-of-block code")
            lit_look, lit_w = _table(blk.lit_lens)
            dist_look, dist_w = _table(blk.dist_lens)
            while True:
                sym_at = pos
                sym = symbol(lit_look, lit_w)
                if sym < 256:
                    if run == 0:
                        run_at = sym_at
                    out.append(sym)
                    run += 1
                elif sym == 256:
                    break
                else:
                    if sym > 285:
                        raise ScanError("length symbol 286 or 287")
                    length = LENGTH_BASE[sym - 257] + take(LENGTH_EXTRA[sym - 257])
                    ds = symbol(dist_look, dist_w)
                    if ds > 29:
                        raise ScanError("distance symbol 30 or 31")
                    dist = DIST_BASE[ds] + take(DIST_EXTRA[ds])
                    if dist > len(out):
                        raise ScanError("a distance beyond the output")
                    s.tokens.append((run, length, dist))
                    s.ranges.append((run_at if run else sym_at, sym_at, pos))
                    run = 0
                    if dist >= length:
                        out += out[len(out) - dist:len(out) - dist + length]
                    else:
                        for _ in range(length):
                            out.append(out[-dist])
        if final:
            break
    s.tail, s.total_bits, s.output = run, pos, bytes(out)
    s.unused = stream[(pos + 7) >> 3:]
    return s


def kinds(stream: bytes):
    return [b.kind for b in scan(stream).blocks]
