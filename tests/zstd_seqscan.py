"""Reads the sequences of a one-block Zstandard frame back as (literal length, match length, Offset_Value), with
tests/zstd_framegen.py's tables: what the frames of the encoder's tests are asked about beyond their content (was
a repeat code used, which one).  tokens_of resolves the Offset_Values to offsets (the encoder's own token list);
tokens_and_bit_ranges also says where every sequence's fields lie in the sequences' bitstream.  Plain Python; the
table-description reader is the mirror of G.write_ncount."""
import zstd_framegen as G


def read_ncount(b: bytes, max_sym: int):
    """-> (norm, log, bytes used)"""
    acc = int.from_bytes(b, "little")
    log = (acc & 15) + 5
    pos, sym, norm = 4, 0, []
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    prev0 = False
    while remaining > 1 and sym <= max_sym:
        if prev0:
            while True:
                rep = acc >> pos & 3
                pos += 2
                norm += [0] * rep
                sym += rep
                if rep != 3:
                    break
        mx = (2 * threshold - 1) - remaining
        v = acc >> pos & ((1 << nb) - 1)
        if v & (threshold - 1) < mx:
            count = v & (threshold - 1)
            pos += nb - 1
        else:
            count = v & (2 * threshold - 1)
            if count >= threshold:
                count -= mx
            pos += nb
        count -= 1
        remaining -= abs(count)
        norm.append(count)
        sym += 1
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert remaining == 1 and sym <= max_sym + 1
    return norm, log, (pos + 7) // 8


class BackReader:
    def __init__(self, b: bytes):
        assert b and b[-1]
        self.b = bytes(b) + bytes(8)
        self.left = 8 * (len(b) - 1) + b[-1].bit_length() - 1

    def peek(self, n: int) -> int:   # the n <= 56 bits from `left` up
        at = self.left >> 3
        return int.from_bytes(self.b[at:at + 8], "little") >> (self.left & 7) & ((1 << n) - 1)

    def read(self, n: int) -> int:
        self.left -= n
        assert self.left >= 0
        return self.peek(n)


def compressed_block(frame: bytes):
    """-> the one block's (kind, payload) of a single-segment frame"""
    fhd = frame[4]
    assert fhd >> 5 & 1
    fcs = 1 if fhd >> 6 == 0 else 1 << (fhd >> 6)
    at = 5 + fcs
    h = int.from_bytes(frame[at:at + 3], "little")
    assert h & 1
    return h >> 1 & 3, frame[at + 3:at + 3 + (1 if (h >> 1 & 3) == 1 else h >> 3)]


def sequences_of(frame: bytes, ranges=None):
    """-> [(ll, ml, Offset_Value)] of the frame's compressed block, None where its block is not compressed.
    ranges: a list that receives (low, high, na, first) per sequence -- its fields are the bits [low, high) of the
    bitstream (bit 0: the lowest bit of its first byte), na the bits of its state updates and its LL extra bits,
    first their value: the bits [low, low + na)."""
    kind, b = compressed_block(frame)
    if kind != 2:
        return None
    t, sf = b[0] & 3, b[0] >> 2 & 3
    if t < 2:
        hb = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = b[0] >> 3 if hb == 1 else int.from_bytes(b[:hb], "little") >> 4
        lit_end = hb + (regen if t == 0 else 1)
    else:
        hb = 3 if sf < 2 else sf + 2
        lhc = int.from_bytes(b[:5], "little")
        lit_end = hb + {3: lhc >> 14 & 0x3FF, 4: lhc >> 18 & 0x3FFF, 5: lhc >> 22 & 0x3FFFF}[hb]
    s = b[lit_end:]
    n, p = s[0], 1
    if n == 0:
        return []
    if n >= 128:
        assert n < 255
        n, p = ((n - 128) << 8) + s[1], 2
    modes = s[p]
    p += 1
    tables = []
    for mode, (dnorm, dlog), max_sym in ((modes >> 6, G.LL_DEFAULT, 35), (modes >> 4 & 3, G.OF_DEFAULT, 31), (modes >> 2 & 3, G.ML_DEFAULT, 52)):
        if mode == G.PREDEFINED:
            tables.append((G.fse_table(dnorm, dlog), dlog))
        elif mode == G.RLE:
            tables.append(([(s[p], 0, 0)], 0))
            p += 1
        else:
            assert mode == G.FSE
            norm, log, used = read_ncount(s[p:], max_sym)
            assert sum(1 for c in norm if c) >= 2, "an FSE description of a single symbol"
            tables.append((G.fse_table(norm, log), log))
            p += used
    (tll, lll), (tof, lof), (tml, lml) = tables
    r = BackReader(s[p:])
    sll, sof, sml = r.read(lll), r.read(lof), r.read(lml)
    out = []
    for k in range(n):
        lc, oc, mc = tll[sll][0], tof[sof][0], tml[sml][0]
        high = r.left
        ov = (1 << oc) + r.read(oc)
        ml = G.ML_BASE[mc] + r.read(G.ML_BITS[mc])
        mid = r.left
        ll = G.LL_BASE[lc] + r.read(G.LL_BITS[lc])
        out.append((ll, ml, ov))
        if k + 1 < n:
            sll = tll[sll][2] + r.read(tll[sll][1])
            sml = tml[sml][2] + r.read(tml[sml][1])
            sof = tof[sof][2] + r.read(tof[sof][1])
        if ranges is not None:
            ranges.append((r.left, high, mid - r.left, r.peek(mid - r.left)))
    assert r.left == 0
    return out


def resolve(seqs):
    """[(ll, ml, Offset_Value)] -> [(ll, ml, offset)] as this encoder codes offsets: value 1 is the offset of the
    sequence before, a value above 3 is the offset plus 3; it never writes 2 or 3 (nor 1 without literals or first)"""
    out, prev = [], 0
    for ll, ml, ov in seqs:
        if ov == 1:
            if ll == 0 or prev == 0:
                raise ValueError("Offset_Value 1 without literals or in the first sequence")
            off = prev
        elif ov > 3:
            off = ov - 3
        else:
            raise ValueError(f"Offset_Value {ov}: this encoder never writes it")
        out.append((ll, ml, off))
        prev = off
    return out


def tokens_of(frame: bytes):
    """-> [(ll, ml, offset)] of the frame's compressed block, None for a raw or RLE block"""
    seqs = sequences_of(frame)
    return None if seqs is None else resolve(seqs)


def tokens_and_bit_ranges(frame: bytes):
    """-> ([(ll, ml, offset)], [(low, high, na, first)]) or None.  In the reader's order a sequence is OF extra, ML extra,
    LL extra, then the LL, ML and OF state updates: the reverse of what one lane of the kernel appends, so `low`
    modulo 32 is the lane's alignment in the kernel's stage and na the length of its first field."""
    ranges = []
    seqs = sequences_of(frame, ranges)
    return None if seqs is None else (resolve(seqs), ranges)
