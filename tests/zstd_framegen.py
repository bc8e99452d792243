"""A planned-frame writer for Zstandard (RFC 8878), the sibling of tests/deflate_streamgen.py.

Frames are written from a plan, so the expected bytes are known by construction: a plan is a list of blocks, a
compressed block is its literals and a list of sequences (literal length, match length, Offset_Value), and
execute() is the format's own meaning of that list.  The writer has the backward-bitstream writer, an FSE
encoder over the decoding table of the format (predefined, RLE, described and repeated tables) and the frame,
block, literals and sequences headers in every size format.  inspect() lists the forms a frame contains from
its headers; what headers do not show (repeat codes, overlaps, the depth of a tree) the writer reports itself.
It also has a Huffman encoder (length-limited codes, direct and FSE-compressed weights, 1 and 4 streams, treeless).

libzstd (libzstd.so.1 through ctypes, no Python package) is the arbiter: arbiter(chunk, capacity) -> bytes or None.
Plain Python and numpy; importing it needs neither a GPU nor libzstd."""
from __future__ import annotations

import ctypes
import struct

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 * 1024

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = ([4, 3] + [2] * 11 + [1, 1, 1] + [2] * 9 + [3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
assert len(LL_BASE) == len(LL_DEFAULT[0]) == 36 and len(ML_BASE) == len(ML_DEFAULT[0]) == 53 and len(OF_DEFAULT[0]) == 29
PREDEFINED, RLE, FSE, REPEAT = 0, 1, 2, 3
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}


# ------------------------------------------------------------------------------------------------------ libzstd
_lib = None


def libzstd():
    """libzstd.so.1, or None where it does not load."""
    global _lib
    if _lib is None:
        try:
            z = ctypes.CDLL("libzstd.so.1")
        except OSError:
            _lib = False
            return None
        z.ZSTD_compress.restype = z.ZSTD_decompress.restype = z.ZSTD_compressBound.restype = ctypes.c_size_t
        z.ZSTD_isError.restype = ctypes.c_uint
        z.ZSTD_versionNumber.restype = ctypes.c_uint
        z.ZSTD_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
        z.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        _lib = z
    return _lib or None


def compress(data: bytes, level: int) -> bytes:
    z = libzstd()
    buf = ctypes.create_string_buffer(z.ZSTD_compressBound(len(data)))
    n = z.ZSTD_compress(buf, len(buf), data, len(data), level)
    assert not z.ZSTD_isError(n)
    return buf.raw[:n]


def arbiter(chunk: bytes, capacity: int):
    """ZSTD_decompress of the chunk into `capacity` bytes: the content, or None where libzstd refuses."""
    z = libzstd()
    buf = ctypes.create_string_buffer(max(capacity, 1))
    n = z.ZSTD_decompress(buf, capacity, chunk, len(chunk))
    return None if z.ZSTD_isError(n) else buf.raw[:n]


# ------------------------------------------------------------------------------------------------ bit writers
class BackWriter:
    """The backward bitstream: the decoder reads what was added LAST first; close() sets the final-bit marker."""

    def __init__(self):
        self.acc = 0
        self.n = 0

    def add(self, value: int, nbits: int):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0
        self.acc |= value << self.n
        self.n += nbits

    def close(self) -> bytes:
        self.add(1, 1)
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def write_in_read_order(fields) -> bytes:
    """fields: (value, nbits) in the order the decoder reads them."""
    w = BackWriter()
    for v, nb in reversed(fields):
        w.add(v, nb)
    return w.close()


# --------------------------------------------------------------------------------------------------------- FSE
def fse_table(norm, log):
    """The decoding table of a normalized distribution: [(symbol, nbits, base)] (RFC 8878 4.1.1)."""
    size = 1 << log
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [1 if c == -1 else c for c in norm]
    out = []
    for u in range(size):
        s = sym[u]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        out.append((s, nb, (x << nb) - size))
    return out


def fse_states(table, symbols):
    """States s_0..s_{n-1} with table[s_k].symbol == symbols[k] and s_{k+1} inside s_k's range (found backwards, as
    an encoder does); the last state is the symbol's state with the most bits."""
    by_sym = {}
    for u, (s, nb, base) in enumerate(table):
        by_sym.setdefault(s, []).append(u)
    states = [0] * len(symbols)
    states[-1] = max(by_sym[symbols[-1]], key=lambda u: table[u][1])
    for k in range(len(symbols) - 2, -1, -1):
        nxt = states[k + 1]
        states[k] = next(u for u in by_sym[symbols[k]] if table[u][2] <= nxt < table[u][2] + (1 << table[u][1]))
    return states


def normalize(symbols, log, nsym, low=()):
    """A distribution over [0, nsym) with sum 2^log in which every used symbol has a share; symbols of `low` get
    the "less than 1" probability (-1)."""
    hist = [0] * nsym
    for s in symbols:
        hist[s] += 1
    total, size = len(symbols), 1 << log
    norm = [0] * nsym
    for s, h in enumerate(hist):
        if h:
            norm[s] = -1 if s in low else max(1, h * size // total)
    used = sum(abs(c) for c in norm)
    big = max(range(nsym), key=lambda s: norm[s])
    norm[big] += size - used
    assert norm[big] >= 1 and sum(abs(c) for c in norm) == size
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


def write_ncount(norm, log) -> bytes:
    """The table description (4.1.1), the mirror of the decoder's reading."""
    acc, n = log - 5, 4
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    sym, prev0 = 0, False
    while remaining > 1:
        if prev0:
            run = 0
            while norm[sym + run] == 0:
                run += 1
            sym += run
            while run >= 3:
                acc |= 3 << n
                n += 2
                run -= 3
            acc |= run << n
            n += 2
        count = norm[sym]
        sym += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= abs(count)
        v = count + 1
        if v >= threshold:
            v += mx
        acc |= v << n
        n += nb - (1 if v < mx else 0)
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    return acc.to_bytes((n + 7) // 8, "little")


# --------------------------------------------------------------------------------------------------- sequences
def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


def execute(history: bytearray, frame_start: int, literals: bytes, sequences, rep):
    """The meaning of a block: appends to `history`, updates the repeat offsets `rep` (a list of 3) and returns the
    set of forms met (repeat codes, overlaps).  sequences: (ll, ml, Offset_Value)."""
    forms, lit, block_start = set(), 0, len(history)
    for ll, ml, ov in sequences:
        history += literals[lit:lit + ll]
        lit += ll
        if ov > 3:
            off = ov - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            forms.add(f"rep{ov}_ll{'0' if ll == 0 else 'n'}")
            idx = ov - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                assert off > 0
                rep[:] = [off, rep[0], rep[1]] if idx >= 2 else [off, rep[0], rep[2]]
        assert 0 < off <= len(history) - frame_start, "an offset before the frame's start"
        if off < ml:
            forms.add(f"overlap_{off}")
        if off > len(history) - block_start and block_start > frame_start:
            forms.add("match_across_blocks")
        for _ in range(ml):
            history.append(history[-off])
    history += literals[lit:]
    return forms


class SeqCoder:
    """Keeps the three tables of a frame from block to block (Repeat_Mode) and writes sequences sections."""

    def __init__(self):
        self.tables = {}
        self.forms = set()    # the accuracy logs of the tables it described

    def section(self, sequences, modes=(PREDEFINED, PREDEFINED, PREDEFINED), logs=(6, 5, 6), low=(), count_bytes=None):
        """modes / logs: (LL, OF, ML).  count_bytes forces the size of the sequence count."""
        n = len(sequences)
        if count_bytes is None:
            count_bytes = 1 if n < 128 else 2 if n < 0x7F00 else 3
        if n == 0:
            return b"\x00"
        if count_bytes == 1:
            assert n < 128
            out = bytes([n])
        elif count_bytes == 2:
            assert n < 0x7F00
            out = bytes([128 + (n >> 8), n & 255])
        else:
            assert n >= 0x7F00
            out = b"\xff" + struct.pack("<H", n - 0x7F00)
        codes = {"ll": [ll_code(s[0]) for s in sequences], "of": [s[2].bit_length() - 1 for s in sequences],
                 "ml": [ml_code(s[1]) for s in sequences]}
        out += bytes([modes[0] << 6 | modes[1] << 4 | modes[2] << 2])
        logsd = {}
        for name, mode, log, (dnorm, dlog), nsym in (("ll", modes[0], logs[0], LL_DEFAULT, 36), ("of", modes[1], logs[1], OF_DEFAULT, 32),
                                                      ("ml", modes[2], logs[2], ML_DEFAULT, 53)):
            if mode == PREDEFINED:
                self.tables[name] = (fse_table(dnorm, dlog), dlog)
            elif mode == RLE:
                assert len(set(codes[name])) == 1
                self.tables[name] = ([(codes[name][0], 0, 0)], 0)
                out += bytes([codes[name][0]])
            elif mode == FSE:
                norm = normalize(codes[name], log, nsym, low)
                self.tables[name] = (fse_table(norm, log), log)
                self.forms.add(f"{name}_log_{log}")
                out += write_ncount(norm, log)
            else:
                assert name in self.tables
            logsd[name] = self.tables[name][1]
        st = {k: fse_states(self.tables[k][0], codes[k]) for k in ("ll", "of", "ml")}
        fields = [(st["ll"][0], logsd["ll"]), (st["of"][0], logsd["of"]), (st["ml"][0], logsd["ml"])]
        for k, (ll, ml, ov) in enumerate(sequences):
            oc, mc, lc = codes["of"][k], codes["ml"][k], codes["ll"][k]
            fields += [(ov - (1 << oc), oc), (ml - ML_BASE[mc], ML_BITS[mc]), (ll - LL_BASE[lc], LL_BITS[lc])]
            if k + 1 < n:
                for name in ("ll", "ml", "of"):
                    s, nb, base = self.tables[name][0][st[name][k]]
                    fields.append((st[name][k + 1] - base, nb))
        return out + write_in_read_order(fields)


# ------------------------------------------------------------------------------------------------------ headers
def literals_raw(data: bytes, header_bytes=None) -> bytes:
    n = len(data)
    hb = header_bytes or (1 if n < 32 else 2 if n < 4096 else 3)
    if hb == 1:
        assert n < 32
        return bytes([n << 3]) + data
    if hb == 2:
        assert n < 4096
        return struct.pack("<H", n << 4 | 1 << 2) + data
    return struct.pack("<I", n << 4 | 3 << 2)[:3] + data


def literals_rle(byte: int, n: int, header_bytes=None) -> bytes:
    hb = header_bytes or (1 if n < 32 else 2 if n < 4096 else 3)
    if hb == 1:
        head = bytes([n << 3 | 1])
    elif hb == 2:
        head = struct.pack("<H", n << 4 | 1 << 2 | 1)
    else:
        head = struct.pack("<I", n << 4 | 3 << 2 | 1)[:3]
    return head + bytes([byte])


# ------------------------------------------------------------------------------------------------------ Huffman
def huf_lengths(data: bytes, max_bits=11):
    """Code lengths of a complete prefix code for the bytes of `data` (at least two distinct), at most max_bits long:
    Huffman's algorithm, then the longest codes shortened and the Kraft sum restored."""
    import heapq
    hist = {}
    for b in data:
        hist[b] = hist.get(b, 0) + 1
    assert len(hist) >= 2
    heap = [(n, s, (s,)) for s, n in sorted(hist.items())]
    heapq.heapify(heap)
    length = dict.fromkeys(hist, 0)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for sym in a[2] + b[2]:
            length[sym] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    unit = 1 << max_bits
    for sym in length:
        length[sym] = min(length[sym], max_bits)
    kraft = sum(unit >> l for l in length.values())
    by_rarity = sorted(length, key=lambda x: (hist[x], x))
    while kraft > unit:       # lengthen the rarest symbol that can still grow
        sym = next(x for x in by_rarity if length[x] < max_bits)
        kraft -= unit >> (length[sym] + 1)
        length[sym] += 1
    while kraft < unit:       # shorten the most frequent symbol whose gain still fits
        sym = next(x for x in reversed(by_rarity) if length[x] > 1 and (unit >> length[x]) <= unit - kraft)
        kraft += unit >> length[sym]
        length[sym] -= 1
    return length


def huf_weights(length):
    """-> (weights[0 .. last symbol], table log): weight = log + 1 - length, 0 for a symbol without a code"""
    log = max(length.values())
    return [log + 1 - length[s] if s in length else 0 for s in range(max(length) + 1)], log


def huf_codes(weights, log):
    """symbol -> (code, bits), the code read most significant bit first: the decoding table's order (by weight, then
    by symbol, the lightest first)"""
    codes, start = {}, 0
    for w in range(1, log + 1):
        for sym, sw in enumerate(weights):
            if sw == w:
                codes[sym] = (start >> (w - 1), log + 1 - w)
                start += 1 << (w - 1)
    assert start == 1 << log
    return codes


def huf_stream(data: bytes, codes, extra_low_bits=()) -> bytes:
    w = BackWriter()
    for v, nb in extra_low_bits:   # (bits below the last symbol: no legal stream has them)
        w.add(v, nb)
    for b in reversed(data):
        w.add(*codes[b])
    return w.close()


def weights_direct(weights) -> bytes:
    """the description with 4 bits a weight; the last weight is implied"""
    body = list(weights[:-1])
    assert 1 <= len(body) <= 128
    nib = body + [0] * (len(body) & 1)
    return bytes([127 + len(body)]) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))


def weights_fse(weights, log=6, short_by=0) -> bytes:
    """the FSE-compressed description: two interleaved states, symbol k decoded by state k % 2.  short_by: bits
    left out at the low end of the bitstream (no legal description lacks them)."""
    body = list(weights[:-1])
    assert len(body) >= 2
    norm = normalize(body, log, 13)
    table = fse_table(norm, log)
    chains = [fse_states(table, body[0::2]), fse_states(table, body[1::2])]
    assert table[chains[len(body) % 2][-1]][1] >= 1   # the state of the last symbol but one must ask for bits
    fields = [(chains[0][0], log), (chains[1][0], log)]
    for k in range(len(body) - 2):
        st, nxt = chains[k % 2][k // 2], chains[k % 2][k // 2 + 1]
        fields.append((nxt - table[st][2], table[st][1]))
    if short_by:
        total = sum(nb for _, nb in fields)
        acc = 0
        for v, nb in fields:
            acc = acc << nb | v
        fields = [(acc >> short_by, total - short_by)]
    out = write_ncount(norm, log) + write_in_read_order(fields)
    assert len(out) < 128
    return bytes([len(out)]) + out


def literals_huffman(data: bytes, streams=4, header_bytes=None, description=b"", codes=None, treeless=False, extra_low_bits=()) -> bytes:
    """A Huffman-coded literals section: `description` (weights_direct / weights_fse, empty for treeless literals) and
    1 or 4 streams coded with `codes`."""
    n = len(data)
    if streams == 1:
        body = huf_stream(data, codes, extra_low_bits)
    else:
        seg = (n + 3) // 4
        parts = [huf_stream(data[i * seg:(i + 1) * seg], codes, extra_low_bits if i == 3 else ()) for i in range(4)]
        body = b"".join(struct.pack("<H", len(q)) for q in parts[:3]) + b"".join(parts)
    comp = len(description) + len(body)
    hb = header_bytes or (3 if max(n, comp) < 1024 else 4 if max(n, comp) < 16384 else 5)
    assert not (streams == 1 and hb != 3)
    bits = {3: 10, 4: 14, 5: 18}[hb]
    assert n < 1 << bits and comp < 1 << bits
    sf = 0 if streams == 1 else hb - 2
    head = (3 if treeless else 2) | sf << 2 | n << 4 | comp << (4 + bits)
    return head.to_bytes(hb, "little") + description + body


def block(kind: int, payload: bytes, last: bool, size=None) -> bytes:
    """kind 0 raw, 1 RLE (payload: one byte, size: the run), 2 compressed."""
    size = len(payload) if size is None else size
    return struct.pack("<I", size << 3 | kind << 1 | int(last))[:3] + payload


def frame_header(content_size=None, fcs_bytes=None, single_segment=None, window_log=None, checksum=False, dict_id=None,
                 reserved=0) -> bytes:
    if fcs_bytes is None:
        fcs_bytes = 0 if content_size is None else 1 if content_size < 256 else 2 if content_size < 65536 + 256 else 4
    if single_segment is None:
        single_segment = fcs_bytes > 0 and window_log is None
    assert fcs_bytes in (0, 1, 2, 4, 8) and not (fcs_bytes == 1 and not single_segment)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    did = b"" if dict_id is None else struct.pack("<I", dict_id)
    fhd = flag << 6 | int(single_segment) << 5 | reserved << 3 | int(checksum) << 2 | (3 if dict_id is not None else 0)
    out = struct.pack("<IB", MAGIC, fhd)
    if not single_segment:
        out += bytes([((window_log or 17) - 10) << 3])
    out += did
    if fcs_bytes:
        out += (content_size - (256 if fcs_bytes == 2 else 0)).to_bytes(fcs_bytes, "little")
    return out


def skippable(payload: bytes, nibble=0) -> bytes:
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + payload


def xxh64(data: bytes, seed=0) -> int:
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    M = (1 << 64) - 1
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda a, v: rotl((a + v * P2) & M, 31) * P1 & M
    n, at = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while at + 32 <= n:
            for j in range(4):
                v[j] = rnd(v[j], int.from_bytes(data[at + 8 * j: at + 8 * j + 8], "little"))
            at += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for x in v:
            h = ((h ^ rnd(0, x)) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while at + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[at:at + 8], "little")), 27) * P1 + P4) & M
        at += 8
    if at + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[at:at + 4], "little") * P1 & M), 23) * P2 + P3) & M
        at += 4
    while at < n:
        h = rotl(h ^ (data[at] * P5 & M), 11) * P1 & M
        at += 1
    h ^= h >> 33
    h = h * P2 & M
    h ^= h >> 29
    h = h * P3 & M
    return h ^ (h >> 32)


def frame(blocks, declare=True, checksum=False, **header):
    """blocks: ("raw", bytes) | ("rle", byte, n) | ("seq", literals part (literals_raw / literals_rle bytes), literal
    bytes, sequences, SeqCoder.section keywords).  -> (frame, content, forms)"""
    content, forms, rep, coder, body = bytearray(), set(), [1, 4, 8], SeqCoder(), b""
    if not blocks:
        blocks = [("raw", b"")]
    for i, b in enumerate(blocks):
        last = i + 1 == len(blocks)
        if b[0] == "raw":
            content += b[1]
            body += block(0, b[1], last)
        elif b[0] == "rle":
            content += bytes([b[1]]) * b[2]
            body += block(1, bytes([b[1]]), last, b[2])
        else:
            _, lit_section, lits, seqs, kw = b[:5]
            forms |= execute(content, 0, lits, seqs, rep) | (set(b[5]) if len(b) > 5 else set())
            body += block(2, lit_section + coder.section(seqs, **kw), last)
    forms |= coder.forms
    head = frame_header(len(content) if declare else None, checksum=checksum, **header)
    tail = struct.pack("<I", xxh64(bytes(content)) & 0xFFFFFFFF) if checksum else b""
    return head + body + tail, bytes(content), forms


# ---------------------------------------------------------------------------------------------------- inspector
def inspect(chunk: bytes):
    """The forms a legal chunk contains, from its headers: a set of strings."""
    forms, at, frames = set(), 0, 0
    while at < len(chunk):
        magic = struct.unpack_from("<I", chunk, at)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            forms.add("skippable_" + ("before" if frames == 0 else "after_a_frame"))
            at += 8 + struct.unpack_from("<I", chunk, at + 4)[0]
            continue
        assert magic == MAGIC
        frames += 1
        if frames == 2:
            forms.add("two_frames")
        fhd = chunk[at + 4]
        single, flag = fhd >> 5 & 1, fhd >> 6
        fcs = (1 if single else 0) if flag == 0 else 1 << flag
        forms.add(f"fcs_{fcs}")
        forms.add("single_segment" if single else "window_descriptor")
        if fhd & 4:
            forms.add("checksum")
        at += 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + fcs
        nblocks = 0
        while True:
            h = int.from_bytes(chunk[at:at + 3], "little")
            last, kind, size = h & 1, h >> 1 & 3, h >> 3
            at += 3
            nblocks += 1
            forms.add(("raw_block", "rle_block", "compressed_block")[kind])
            if size == BLOCK_MAX and kind != 2:
                forms.add("block_of_128k")
            if kind == 2:
                b = chunk[at:at + size]
                t, sf = b[0] & 3, b[0] >> 2 & 3
                if t < 2:
                    hb = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                    regen = b[0] >> 3 if hb == 1 else int.from_bytes(b[:hb], "little") >> 4
                    forms.add(f"{('raw', 'rle')[t]}_literals_{hb}")
                    lit_end = hb + (regen if t == 0 else 1)
                else:
                    hb = 3 if sf < 2 else sf + 2
                    lhc = int.from_bytes(b[:5], "little")
                    comp = {3: lhc >> 14 & 0x3FF, 4: lhc >> 18 & 0x3FFF, 5: lhc >> 22 & 0x3FFFF}[hb]
                    streams = 1 if sf == 0 else 4
                    forms.add(f"{('huffman', 'treeless')[t - 2]}_literals_{streams}_stream_{hb}")
                    if t == 2:
                        forms.add("weights_direct" if b[hb] >= 128 else "weights_fse")
                        if b[hb] < 128:
                            forms.add(f"weights_log_{(b[hb + 1] & 15) + 5}")
                    lit_end = hb + comp
                s = b[lit_end:]
                n = s[0]
                cb = 1 if n < 128 else 2 if n < 255 else 3
                forms.add(f"seq_count_{0 if n == 0 else cb}")
                if n:
                    m = s[cb]
                    for name, mode in (("ll", m >> 6), ("of", m >> 4 & 3), ("ml", m >> 2 & 3)):
                        forms.add(f"{name}_{('predefined', 'rle', 'fse', 'repeat')[mode]}")
            at += 1 if kind == 1 else size
            if last:
                break
        if nblocks >= 3:
            forms.add("three_blocks")
        if fhd & 4:
            at += 4
    assert at == len(chunk)
    return forms


# --------------------------------------------------------------------------------------------------------- plans
def legal_plans():
    """-> [(name, chunk, content, forms met while executing)]"""
    out = []

    def add(name, fr):
        out.append((name, fr[0], fr[1], fr[2]))
    text = b"It was the best of times, it was the worst of times, it was the age of wisdom. " * 40
    add("empty_frame", frame([], single_segment=True, fcs_bytes=1))
    add("raw_rle_blocks", frame([("raw", text[:100]), ("rle", 0x41, 1000), ("raw", text[:7])]))
    add("block_of_128k", frame([("raw", (text * 42)[:BLOCK_MAX]), ("rle", 7, BLOCK_MAX)], fcs_bytes=4))
    add("no_content_size", frame([("raw", text[:300])], declare=False, window_log=10))
    add("fcs_8_bytes", frame([("raw", text[:300])], fcs_bytes=8))
    add("fcs_2_bytes", frame([("raw", text[:300])], fcs_bytes=2))
    add("window_and_size", frame([("rle", 9, 70000)], window_log=17, fcs_bytes=4))
    add("checksum", frame([("raw", text[:1000]), ("rle", 1, 33)], checksum=True))
    add("checksum_short", frame([("raw", text[:31])], checksum=True))
    add("checksum_empty", frame([], checksum=True, single_segment=True, fcs_bytes=1))
    add("dictionary_id_zero", frame([("raw", text[:50])], dict_id=0))
    a, b = frame([("raw", text[:500])]), frame([("rle", 0x5A, 77)], checksum=True)
    out.append(("two_frames", a[0] + b[0], a[1] + b[1], set()))
    out.append(("skippable_everywhere", skippable(b"skip me") + a[0] + skippable(b"", 5) + b[0] + skippable(b"x" * 40, 15),
                a[1] + b[1], set()))
    out.append(("only_skippable", skippable(b"nothing else"), b"", set()))
    out.append(("empty_chunk", b"", b"", set()))
    # literals without sequences: raw and RLE literals in their three header sizes
    for hb, n in ((1, 20), (2, 20), (2, 3000), (3, 20), (3, 70000)):
        add(f"raw_literals_{hb}_{n}", frame([("seq", literals_raw((text * 30)[:n], hb), (text * 30)[:n], [], {})]))
        add(f"rle_literals_{hb}_{n}", frame([("seq", literals_rle(0x61, n, hb), b"a" * n, [], {})]))
    # Huffman-coded literals: direct and FSE-compressed weights, 1 and 4 streams in every header size, treeless
    # literals that reuse the tree of the block before, the deepest tree
    words = (text * 30)
    def huf(data, streams, mode, hb=None, wlog=6):
        w, log = huf_weights(huf_lengths(data))
        desc = weights_direct(w) if mode == "direct" else weights_fse(w, wlog)
        return literals_huffman(data, streams, hb, desc, huf_codes(w, log)), huf_codes(w, log)
    for streams, mode, n, hb in ((1, "direct", 300, 3), (1, "fse", 900, 3), (4, "direct", 300, 3), (4, "fse", 1000, 3), (4, "fse", 1000, 4),
                                 (4, "fse", 9000, 4), (4, "fse", 1000, 5), (4, "fse", 70000, 5), (4, "fse", 6, 3), (4, "fse", 9, 3)):
        data = words[:n] if n > 20 else b"abcabcaab"[:n]
        section, _ = huf(data, streams, mode, hb, 6 if n > 20 else 5)
        add(f"huffman_{streams}_stream_{mode}_{n}_header_{hb}", frame([("seq", section, data, [(5, 4, 3 + 3)] if n > 20 else [], {})]))
    first, second, third = words[:2000], words[2000:2700], words[2700:3500]
    section, codes = huf(first, 4, "fse")
    assert set(second) | set(third) <= set(codes)
    add("treeless_1_and_4_streams", frame([("seq", section, first, [(100, 30, 3 + 50)], {}),
                                           ("seq", literals_huffman(second, 1, 3, b"", codes, treeless=True), second, [(7, 9, 3 + 1000)], {}),
                                           ("seq", literals_huffman(third, 4, None, b"", codes, treeless=True), third, [], {})]))
    deep = {sym: min(sym + 1, 11) for sym in range(12)}          # lengths 1, 2, .. 10, 11, 11
    data = bytes(sym for sym in range(12) for _ in range(1 + (2048 >> deep[sym]))) * 2
    w, log = huf_weights(deep)
    assert log == 11
    for mode, desc in (("direct", weights_direct(w)), ("fse", weights_fse(w, 6))):
        add(f"huffman_depth_11_{mode}", frame([("seq", literals_huffman(data, 4, None, desc, huf_codes(w, log)), data, [], {}, {"huffman_depth_11"})]))
    # every repeat-offset case, with and without literals in front, then self-overlapping matches
    lits = text[:400]
    reps = [(10, 5, 3 + 7), (4, 6, 3 + 15), (3, 4, 3 + 9)]
    for ov in (1, 2, 3):
        for ll in (0, 5):
            add(f"repeat_code_{ov}_ll_{ll}", frame([("seq", literals_raw(lits), lits, reps + [(ll, 8, ov), (2, 5, 1)], {})]))
    for off in (1, 2, 3, 63, 64, 65):
        add(f"overlap_{off}", frame([("seq", literals_raw(lits), lits, [(70, 200 + off, off + 3), (3, 131, off + 3)], {})]))
    # tables and offsets that persist over three blocks; a match that reaches back across a block boundary
    many = [(3, 4 + k % 9, 3 + 1 + k % 40) for k in range(100)]
    fse = dict(modes=(FSE, FSE, FSE), logs=(6, 6, 7))
    rep_all = dict(modes=(REPEAT, REPEAT, REPEAT))
    add("three_blocks_repeat_mode", frame([("raw", text[:200]), ("seq", literals_raw(lits), lits, many, fse),
                                           ("seq", literals_raw(lits[:310]), lits[:310], [(3, 12, 3 + 40)] + many, rep_all),
                                           ("seq", literals_rle(0x2E, 350), b"." * 350, many + [(3, 5, 3 + 2)], rep_all)], checksum=True))
    add("rle_modes", frame([("seq", literals_raw(lits), lits, [(2, 7, 3 + 2)] * 50, dict(modes=(RLE, RLE, RLE)))]))
    add("max_accuracy_logs", frame([("seq", literals_raw(lits * 3), lits * 3, [(k % 17, 3 + k % 40, 3 + 1 + (k % 3 if k > 3 else 0)) for k in range(1, 121)],
                                     dict(modes=(FSE, FSE, FSE), logs=(9, 8, 9)))]))
    add("less_than_one", frame([("seq", literals_raw(lits), lits, many + [(17, 40, 3 + 100)], dict(modes=(FSE, FSE, FSE), logs=(6, 6, 6), low=(16, 32)))]))
    add("two_byte_count", frame([("seq", literals_raw(lits), lits, [(1, 3, 4)] * 300, dict(modes=(RLE, RLE, RLE)))]))
    add("two_byte_count_small", frame([("seq", literals_raw(lits), lits, [(1, 3, 4)] * 100, dict(modes=(RLE, RLE, RLE), count_bytes=2))]))
    add("three_byte_count", frame([("seq", literals_raw(b"xy"), b"xy", [(2, 3, 4)] + [(0, 3, 3 + 1)] * 0x7F00, {})], fcs_bytes=4))
    add("long_lengths", frame([("seq", literals_raw((text * 30)[:70000], 3), (text * 30)[:70000], [(66000, 70000, 3 + 65000), (100, 131074, 3 + 1)], {})]))
    return out


LEGAL_FORMS_PLANNED = {
    "raw_block", "rle_block", "compressed_block", "raw_literals_1", "raw_literals_2", "raw_literals_3", "rle_literals_1",
    "rle_literals_2", "rle_literals_3", "ll_predefined", "of_predefined", "ml_predefined", "ll_fse", "of_fse", "ml_fse",
    "ll_rle", "of_rle", "ml_rle", "ll_repeat", "of_repeat", "ml_repeat", "seq_count_0", "seq_count_1", "seq_count_2",
    "seq_count_3", "fcs_0", "fcs_1", "fcs_2", "fcs_4", "fcs_8", "single_segment", "window_descriptor", "checksum",
    "skippable_before", "skippable_after_a_frame", "two_frames", "three_blocks", "block_of_128k",
    "rep1_ll0", "rep1_lln", "rep2_ll0", "rep2_lln", "rep3_ll0", "rep3_lln",
    "overlap_1", "overlap_2", "overlap_3", "overlap_63", "overlap_64", "overlap_65",
    "ll_log_9", "ml_log_9", "of_log_8", "match_across_blocks",
    "huffman_literals_1_stream_3", "huffman_literals_4_stream_3", "huffman_literals_4_stream_4", "huffman_literals_4_stream_5",
    "treeless_literals_1_stream_3", "treeless_literals_4_stream_3", "weights_direct", "weights_fse", "weights_log_5", "weights_log_6",
    "huffman_depth_11",
}
# what libzstd's own frames (tests/zstd_fixtures.py) must show as well
LEGAL_FORMS_FROM_LIBZSTD = {
    "huffman_literals_1_stream_3", "huffman_literals_4_stream_3", "huffman_literals_4_stream_4", "huffman_literals_4_stream_5",
    "weights_fse",
}


def _tiny_huffman(data, streams, **kw):
    w, log = huf_weights(huf_lengths(b"abcabcaab"))
    return literals_huffman(data, streams, 3, weights_fse(w, 5), huf_codes(w, log), **kw)


def illegal_plans():
    """-> [(name, chunk)]: one per check of the decoder that a header-level or sequence-level plan can reach."""
    text = b"It was the best of times, it was the worst of times. " * 20
    good = frame([("raw", text[:100]), ("rle", 0x41, 50)], checksum=True)[0]
    out = [("bad_magic", b"\x27" + good[1:]), ("reserved_frame_bit", frame([("raw", text[:10])], reserved=1)[0]),
           ("dictionary", frame([("raw", text[:10])], dict_id=7)[0]), ("checksum_wrong", good[:-1] + bytes([good[-1] ^ 1])),
           ("checksum_missing", good[:-4]), ("trailing_bytes", good + b"\x00\x00"), ("truncated_in_block", good[:40]),
           ("window_too_large", struct.pack("<IBB", MAGIC, 0, 22 << 3) + block(0, b"abc", True))]
    h = frame_header(10, single_segment=True, fcs_bytes=1)
    out += [("reserved_block_type", h + block(3, b"0123456789", True)), ("content_size_too_small", h + block(0, b"0123456789A", True)),
            ("content_size_too_large", h + block(0, b"012345678", True)), ("block_past_the_end", h + block(0, b"0123456", True, 10)),
            ("no_last_block", h + block(0, b"0123456789", False)), ("skippable_past_the_end", struct.pack("<II", 0x184D2A50, 9) + b"12345678"),
            ("compressed_block_of_128k", frame_header(None, window_log=20) + block(2, bytes(BLOCK_MAX), True)),
            ("compressed_block_too_short", h + block(2, b"\x00\x00", True))]
    lits = text[:200]

    def one(seq_bytes, lit=literals_raw(lits)):
        return frame_header(None, window_log=17) + block(2, lit + seq_bytes, True)
    c = SeqCoder()
    ok = c.section([(5, 10, 3 + 5), (3, 4, 1)])
    out += [("offset_before_the_start", one(SeqCoder().section([(5, 10, 3 + 6)]))),
            ("offset_before_the_frame", frame([("raw", text)])[0] + one(SeqCoder().section([(5, 10, 3 + 6)]))),
            ("literals_run_out", one(SeqCoder().section([(150, 10, 4), (60, 3, 4)]))),
            ("sequences_bitstream_no_marker", one(ok[:-1] + b"\x00")),
            ("repeat_mode_without_tables", one(SeqCoder().section([(5, 10, 8)])[:1] + bytes([0xFC]) + ok[2:])),
            ("rle_symbol_too_large", one(bytes([1, 1 << 6, 36, 0x01]))),
            ("zero_sequences_with_bytes", one(b"\x00\x00")),
            ("sequence_count_cut", one(b"\xff\x00")),
            ("fse_log_too_large", one(bytes([1, 2 << 4, 0x0F, 0x00, 0x01]))),
            ("literals_past_the_block", frame_header(None, window_log=17) + block(2, literals_raw(lits)[:50], True)),
            ("treeless_without_a_tree", one(b"\x00", lit=struct.pack("<I", 3 | 1 << 2 | 20 << 4 | 10 << 14)[:3] + bytes(10))),
            ("huffman_depth_12", one(b"\x00", lit=literals_huffman(bytes([0, 1, 2, 3] * 50), 1, 3, weights_direct([11, 11, 11, 11]),
                                                                   huf_codes([11, 11, 11, 11], 12)))),
            ("four_streams_for_5_literals", one(b"\x00", lit=_tiny_huffman(b"abcab", 4))),
            ("huffman_stream_with_a_bit_too_many", one(b"\x00", lit=_tiny_huffman(b"abcabcaab" * 9, 1, extra_low_bits=[(1, 1)]))),
            ("huffman_weights_sum", one(b"\x00", lit=struct.pack("<I", 2 | 20 << 4 | 10 << 14)[:3] + bytes([128 + 2, 0x12, 0x30]) + bytes(6)))]
    return out


def documented_differences():
    """-> [(name, chunk)]: chunks that libzstd 1.4.8 accepts and this decoder refuses, one per documented difference of
    include/hipcomp/zstd.h that a plan can reach."""
    text = b"It was the best of times, it was the worst of times. " * 20
    lits = text[:200]
    ok = SeqCoder().section([(5, 10, 3 + 5), (3, 4, 1)])
    # one byte more at the low end of the sequences' bitstream: 8 bits that no sequence reads
    return [("sequences_bitstream_not_exactly_consumed",
             frame_header(None, window_log=17) + block(2, literals_raw(lits) + ok[:2] + b"\x55" + ok[2:], True)),
            # weights 2, 1 and the implied 1, the bitstream one bit short of its two 5-bit states
            ("fse_weights_shorter_than_their_initial_states",
             frame_header(None, window_log=17) + block(2, literals_huffman(bytes([0, 1, 2, 2, 1, 0] * 20), 1, 3,
                                                                             weights_fse([2, 1, 1], 5, short_by=1), huf_codes([2, 1, 1], 2)) + b"\x00", True))]


def libzstd_frame_with_overread(frames):
    """A frame of libzstd's own (tests/zstd_fixtures.py, text at level 3) with one bit flipped in its sequences section:
    the walk then reads past the bitstream's start, which libzstd 1.4.8 tolerates (documented difference 1)."""
    chunk, content = next((c, d) for n, c, d in frames if n == "text_level_3")
    b = bytearray(chunk)
    b[OVERREAD_AT] ^= 1
    return bytes(b), len(content)


OVERREAD_AT = 293   # inside the first block's sequences bitstream (tests/test_zstd_tables_cpu.py asserts that)
