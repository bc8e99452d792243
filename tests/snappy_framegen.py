"""Snappy framed streams (.sz; magic ff 06 00 00 "sNaPpY") in pure Python for the tests of the Snappy manager's
framed-stream methods (hipcomp/snappy.hpp): CRC-32C and its mask, chunk builders, a small Snappy block writer and
decoder, a stream parser and decoder with the reason codes of csrc/snappy_frame.hpp, and a planner of streams -- legal
ones of every form the reader takes and hostile ones for every refusal it owes, by name, with truncations at every
structural boundary.  tests/test_snappy_framegen_cpu.py holds it to the CRC test vectors and to pyarrow's Snappy
codec."""
import struct
import zlib
from dataclasses import dataclass

import numpy as np

IDENTIFIER = b"\xff\x06\x00\x00sNaPpY"
MAX_CONTENT = 65536
SUCCESS, CANNOT_DECOMPRESS, BAD_CHECKSUM = 0, 12, 13
# csrc/snappy_frame.hpp, enum Reason
REASONS = {"ok": 0, "truncated": 1, "no_identifier": 2, "bad_identifier": 3, "reserved_unskippable": 4, "short_chunk": 5,
           "no_payload": 6, "bad_preamble": 7, "preamble_too_large": 8, "stored_too_large": 9, "bad_block": 10,
           "size_mismatch": 11, "bad_checksum": 12}
# what shows without decoding: configure_frame_decompression refuses these
WALK_REASONS = ("truncated", "no_identifier", "bad_identifier", "reserved_unskippable", "short_chunk", "no_payload",
                "bad_preamble", "preamble_too_large", "stored_too_large")
M = 0xFFFFFFFF


# ---- CRC-32C ---------------------------------------------------------------------------------------------------
POLY = 0x82F63B78


def _table():
    t = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
        t.append(c)
    return t


_T = _table()
_TN = np.array(_T, dtype=np.uint32)


def _mulmod(a, b):
    """a * b mod P, bit-reflected (bit 31 is x^0)"""
    p = 0
    for k in range(31, -1, -1):
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def _x8n(n):
    """x^(8n) mod P"""
    r, p = 1 << 31, 1 << 23   # x^0, x^8
    while n:
        if n & 1:
            r = _mulmod(r, p)
        p = _mulmod(p, p)
        n >>= 1
    return r


def _lockstep(rows, init):
    """the CRC registers after the rows of a (K, L) byte array, all K at once; init: the K start values"""
    reg = init.copy()
    for j in range(rows.shape[1]):
        reg = (reg >> np.uint32(8)) ^ _TN[(reg ^ rows[:, j]) & np.uint32(0xFF)]
    return reg


def _bytewise(reg, data):
    for b in data:
        reg = (reg >> 8) ^ _T[(reg ^ b) & 0xFF]
    return reg


def crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli) of data.  Long inputs: 256 segments in lockstep, joined by reg(A || B, i) =
    reg(A, i) * x^(8|B|) ^ reg(B, 0)."""
    n = len(data)
    if n < 4096:
        return _bytewise(M, data) ^ M
    K = 256
    L = n // K
    rows = np.frombuffer(data, dtype=np.uint8, count=K * L).reshape(K, L)
    init = np.zeros(K, dtype=np.uint32)
    init[0] = M
    regs = _lockstep(rows, init).tolist()
    shift, acc = _x8n(L), regs[0]
    for r in regs[1:]:
        acc = _mulmod(acc, shift) ^ r
    return _bytewise(acc, data[K * L:]) ^ M


def crc32c_many(pieces):
    """[crc32c(p) for p in pieces]; pieces of one length go in lockstep (40 960 chunks of 1024 bytes take a second)"""
    out, by_len = [None] * len(pieces), {}
    for i, p in enumerate(pieces):
        by_len.setdefault(len(p), []).append(i)
    for n, idx in by_len.items():
        if len(idx) < 16 or n == 0:
            for i in idx:
                out[i] = crc32c(pieces[i])
            continue
        rows = np.frombuffer(b"".join(pieces[i] for i in idx), dtype=np.uint8).reshape(len(idx), n)
        regs = _lockstep(rows, np.full(len(idx), M, dtype=np.uint32))
        for i, r in zip(idx, regs.tolist()):
            out[i] = r ^ M
    return out


def mask(c: int) -> int:
    return (((c >> 15) | (c << 17)) + 0xa282ead8) & M


def unmask(m: int) -> int:
    r = (m - 0xa282ead8) & M
    return ((r >> 17) | (r << 15)) & M


# ---- Snappy blocks ---------------------------------------------------------------------------------------------
def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def literal(data: bytes) -> bytes:
    n = len(data) - 1
    if n < 60:
        return bytes([n << 2]) + data
    k = (n.bit_length() + 7) // 8
    return bytes([(59 + k) << 2]) + n.to_bytes(k, "little") + data


def copy(offset: int, length: int) -> bytes:
    """a copy element with a 2-byte offset, 1 <= length <= 64"""
    return bytes([((length - 1) << 2) | 2]) + struct.pack("<H", offset)


def block_of(content: bytes, declared=None) -> bytes:
    """A raw Snappy block of content by a small greedy matcher (not the library's encoder: blocks of the tests' own)."""
    out = bytearray(varint(len(content) if declared is None else declared))
    table, i, lit, n = {}, 0, 0, len(content)
    while i + 4 <= n:
        key = content[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is not None and i - cand <= 65535:
            m = 4
            while i + m < n and m < 64 and content[cand + m] == content[i + m]:
                m += 1
            if lit < i:
                out += literal(content[lit:i])
            out += copy(i - cand, m)
            i += m
            lit = i
        else:
            i += 1
    if lit < n:
        out += literal(content[lit:])
    return bytes(out)


def read_varint(buf: bytes, at: int, room: int):
    """(value, bytes) of the varint at buf[at, at + room), or None where it does not end within 5 bytes and room"""
    value = 0
    for k in range(min(5, room)):
        b = buf[at + k]
        value |= (b & 0x7F) << (7 * k)
        if not b & 0x80:
            return value, k + 1
    return None


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


def decode_block(block: bytes) -> bytes:
    """The block's bytes.  Refused("bad_block") where a decoder must refuse, Refused("size_mismatch") where the
    elements give another size than the preamble."""
    pre = read_varint(block, 0, len(block))
    if pre is None:
        raise Refused("bad_block")
    want, c = pre
    out, end = bytearray(), len(block)
    while c < end:
        tag = block[c]
        c += 1
        kind, n6 = tag & 3, tag >> 2
        if kind == 0:
            n = n6 + 1
            if n6 >= 60:
                k = n6 - 59
                if end - c < k:
                    raise Refused("bad_block")
                n = int.from_bytes(block[c:c + k], "little") + 1
                c += k
            if n > end - c:
                raise Refused("bad_block")
            out += block[c:c + n]
            c += n
        else:
            if kind == 1:
                if end - c < 1:
                    raise Refused("bad_block")
                n, off = 4 + (n6 & 7), ((n6 >> 3) << 8) | block[c]
                c += 1
            else:
                k = 2 if kind == 2 else 4
                if end - c < k:
                    raise Refused("bad_block")
                n, off = n6 + 1, int.from_bytes(block[c:c + k], "little")
                c += k
            if off == 0 or off > len(out):
                raise Refused("bad_block")
            for _ in range(n):
                out.append(out[-off])
        if len(out) > want:
            raise Refused("size_mismatch")
    if len(out) != want:
        raise Refused("size_mismatch")
    return bytes(out)


# ---- chunks and streams ----------------------------------------------------------------------------------------
def chunk(kind: int, body: bytes) -> bytes:
    return bytes([kind]) + len(body).to_bytes(3, "little") + body


def stored_chunk(content: bytes, crc=None) -> bytes:
    return chunk(1, struct.pack("<I", mask(crc32c(content)) if crc is None else crc) + content)


def compressed_chunk(block: bytes, content: bytes, crc=None) -> bytes:
    return chunk(0, struct.pack("<I", mask(crc32c(content)) if crc is None else crc) + block)


def padding(n: int, kind: int = 0xfe) -> bytes:
    return chunk(kind, bytes((7 * i + kind) & 0xFF for i in range(n)))


def written_stream(chunks, blocks) -> bytes:
    """The stream compress_frame owes for these chunks and the batched encoder's blocks of them."""
    out = [IDENTIFIER]
    for c, b, crc in zip(chunks, blocks, crc32c_many(chunks)):
        out.append(compressed_chunk(b, c, mask(crc)) if len(b) < len(c) else stored_chunk(c, mask(crc)))
    return b"".join(out)


def parse_chunk(buf: bytes, at: int, first: bool):
    """csrc/snappy_frame.hpp, parse_chunk, said again: (kind, bytes, payload, content, crc) of the chunk at buf[at];
    kind "skipped" / "compressed" / "stored".  Refused(reason) in the header's order of tests."""
    avail = len(buf) - at
    if avail < 4:
        raise Refused("truncated")
    kind, length = buf[at], int.from_bytes(buf[at + 1:at + 4], "little")
    if first and kind != 0xff:
        raise Refused("no_identifier")
    if kind == 0xff:
        if length != 6:
            raise Refused("bad_identifier")
        if avail < 10:
            raise Refused("truncated")
        if buf[at:at + 10] != IDENTIFIER:
            raise Refused("bad_identifier")
        return "skipped", 10, 0, 0, 0
    if 0x02 <= kind <= 0x7f:
        raise Refused("reserved_unskippable")
    if kind >= 0x80:
        if length > avail - 4:
            raise Refused("truncated")
        return "skipped", 4 + length, 0, 0, 0
    if length < 4:
        raise Refused("short_chunk")
    if kind == 1 and length - 4 > MAX_CONTENT:
        raise Refused("stored_too_large")
    if length > avail - 4:
        raise Refused("truncated")
    crc, = struct.unpack_from("<I", buf, at + 4)
    if kind == 1:
        return "stored", 4 + length, length - 4, length - 4, crc
    if length == 4:
        raise Refused("no_payload")
    pre = read_varint(buf, at + 8, length - 4)
    if pre is None:
        raise Refused("bad_preamble")
    if pre[0] > MAX_CONTENT:
        raise Refused("preamble_too_large")
    return "compressed", 4 + length, length - 4, pre[0], crc


def parse(buf: bytes):
    """[(kind, payload bytes, declared content bytes, stored crc)] of the data chunks; Refused(reason)"""
    out, at = [], 0
    while at < len(buf):
        kind, n, payload, content, crc = parse_chunk(buf, at, at == 0)
        if kind != "skipped":
            out.append((kind, buf[at + 8:at + 8 + payload], content, crc))
        at += n
    return out


def decode(buf: bytes, verify: bool, block_decoder=decode_block):
    """(reason, content or None): the verdict decompress_frame owes.  Every chunk is looked at: a CRC that does not
    fit (where verified, and only of a chunk that decoded) wins over a chunk that does not decode."""
    try:
        chunks = parse(buf)
    except Refused as r:
        return r.reason, None
    out, failed, decoded = bytearray(), None, []
    for kind, payload, content, crc in chunks:
        try:
            data = payload if kind == "stored" else block_decoder(payload)
            if len(data) != content:
                raise Refused("size_mismatch")
        except Refused as r:
            failed = failed or r.reason
            out += bytes(content)
            continue
        out += data
        decoded.append((data, crc))
    bad_crc = verify and any(mask(c) != crc for c, (_, crc) in zip(crc32c_many([d for d, _ in decoded]), decoded))
    if bad_crc:
        return "bad_checksum", None
    if failed:
        return failed, None
    return "ok", bytes(out)


# ---- the planner -----------------------------------------------------------------------------------------------
@dataclass
class Plan:
    name: str
    data: bytes
    content: bytes = b""     # legal plans and plans with a CRC that does not fit: what the input decodes to
    reason: str = "ok"       # why the reader refuses it whatever the policy (REASONS)
    chunks: int = 0          # data chunks, where the walk accepts the input
    declared: int = 0        # the sum of the stored lengths and the preambles, where the walk accepts the input
    bad_crc: bool = False    # a data chunk's CRC does not fit: BadChecksum where verified
    truncated_at: str = ""   # the structural boundary a truncation cuts at

    def status(self, policy: int) -> int:
        """hipcompStatus_t decompress_frame owes under the ChecksumPolicy."""
        if self.bad_crc and policy in (2, 3, 4):
            return BAD_CHECKSUM
        return SUCCESS if self.reason == "ok" else CANNOT_DECOMPRESS

    def expected_reason(self, verify: bool) -> str:
        return "bad_checksum" if self.bad_crc and verify else self.reason

    @property
    def configures(self) -> bool:
        return self.reason not in WALK_REASONS


def text(n, salt=0):
    words = [b"stream", b"chunk", b"snappy", b"wave", b"lane", b"offset", b"literal", b"copy", b"frame", b"chain"]
    out, k = bytearray(), salt + 1
    while len(out) < n:
        k = (k * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[(k >> 8) % len(words)] + b" "
    return bytes(out[:n])


def noise(n, salt=0):
    return np.random.default_rng(1000 + salt).integers(0, 256, n, dtype=np.uint8).tobytes()


SMALLEST = bytes.fromhex("ff060000734e61507059010d0000e5b08ac7313233343536373839")
MANY_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 65535, 65536)


def _many_chunks():
    """About 300 chunks, stored and compressed in turn, of the edge lengths and random ones, ordered so that the
    output offsets meet every residue mod 16 (asserted): (stream, content, count)."""
    rng = np.random.default_rng(5)
    lengths = list(MANY_LENGTHS) * 2
    lengths += [int(x) for x in rng.integers(1, 3000, 300 - len(lengths))]
    # odd lengths first walk the offsets through the residues; the rest follow shuffled
    lengths = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1] + [lengths[i] for i in rng.permutation(len(lengths))]
    parts, content, residues, at = [IDENTIFIER], bytearray(), set(), 0
    for k, n in enumerate(lengths):
        c = text(n, k) if k % 3 else noise(n, k)
        residues.add(at % 16)
        at += n
        content += c
        parts.append(stored_chunk(c) if k % 2 else compressed_chunk(block_of(c), c))
        if k % 50 == 49:
            parts.append(padding(k % 7))
    assert residues == set(range(16))
    return b"".join(parts), bytes(content), len(lengths)


def legal_plans():
    plans = []

    def add(name, data, content, chunks):
        plans.append(Plan(name, data, content=content, chunks=chunks, declared=len(content)))
    add("smallest", SMALLEST, b"123456789", 1)
    add("identifier_only", IDENTIFIER, b"", 0)
    add("no_bytes", b"", b"", 0)
    for n in (1, 65536):
        t, z = text(n, n), noise(n, n)
        add("compressed_%d" % n, IDENTIFIER + compressed_chunk(block_of(t), t), t, 1)
        add("stored_%d" % n, IDENTIFIER + stored_chunk(z), z, 1)
    # all literals: the block (preamble, literal tag with a length field) is longer than its content
    z = noise(300, 3)
    b = varint(300) + literal(z)
    assert len(b) > len(z) and decode_block(b) == z
    add("block_longer_than_content", IDENTIFIER + compressed_chunk(b, z), z, 1)
    add("stored_empty", IDENTIFIER + stored_chunk(b"") + stored_chunk(b"x"), b"x", 2)
    add("preamble_zero", IDENTIFIER + compressed_chunk(b"\x00", b"") + stored_chunk(b"y"), b"y", 2)
    add("preamble_zero_two_bytes", IDENTIFIER + compressed_chunk(b"\x80\x00", b""), b"", 1)
    t = text(500, 9)
    one = compressed_chunk(block_of(t), t)
    for n in (0, 1, 70000):
        add("padding_%d" % n, IDENTIFIER + padding(n) + one + padding(n), t, 1)
    for kind in (0x80, 0xfd):
        add("skippable_%02x" % kind, IDENTIFIER + one + padding(33, kind) + stored_chunk(t[:77]), t + t[:77], 2)
    add("repeated_identifier", IDENTIFIER + IDENTIFIER + one + IDENTIFIER + one + IDENTIFIER, t + t, 2)
    add("two_streams", SMALLEST + IDENTIFIER + one, b"123456789" + t, 2)
    add("padding_last_short", IDENTIFIER + one + padding(3), t, 1)
    stream, content, count = _many_chunks()
    add("many_chunks", stream, content, count)
    return plans


def hostile_plans():
    t, z = text(500, 9), noise(200, 4)
    good = compressed_chunk(block_of(t), t)
    plans = []

    def add(name, data, reason, **kw):
        plans.append(Plan(name, data, reason=reason, **kw))
    add("no_identifier", good, "no_identifier")
    add("padding_first", padding(4) + IDENTIFIER + good, "no_identifier")
    add("identifier_length_5", chunk(0xff, b"sNaPp") + good, "bad_identifier")
    add("identifier_length_7", chunk(0xff, b"sNaPpY!") + good, "bad_identifier")
    add("identifier_body", chunk(0xff, b"sNaPpy") + good, "bad_identifier")
    add("second_identifier_body", IDENTIFIER + good + chunk(0xff, b"SNaPpY") + good, "bad_identifier")
    for kind in (0x02, 0x7f):
        add("reserved_%02x" % kind, IDENTIFIER + good + chunk(kind, b"abcd"), "reserved_unskippable")
    add("body_runs_out_stored", IDENTIFIER + stored_chunk(z)[:-1], "truncated")
    add("body_runs_out_padding", IDENTIFIER + good + padding(9)[:-2], "truncated")
    add("header_runs_out", IDENTIFIER + good + b"\x00\x10", "truncated")
    for kind in (0, 1):
        for n in (0, 3):
            add("short_chunk_%d_%d" % (kind, n), IDENTIFIER + chunk(kind, b"\x01\x02\x03"[:n]) + good, "short_chunk")
    add("no_payload", IDENTIFIER + chunk(0, b"\x00\x00\x00\x00") + good, "no_payload")
    add("preamble_incomplete_1", IDENTIFIER + compressed_chunk(b"\x80", b""), "bad_preamble")
    add("preamble_incomplete_2", IDENTIFIER + compressed_chunk(b"\xff\xff", b"") + good, "bad_preamble")
    add("preamble_6_bytes", IDENTIFIER + compressed_chunk(b"\x80\x80\x80\x80\x80\x00", b""), "bad_preamble")
    add("preamble_65537", IDENTIFIER + compressed_chunk(block_of(t, declared=65537), t), "preamble_too_large")
    add("preamble_2_32_plus_5", IDENTIFIER + compressed_chunk(b"\x85\x80\x80\x80\x10" + literal(b"12345"), b"12345"),
        "preamble_too_large")
    add("stored_65537", IDENTIFIER + stored_chunk(noise(65537, 6)), "stored_too_large")
    # blocks that do not decode: the walk takes them
    two = dict(chunks=2, declared=600)
    add("block_garbage", IDENTIFIER + compressed_chunk(varint(100) + b"\xfe\xfd\xfc" + z[:20], b"") + stored_chunk(t), "bad_block",
        **two)
    early = varint(100) + literal(b"abcdefgh") + copy(9, 60) + literal(t[:32])
    add("match_before_chunk", IDENTIFIER + compressed_chunk(early, b"") + stored_chunk(t), "bad_block", **two)
    # the second chunk's match would land in the first chunk's output: chunks do not see each other's
    add("match_into_chunk_before", IDENTIFIER + stored_chunk(t) + compressed_chunk(early, b""), "bad_block", **two)
    add("literal_runs_out", IDENTIFIER + compressed_chunk(varint(100) + literal(t[:100])[:-5], b"") + stored_chunk(t), "bad_block",
        **two)
    add("decodes_short", IDENTIFIER + compressed_chunk(block_of(t[:90], declared=100), b"") + stored_chunk(t), "size_mismatch", **two)
    add("decodes_long", IDENTIFIER + compressed_chunk(block_of(t[:110], declared=100), b"") + stored_chunk(t), "size_mismatch",
        **two)
    # CRCs that do not fit: refused where they are verified
    crc = crc32c(t)
    ok = dict(content=t + z, chunks=2, declared=len(t + z))
    add("wrong_crc_stored", IDENTIFIER + good + stored_chunk(z, mask(crc32c(z)) ^ 1), "ok", bad_crc=True, **ok)
    add("wrong_crc_compressed", IDENTIFIER + compressed_chunk(block_of(t), t, mask(crc) ^ 0x80000000) + stored_chunk(z), "ok",
        bad_crc=True, **ok)
    add("unmasked_crc", IDENTIFIER + compressed_chunk(block_of(t), t, crc) + stored_chunk(z), "ok", bad_crc=True, **ok)
    add("ieee_crc_masked", IDENTIFIER + good + stored_chunk(z, mask(zlib.crc32(z))), "ok", bad_crc=True, **ok)
    add("wrong_crc_and_bad_block", IDENTIFIER + stored_chunk(z, 12345) + compressed_chunk(early, b"") + good, "bad_block",
        bad_crc=True, chunks=3, declared=len(z) + 100 + len(t))
    return plans


TRUNCATION_POINTS = ("inside_identifier_header", "inside_identifier", "inside_header", "inside_crc", "inside_preamble",
                     "inside_body", "inside_stored_body")


def truncation_plans():
    """One stream with both kinds of data chunk, cut inside every part; cut between two chunks it is a stream."""
    t = text(500, 9)
    first = compressed_chunk(block_of(t), t)
    assert first[8] & 0x80, "the preamble has two bytes"
    whole = IDENTIFIER + first + stored_chunk(t[:64])
    cuts = {"inside_identifier_header": 2, "inside_identifier": 7, "inside_header": 12, "inside_crc": 16, "inside_preamble": 19,
            "inside_body": 10 + len(first) - 1, "inside_stored_body": len(whole) - 10}
    assert tuple(cuts) == TRUNCATION_POINTS
    plans = [Plan("whole", whole, content=t + t[:64], chunks=2, declared=564),
             Plan("cut_between_chunks", whole[:10 + len(first)], content=t, chunks=1, declared=500)]
    for name, cut in cuts.items():
        plans.append(Plan("cut_" + name, whole[:cut], reason="truncated", truncated_at=name))
    return plans


def all_plans(cache=[]):
    if not cache:
        cache.extend(legal_plans() + hostile_plans() + truncation_plans())
    return list(cache)
