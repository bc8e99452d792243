"""The chunk index of a seekable Snappy framed stream (csrc/snappy_frame_index.hpp; INTEGRATION.md, "Seekable Snappy
framed streams") in pure Python for the tests of the Snappy manager's indexed framed-stream methods, on top of
snappy_framegen: a writer and a parser of the index that give the header's reason codes, and a planner of indexed
inputs by name -- legal ones of every form and one forged one for every refusal -- each with the reason its index
should or should not apply.  Every planned input is a sound or unsound .sz stream in its own right: a reader that
knows nothing of the index steps over it as a reserved skippable chunk, and what the planner expects of every input
is what snappy_framegen's parser and decoder say of the same bytes.  tests/test_snappy_frame_index_cpu.py holds all
of it to the header and to pyarrow's Snappy codec."""
import struct
from dataclasses import dataclass

import snappy_framegen as G

INDEX_TYPE = 0xa5
SIGNATURE = b"HCSNPIDX"
MAX_CHUNKS = (0xFFFFFF - 36) // 4
MAX_UNITS = 32
# csrc/snappy_frame_index.hpp, enum IndexReason
REASONS = {"ok": 0, "not_there": 1, "length": 2, "signature": 3, "version": 4, "flags": 5, "chunk_bytes": 6, "count": 7,
           "crc": 8, "type": 9, "offset": 10, "word": 11, "stored_length": 12, "no_payload": 13, "preamble": 14,
           "behind": 15, "decode": 16, "too_many_units": 17}
# only the device meets these: the decode of a block, the size of the reader's unit table
DEVICE_REASONS = ("decode", "too_many_units")


def index_bytes(n):
    return 40 + 4 * n


def index_chunk(words, chunk_bytes, content_bytes, *, kind=INDEX_TYPE, signature=SIGNATURE, version=1, flags=0, n=None,
                length=None, crc="masked", pad=b"") -> bytes:
    """The index of a stream whose data chunks begin with these words; the keywords forge single fields (the CRC fits
    them unless crc is "wrong" or "unmasked"), pad: bytes behind the CRC that the length field counts."""
    n = len(words) if n is None else n
    body = signature + struct.pack("<IIIIQ", version, flags, chunk_bytes, n, content_bytes) + struct.pack("<%dI" % len(words), *words)
    c = G.crc32c(body)
    c = {"masked": G.mask(c), "wrong": G.mask(c) ^ 0x10, "unmasked": c}[crc]
    body += struct.pack("<I", c) + pad
    return bytes([kind]) + (len(body) if length is None else length).to_bytes(3, "little") + body


def data_words(stream: bytes):
    """The first four bytes of the data chunks of a stream the walk accepts, as little-endian words."""
    out, at = [], 0
    while at < len(stream):
        kind, n, _, _, _ = G.parse_chunk(stream, at, at == 0)
        if kind != "skipped":
            out.append(struct.unpack_from("<I", stream, at)[0])
        at += n
    return out


def parse_index(buf: bytes, at: int):
    """csrc/snappy_frame_index.hpp, parse_index_fields and index_crc_fits, said again: (reason, head)"""
    avail = len(buf) - at
    if avail < 4 or buf[at] != INDEX_TYPE:
        return "not_there", None
    length = int.from_bytes(buf[at + 1:at + 4], "little")
    if length < 36 or length > avail - 4:
        return "length", None
    if buf[at + 4:at + 12] != SIGNATURE:
        return "signature", None
    version, flags, chunk_bytes, n, content = struct.unpack_from("<IIIIQ", buf, at + 12)
    if version != 1:
        return "version", None
    if flags:
        return "flags", None
    if chunk_bytes == 0 or chunk_bytes > G.MAX_CONTENT:
        return "chunk_bytes", None
    if length != 36 + 4 * n:
        return "length", None
    if -(-content // chunk_bytes) != n:
        return "count", None
    if G.mask(G.crc32c(buf[at + 4:at + 36 + 4 * n])) != struct.unpack_from("<I", buf, at + 36 + 4 * n)[0]:
        return "crc", None
    return "ok", {"chunk_bytes": chunk_bytes, "chunks": n, "content_bytes": content,
                  "words": list(struct.unpack_from("<%dI" % n, buf, at + 36))}


def index_applies(buf: bytes, at: int):
    """index_applies of the header: (reason, the byte behind the last data chunk, head)"""
    if buf[at:at + 10] != G.IDENTIFIER:
        return "not_there", None, None
    reason, h = parse_index(buf, at + 10)
    if reason != "ok":
        return reason, None, None
    pos, n = at + 10 + index_bytes(h["chunks"]), h["chunks"]
    for i, word in enumerate(h["words"]):
        kind, length = word & 0xFF, word >> 8
        if kind not in (0, 1):
            return "type", None, h
        if len(buf) - pos < 4 + length:
            return "offset", None, h
        if struct.unpack_from("<I", buf, pos)[0] != word:
            return "word", None, h
        share = h["chunk_bytes"] if i + 1 < n else h["content_bytes"] - h["chunk_bytes"] * i
        if kind == 1:
            if length != 4 + share:
                return "stored_length", None, h
        else:
            if length <= 4:
                return "no_payload", None, h
            pre = G.read_varint(buf, pos + 8, length - 4)
            if pre is None or pre[0] != share:
                return "preamble", None, h
        pos += 4 + length
    return "ok", pos, h


def step_behind(buf: bytes, pos: int):
    """step_behind_unit of the header: (reason, pos, an identifier stands there)"""
    while pos < len(buf):
        try:
            kind, n, _, _, _ = G.parse_chunk(buf, pos, False)
        except G.Refused:
            return "behind", pos, False
        if kind != "skipped":
            return "behind", pos, False
        if buf[pos] == 0xff:
            return "ok", pos, True
        pos += n
    return "ok", pos, False


def input_is_indexed(buf: bytes):
    """input_is_indexed of the header: (reason, units, chunks, content bytes)"""
    pos, units, chunks, content, more = 0, 0, 0, 0, True
    while more:
        reason, end, h = index_applies(buf, pos)
        if reason != "ok":
            return reason, units, chunks, content
        units, chunks, content = units + 1, chunks + h["chunks"], content + h["content_bytes"]
        reason, pos, more = step_behind(buf, end)
        if reason != "ok":
            return reason, units, chunks, content
    return "ok", units, chunks, content


# ---- streams of the form compress_frame writes -------------------------------------------------------------------
def pieces_of(content: bytes, chunk_bytes: int):
    return [content[i:i + chunk_bytes] for i in range(0, len(content), chunk_bytes)]


def data_chunks(pieces, kinds):
    """one data chunk per piece: kinds[i % len(kinds)] "c" compressed (a block of the tests' own writer) / "s" stored"""
    crcs = G.crc32c_many(pieces)
    return [G.compressed_chunk(G.block_of(p), p, G.mask(c)) if kinds[i % len(kinds)] == "c" else G.stored_chunk(p, G.mask(c))
            for i, (p, c) in enumerate(zip(pieces, crcs))]


def unit_of(chunks, chunk_bytes, content_bytes, **forge) -> bytes:
    """identifier, the index of these data chunks, the chunks"""
    words = [struct.unpack_from("<I", c)[0] for c in chunks]
    return G.IDENTIFIER + index_chunk(words, chunk_bytes, content_bytes, **forge) + b"".join(chunks)


def written_form(content: bytes, chunk_bytes: int, kinds="cs", **forge) -> bytes:
    return unit_of(data_chunks(pieces_of(content, chunk_bytes), kinds), chunk_bytes, len(content), **forge)


def mixed(n, salt=0, period=256):
    """text and noise in turn, `period` bytes each"""
    out = bytearray()
    k = 0
    while len(out) < n:
        out += G.text(period, salt + k) if k % 2 == 0 else G.noise(period, salt + k)
        k += 1
    return bytes(out[:n])


# ---- the planner -----------------------------------------------------------------------------------------------
@dataclass
class IndexPlan:
    name: str
    data: bytes                   # the input with its index chunks
    reason: str                   # input_is_indexed's word on it (REASONS): "ok" -- every index applies by the host's tests
    why: str                      # what was done to it
    plain_reason: str = "ok"      # snappy_framegen's word on the same bytes, no CRC looked at (G.REASONS)
    content: bytes = b""          # what they decode to, where they do
    chunks: int = 0               # data chunks, where the walk accepts the input
    declared: int = 0             # the sum of the stored lengths and the preambles, where the walk accepts the input
    bad_crc: bool = False         # a data chunk's CRC does not fit: BadChecksum where verified
    device_refuses: str = ""      # the host's tests pass; the device refuses for this reason (DEVICE_REASONS)

    @property
    def applies(self) -> bool:
        """The indexed read takes it: no chunk is listed by the walk."""
        return self.reason == "ok" and not self.device_refuses

    @property
    def configures(self) -> bool:
        return self.plain_reason not in G.WALK_REASONS

    def status(self, policy: int) -> int:
        """hipcompStatus_t decompress_frame owes under the ChecksumPolicy."""
        if not self.configures:
            return G.CANNOT_DECOMPRESS
        if self.bad_crc and policy in (2, 3, 4):
            return G.BAD_CHECKSUM
        return G.SUCCESS if self.plain_reason == "ok" else G.CANNOT_DECOMPRESS


def plan_of(name, data, why, device_refuses="") -> IndexPlan:
    """The plan of an input: the index's verdict from this module, everything else from snappy_framegen."""
    p = IndexPlan(name, data, input_is_indexed(data)[0], why, device_refuses=device_refuses)
    p.plain_reason, content = G.decode(data, False)
    if p.configures:
        parsed = G.parse(data)
        p.chunks, p.declared = len(parsed), sum(c[2] for c in parsed)
    if content is not None:
        p.content = content
        p.bad_crc = G.decode(data, True)[0] == "bad_checksum"
    elif p.configures:
        p.bad_crc = G.decode(data, True)[0] == "bad_checksum"
    return p


CB = 256             # content bytes per data chunk of the planned units
GOOD_BYTES = 6 * CB + 100
KINDS = "cscscsc"    # seven data chunks: compressed, stored, compressed, ...


def _put(data: bytes, at: int, new: bytes) -> bytes:
    return data[:at] + new + data[at + len(new):]


def plans(cache=[]):
    if cache:
        return list(cache)
    out = []
    content = G.text(GOOD_BYTES, 1)
    chunks = data_chunks(pieces_of(content, CB), KINDS)
    words = [struct.unpack_from("<I", c)[0] for c in chunks]
    n = len(chunks)
    good = unit_of(chunks, CB, len(content))
    data_at = 10 + index_bytes(n)
    starts = [data_at + sum(len(c) for c in chunks[:i]) for i in range(n)]

    def add(name, data, reason, why, **kw):
        p = plan_of(name, data, why, **kw)
        assert p.reason == reason, (name, p.reason, reason)
        out.append(p)

    def forged(**kw):
        return unit_of(chunks, CB, len(content), **kw)

    def with_words(w, **kw):
        return G.IDENTIFIER + index_chunk(w, CB, len(content), **kw) + b"".join(chunks)

    # ---- legal inputs ----
    add("good", good, "ok", "one unit, a short last chunk")
    add("good_empty", G.IDENTIFIER + index_chunk([], CB, 0), "ok", "N = 0: the identifier and a 40-byte index")
    add("good_full_last", written_form(G.text(3 * CB, 2), CB, "sc"), "ok", "a last chunk of exactly chunk_bytes")
    add("chunk_bytes_1", written_form(b"seven b", 1, "sc"), "ok", "chunk_bytes 1: seven chunks of a byte, a block longer than its byte among them")
    add("chunk_bytes_1000", written_form(mixed(2500, 3, 500), 1000, "cs"), "ok", "chunk_bytes 1000")
    add("chunk_bytes_65536", written_form(G.text(65536, 4) + G.noise(1234, 5), 65536, "cs"), "ok", "chunk_bytes 65536, two chunks")
    second = written_form(G.text(2 * CB + 33, 6), CB, "scc")
    third = written_form(G.noise(CB + 1, 7), CB, "s")
    add("two_units", good + second, "ok", "two units back to back")
    add("three_units", good + second + third, "ok", "three units back to back")
    add("padding_between_units", good + G.padding(5) + second, "ok", "a padding chunk between two units")
    add("skippable_80_between_units", good + G.padding(9, 0x80) + second, "ok", "a reserved skippable chunk 0x80 between two units")
    add("skippable_fd_between_units", good + G.padding(0, 0xfd) + G.padding(70, 0xfd) + second, "ok", "two chunks 0xfd between two units")
    add("stray_index_between_units", good + index_chunk(words, CB, len(content)) + second, "ok",
        "an index that does not stand behind an identifier: a skippable chunk like any")
    add("padding_at_the_end", good + G.padding(3) + index_chunk([], 7, 0), "ok", "padding and a stray index behind the last unit")
    small = [written_form(bytes([65 + k, 66 + k, 67 + k]), 2, "sc") for k in range(MAX_UNITS + 1)]
    add("units_32", b"".join(small[:MAX_UNITS]), "ok", "as many units as the reader's table holds")
    add("units_33", b"".join(small), "ok", "one unit more than the reader's table holds", device_refuses="too_many_units")
    wrong = bytearray(good)
    wrong[starts[1] + 4] ^= 1
    add("wrong_data_crc_stored", bytes(wrong), "ok", "one bit of the stored chunk 1's CRC: no reason against the index")
    wrong = bytearray(good)
    wrong[starts[2] + 7] ^= 0x80
    add("wrong_data_crc_compressed", bytes(wrong), "ok", "one bit of the compressed chunk 2's CRC: no reason against the index")
    # ---- the index in itself ----
    add("wrong_signature", forged(signature=b"HCSNPIDY"), "signature", "the last letter of the signature")
    add("wrong_version", forged(version=2), "version", "version 2")
    add("reserved_flag", forged(flags=1), "flags", "flag bit 0")
    add("reserved_flag_31", forged(flags=1 << 31), "flags", "flag bit 31")
    add("chunk_bytes_zero", G.IDENTIFIER + index_chunk(words, 0, len(content)) + b"".join(chunks), "chunk_bytes", "chunk_bytes 0")
    add("chunk_bytes_65537", G.IDENTIFIER + index_chunk(words, 65537, len(content)) + b"".join(chunks), "chunk_bytes", "chunk_bytes 65537")
    add("n_too_large", with_words(words + [words[-1]]), "count", "N + 1 words")
    add("n_too_small", with_words(words[:-1]), "count", "N - 1 words")
    add("length_disagrees", forged(length=36 + 4 * n + 4, pad=b"\0\0\0\0"), "length", "four bytes more than 36 + 4N")
    add("length_below_36", G.IDENTIFIER + bytes([INDEX_TYPE]) + (35).to_bytes(3, "little") + bytes(35) + b"".join(chunks), "length",
        "a length field of 35")
    add("length_past_the_input", forged(n=0x3FFFF0, length=36 + 4 * 0x3FFFF0), "length", "N of 4 194 288: 4N bytes are not there")
    add("wrong_crc", forged(crc="wrong"), "crc", "one bit of the index's CRC flipped")
    add("unmasked_crc", forged(crc="unmasked"), "crc", "the CRC-32C without the format's mask")
    add("padding_before_index", G.IDENTIFIER + G.padding(2) + good[10:], "not_there", "a padding chunk between the identifier and the index")
    add("other_skippable_type", forged(kind=0xa4), "not_there", "the index under type 0xa4")
    add("no_identifier_before_second_index", good + good[10:], "behind", "a second index and its data chunks without an identifier")
    # ---- the words against the stream ----
    for delta in (1, -1):
        w = list(words)
        w[3] += delta << 8
        add("word_length_%s" % ("plus_1" if delta > 0 else "minus_1"), with_words(w), "word", "the length of word 3 changed by one")
    w = list(words)
    w[-1] += 1 << 8
    add("last_word_length_plus_1", with_words(w), "offset", "the length of the last word one more: the chunk would end behind the input")
    for i in (2, 3):
        w = list(words)
        w[i] ^= 1
        add("word_type_flipped_%d" % i, with_words(w), "word", "the type of word %d flipped between 0x00 and 0x01" % i)
    for kind in (0x02, 0x80, 0xfe, 0xff):
        w = list(words)
        w[4] = (w[4] & ~0xFF) | kind
        add("word_type_%02x" % kind, with_words(w), "type", "the type of word 4 is 0x%02x" % kind)
    empty = [chunks[0], G.chunk(0, b"\x00\x00\x00\x00"), chunks[2]]
    add("compressed_length_4", unit_of(empty, CB, 2 * CB + 10), "no_payload", "a compressed chunk that ends behind its CRC, word and stream alike")
    t = G.text(4 * CB, 8)
    short = data_chunks([t[:CB], t[CB:CB + 90], t[2 * CB:3 * CB], t[3 * CB:3 * CB + 200]], "cscs")
    add("stored_chunk_short", unit_of(short, CB, CB + 90 + CB + 200), "stored_length", "a stored chunk of 90 bytes where 256 are due")
    short = data_chunks([t[:CB], t[CB:CB + 128], t[2 * CB:3 * CB], t[3 * CB:3 * CB + 200]], "c")
    add("preamble_not_the_share", unit_of(short, CB, CB + 128 + CB + 200), "preamble", "a compressed chunk of 128 bytes where 256 are due")
    cut_varint = [chunks[0], G.compressed_chunk(b"\x80", b"")]
    add("preamble_incomplete", unit_of(cut_varint, CB, CB + 44), "preamble", "a preamble of one byte with its continuation bit")
    between = chunks[:3] + [G.padding(4)] + chunks[3:]
    add("padding_between_data_chunks", G.IDENTIFIER + index_chunk(words, CB, len(content)) + b"".join(between), "word",
        "a padding chunk between data chunks 2 and 3")
    between = chunks[:5] + [G.IDENTIFIER] + chunks[5:]
    add("identifier_between_data_chunks", G.IDENTIFIER + index_chunk(words, CB, len(content)) + b"".join(between), "word",
        "a repeated identifier between data chunks 4 and 5")
    # ---- what follows the unit ----
    add("data_chunk_behind_unit", good + G.stored_chunk(b"more"), "behind", "a data chunk the index does not list")
    add("unskippable_behind_unit", good + G.chunk(0x7f, b"abcd"), "behind", "a reserved unskippable chunk behind the unit")
    add("identifier_at_the_end", good + G.IDENTIFIER, "not_there", "an identifier with nothing behind it opens no unit")
    add("plain_stream_behind_unit", good + G.SMALLEST, "not_there", "a stream without an index behind the unit")
    add("plain_stream", G.IDENTIFIER + b"".join(chunks), "not_there", "no index at all")
    add("no_bytes", b"", "not_there", "an input of no bytes")
    # ---- truncations, in every structural place ----
    cuts = {"inside_identifier": 7, "behind_identifier": 10, "inside_index_header": 12, "inside_index_fields": 10 + 30,
            "inside_index_words": 10 + 36 + 9, "inside_index_crc": data_at - 2, "behind_index": data_at,
            "inside_data_header": starts[2] + 2, "inside_data_crc": starts[2] + 6, "inside_data_body": starts[3] - 1,
            "inside_last_chunk": len(good) - 1}
    reasons = {"inside_identifier": "not_there", "behind_identifier": "not_there", "inside_index_header": "not_there"}
    for name, cut in cuts.items():
        add("cut_" + name, good[:cut], reasons.get(name, "length" if cut < data_at else "offset"), "the good unit cut at byte %d" % cut)
    add("cut_between_data_chunks", good[:starts[4]], "offset", "the good unit cut in front of data chunk 4")
    add("cut_inside_padding_behind", good + G.padding(9)[:-2], "behind", "a padding chunk behind the unit, cut")
    add("cut_inside_second_unit", good + second[:30], "length", "a second unit cut inside its index")
    # ---- blocks only the decode can tell ----
    garbage = list(chunks)
    garbage[2] = G.compressed_chunk(G.varint(CB) + b"\xfe\xfd\xfc" + G.noise(40, 9), b"")
    add("damaged_block", unit_of(garbage, CB, len(content)), "ok", "a block of garbage behind a preamble that fits", device_refuses="decode")
    piece = content[4 * CB:5 * CB]
    short_block = list(chunks)
    short_block[4] = G.compressed_chunk(G.block_of(piece[:200], declared=CB), piece)
    add("block_decodes_short", unit_of(short_block, CB, len(content)), "ok", "a block of 200 bytes behind a preamble of 256",
        device_refuses="decode")
    cache.extend(out)
    return list(out)
