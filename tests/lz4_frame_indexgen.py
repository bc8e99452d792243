"""The block index of a seekable LZ4 frame (csrc/lz4_frame_index.hpp; INTEGRATION.md, "Seekable LZ4 frames") in pure
Python for the tests of the LZ4 manager's indexed frame methods: a writer and a parser of the index that give the
header's reason codes, and a list of planned indexed inputs, each with the reason its index should or should not
apply.  Every planned input is a sound or unsound .lz4 file in its own right: a reader that knows nothing of the
index skips it as a skippable frame.  tests/test_lz4_frame_index_cpu.py holds all of it to the header and to liblz4."""
import ctypes
import struct
from dataclasses import dataclass

import lz4_framegen as G

INDEX_MAGIC = 0x184D2A54
SIGNATURE = b"HCLZ4IDX"
MAX_BLOCK_BYTES = 4 << 20
STORED = 0x80000000
# csrc/lz4_frame_index.hpp, enum IndexReason
REASONS = {"ok": 0, "not_there": 1, "payload_size": 2, "signature": 3, "version": 4, "flags": 5, "block_bytes": 6,
           "count": 7, "hash": 8, "no_frame": 9, "frame_form": 10, "content_size": 11, "block_sums": 12, "block_max": 13,
           "offset": 14, "word": 15, "length": 16, "stored_length": 17, "end_mark": 18, "decode": 19, "too_many_frames": 20}
# only the device meets these: the decode of a block, the size of the reader's frame table
DEVICE_REASONS = ("decode", "too_many_frames")


def index_bytes(n):
    return 44 + 4 * n


def index_frame(words, block_bytes, content_bytes, block_sums, *, magic=INDEX_MAGIC, signature=SIGNATURE, version=1,
                flags=None, n=None, payload=None, bad_hash=False, pad=b"") -> bytes:
    """The index of a frame with these size words; the keywords forge single fields (the hash fits them unless
    bad_hash), pad: bytes behind the hash that the payload size counts."""
    n = len(words) if n is None else n
    flags = (1 if block_sums else 0) if flags is None else flags
    body = signature + struct.pack("<IIIIQ", version, flags, block_bytes, n, content_bytes) + struct.pack("<%dI" % len(words), *words)
    h = G.xxh32(body) ^ (0x10 if bad_hash else 0)
    body += struct.pack("<I", h) + pad
    return struct.pack("<II", magic, len(body) if payload is None else payload) + body


def size_words(frame: bytes):
    """The size words of the data blocks of one frame (a sound one), as they stand in it."""
    f, = G.parse(frame)
    return [len(p) | (STORED if stored else 0) for p, stored, _ in f["blocks"]]


def parse_index(buf: bytes, at: int):
    """csrc/lz4_frame_index.hpp, parse_index_fields and index_hash_fits, said again: (reason, head)"""
    avail = len(buf) - at
    if avail < 8 or struct.unpack_from("<I", buf, at)[0] != INDEX_MAGIC:
        return "not_there", None
    payload, = struct.unpack_from("<I", buf, at + 4)
    if payload < 36 or payload > avail - 8:
        return "payload_size", None
    if buf[at + 8:at + 16] != SIGNATURE:
        return "signature", None
    version, flags, block_bytes, n, content = struct.unpack_from("<IIIIQ", buf, at + 16)
    if version != 1:
        return "version", None
    if flags & ~1:
        return "flags", None
    if block_bytes == 0 or block_bytes > MAX_BLOCK_BYTES:
        return "block_bytes", None
    if payload != 36 + 4 * n:
        return "payload_size", None
    if -(-content // block_bytes) != n:
        return "count", None
    if G.xxh32(buf[at + 8:at + 40 + 4 * n]) != struct.unpack_from("<I", buf, at + 40 + 4 * n)[0]:
        return "hash", None
    return "ok", {"flags": flags, "block_bytes": block_bytes, "blocks": n, "content_bytes": content,
                  "words": list(struct.unpack_from("<%dI" % n, buf, at + 40))}


def _descriptor(buf: bytes, at: int):
    """What the reader's descriptor parse makes of buf[at:]: None where it refuses, else (header bytes, flg, bd)"""
    p = buf[at:]
    if len(p) < 7 or struct.unpack_from("<I", p)[0] != G.MAGIC:
        return None
    flg, bd = p[4], p[5]
    n = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    if flg & 2 or flg >> 6 != 1 or len(p) < n or bd & 0x8F or (bd >> 4) < 4 or flg & 1:
        return None
    if p[n - 1] != (G.xxh32(p[4:n - 1]) >> 8) & 0xFF:
        return None
    return n, flg, bd


def index_applies(buf: bytes, at: int):
    """index_applies of the header: (reason, the byte behind the EndMark, head)"""
    reason, h = parse_index(buf, at)
    if reason != "ok":
        return reason, None, None
    frame_at = at + index_bytes(h["blocks"])
    d = _descriptor(buf, frame_at)
    if d is None:
        return "no_frame", None, h
    header, flg, bd = d
    if not flg & 0x20 or flg & 4 or not flg & 8:
        return "frame_form", None, h
    if struct.unpack_from("<Q", buf, frame_at + 6)[0] != h["content_bytes"]:
        return "content_size", None, h
    if bool(flg & 0x10) != bool(h["flags"] & 1):
        return "block_sums", None, h
    if h["block_bytes"] > G.BLOCK_MAX[bd >> 4]:
        return "block_max", None, h
    pos, n = frame_at + header, h["blocks"]
    for i, word in enumerate(h["words"]):
        if len(buf) - pos < 4:
            return "offset", None, h
        if struct.unpack_from("<I", buf, pos)[0] != word:
            return "word", None, h
        size = word & ~STORED
        if size < 1 or size > h["block_bytes"]:
            return "length", None, h
        content = h["block_bytes"] if i + 1 < n else h["content_bytes"] - h["block_bytes"] * i
        if word & STORED and size != content:
            return "stored_length", None, h
        pos += 4 + size + (4 if h["flags"] & 1 else 0)
    if len(buf) - pos < 4:
        return "offset", None, h
    if struct.unpack_from("<I", buf, pos)[0] & ~STORED:
        return "end_mark", None, h
    return "ok", pos + 4, h


def input_is_indexed(buf: bytes):
    """input_is_indexed of the header: (reason, frames, blocks, content bytes)"""
    pos, frames, blocks, content = 0, 0, 0, 0
    while pos < len(buf):
        if len(buf) - pos >= 8:
            magic, size = struct.unpack_from("<II", buf, pos)
            if G.SKIPPABLE <= magic <= G.SKIPPABLE + 15 and magic != INDEX_MAGIC:
                if size > len(buf) - pos - 8:
                    return "not_there", frames, blocks, content
                pos += 8 + size
                continue
        reason, end, h = index_applies(buf, pos)
        if reason != "ok":
            return reason, frames, blocks, content
        frames, blocks, content, pos = frames + 1, blocks + h["blocks"], content + h["content_bytes"], end
    return "ok", frames, blocks, content


def strip_indexes(buf: bytes) -> bytes:
    """The input without its skippable frames of the index's magic (sound or not); the rest as it stands."""
    out, pos = bytearray(), 0
    while pos < len(buf):
        if len(buf) - pos >= 8:
            magic, size = struct.unpack_from("<II", buf, pos)
            if magic == INDEX_MAGIC and size <= len(buf) - pos - 8:
                pos += 8 + size
                continue
            if G.SKIPPABLE <= magic <= G.SKIPPABLE + 15 and size <= len(buf) - pos - 8:
                out += buf[pos:pos + 8 + size]
                pos += 8 + size
                continue
        # a frame (or what cannot be read): a sound frame is stepped over whole, anything else ends the stripping
        try:
            end = _frame_end(buf, pos)
        except (ValueError, struct.error):
            out += buf[pos:]
            break
        out += buf[pos:end]
        pos = end
    return bytes(out)


def _frame_end(buf, at):
    d = _descriptor(buf, at)
    if d is None:
        raise ValueError("no frame")
    header, flg, _ = d
    pos = at + header
    while True:
        word, = struct.unpack_from("<I", buf, pos)
        pos += 4
        if word & ~STORED == 0:
            break
        pos += (word & ~STORED) + (4 if flg & 0x10 else 0)
        if pos > len(buf):
            raise ValueError("cut")
    return pos + (4 if flg & 4 else 0)


# ---- frames of the form compress_frame writes ---------------------------------------------------------------------
def compressed_block(size, salt):
    """An LZ4 block that decodes to exactly `size` (>= 33) bytes and is shorter than they are."""
    lits = G._text(24, salt)
    return G.sequence(lits, 24, size - 29) + G.sequence(b"<end>")


def written_form(block_bytes, kinds, last, sums, salt=0, code=None):
    """(frame, content): independent blocks, C.Size, one block per block_bytes of content -- kinds: "c" compressed /
    "s" stored per block, the last one holding `last` bytes."""
    blocks, content = [], bytearray()
    for i, kind in enumerate(kinds):
        size = block_bytes if i + 1 < len(kinds) else last
        if kind == "c":
            b = compressed_block(size, salt + i)
            blocks.append((b, False))
            content += G.decode_block(b)
        else:
            raw = bytes((salt * 7 + i * 31 + k * k) & 0xFF for k in range(size))
            blocks.append((raw, True))
            content += raw
    if code is None:
        code = min(c for c in G.BLOCK_MAX if G.BLOCK_MAX[c] >= block_bytes)
    return G.frame(blocks, code, block_sums=sums, content_size=len(content)), bytes(content)


def indexed(frame: bytes, block_bytes, sums, **forge) -> bytes:
    """The frame behind its index."""
    f, = G.parse(frame)
    return index_frame(size_words(frame), block_bytes, f["content_size"], sums, **forge) + frame


def liblz4_short_interior_frame(parts):
    """A frame LZ4F_compressUpdate / LZ4F_flush make of `parts`, one block each (independent blocks, C.Size, 64 KiB
    block maximum): blocks in the middle of the frame hold fewer bytes than the first.  None without liblz4."""
    L = G.load_lz4f()
    if L is None:
        return None

    class FrameInfo(ctypes.Structure):
        _fields_ = [("blockSizeID", ctypes.c_uint), ("blockMode", ctypes.c_uint), ("contentChecksumFlag", ctypes.c_uint),
                    ("frameType", ctypes.c_uint), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                    ("blockChecksumFlag", ctypes.c_uint)]

    class Preferences(ctypes.Structure):
        _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                    ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]
    prefs = Preferences()
    prefs.frameInfo.blockSizeID = 4
    prefs.frameInfo.blockMode = 1     # independent
    prefs.frameInfo.contentSize = sum(map(len, parts))
    for name in ("LZ4F_createCompressionContext", "LZ4F_compressBegin", "LZ4F_compressUpdate", "LZ4F_flush",
                 "LZ4F_compressEnd", "LZ4F_compressBound", "LZ4F_freeCompressionContext"):
        getattr(L, name).restype = ctypes.c_size_t
    L.LZ4F_createCompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.LZ4F_compressBegin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_compressUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_flush.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_compressEnd.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_compressBound.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_freeCompressionContext.argtypes = [ctypes.c_void_p]
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(ctx), 100))
    cap = 64 + L.LZ4F_compressBound(max(map(len, parts)), ctypes.byref(prefs))
    dst, out = ctypes.create_string_buffer(cap), bytearray()
    try:
        def take(n):
            assert not L.LZ4F_isError(n), n
            out.extend(dst.raw[:n])
        take(L.LZ4F_compressBegin(ctx, dst, cap, ctypes.byref(prefs)))
        for part in parts:
            take(L.LZ4F_compressUpdate(ctx, dst, cap, part, len(part), None))
            take(L.LZ4F_flush(ctx, dst, cap, None))
        take(L.LZ4F_compressEnd(ctx, dst, cap, None))
    finally:
        L.LZ4F_freeCompressionContext(ctx)
    return bytes(out)


# ---- the planner -----------------------------------------------------------------------------------------------
@dataclass
class IndexPlan:
    name: str
    data: bytes                # the input with its index frames
    reason: str                # input_is_indexed's word on it (REASONS): "ok" -- every index applies by the host's tests
    why: str                   # what was done to it
    content: bytes = b""       # what a sound input decodes to
    blocks: int = 0            # its data blocks
    sound: bool = True         # LZ4F_decompress takes the input whole (with and without its index frames)
    device_refuses: bool = False  # the host's tests pass, the decode of a block does not give its content bytes

    @property
    def bare(self) -> bytes:
        return strip_indexes(self.data)

    @property
    def applies(self) -> bool:
        """The indexed read takes it: no block is listed by the walk."""
        return self.reason == "ok" and not self.device_refuses

    def status(self, policy: int) -> int:
        """hipcompStatus_t decompress_frame owes under the ChecksumPolicy, from liblz4's verdict on the input."""
        if not self.sound:
            return G.CANNOT_DECOMPRESS
        if policy == 4 and any(not f["block_sums"] and not f["content_sum"] for f in G.parse(self.bare)):
            return G.CANNOT_VERIFY   # a frame that carries no checksum at all
        return G.SUCCESS


BB = 256            # content bytes per block of the planned frames
KINDS = "cscscsc"   # seven blocks: compressed, stored, compressed, ...
LAST = 100


def plans():
    out = []
    frame, content = written_form(BB, KINDS, LAST, False, 1)
    frame_s, content_s = written_form(BB, KINDS, LAST, True, 2)
    words = size_words(frame)
    n = len(words)

    def add(name, data, reason, why, content=content, blocks=n, **kw):
        out.append(IndexPlan(name, data, reason, why, content=content, blocks=blocks, **kw))

    def forged(**kw):
        return indexed(frame, BB, False, **kw)
    add("good", forged(), "ok", "a sound index")
    add("good_block_sums", indexed(frame_s, BB, True), "ok", "a sound index of a frame with block checksums", content=content_s)
    empty = G.frame([], 4, content_size=0)
    add("good_empty", index_frame([], BB, 0, False) + empty, "ok", "N = 0: the index, the header, the EndMark", content=b"", blocks=0)
    one, one_content = written_form(BB, "c", BB, False, 3)
    add("good_one_full_block", indexed(one, BB, False), "ok", "one block of exactly block_bytes", content=one_content, blocks=1)
    add("wrong_hash", forged(bad_hash=True), "hash", "one bit of the hash flipped")
    add("wrong_signature", forged(signature=b"HCLZ4IDY"), "signature", "the last letter of the signature")
    add("wrong_magic_nibble", forged(magic=G.SKIPPABLE + 0xE), "not_there", "the skippable magic of another format: no index, no walk spared")
    add("wrong_version", forged(version=2), "version", "version 2")
    add("reserved_flag", forged(flags=2), "flags", "flag bit 1")
    add("payload_disagrees", forged(payload=36 + 4 * n + 4, pad=b"\0\0\0\0"), "payload_size", "four bytes more payload than 36 + 4N")
    add("n_too_large", index_frame(words + [words[-1]], BB, len(content), False) + frame, "count", "N + 1 words")
    add("n_too_small", index_frame(words[:-1], BB, len(content), False) + frame, "count", "N - 1 words")
    add("n_beyond_buffer", forged(n=0x3FFFFFFF), "payload_size", "N of 2^30 - 1: 4N bytes are not there (the payload size is the true one)")
    add("block_bytes_zero", index_frame(words, 0, len(content), False) + frame, "block_bytes", "block_bytes 0")
    add("block_bytes_above_4m", index_frame(words, MAX_BLOCK_BYTES + 1, len(content), False) + frame, "block_bytes", "block_bytes 4 MiB + 1")
    add("block_bytes_above_block_max", index_frame(size_words(one), 65537, BB, False) + one, "block_max",
        "block_bytes 65537 in front of a frame of 64 KiB blocks (N = 1 fits it)", content=one_content, blocks=1)
    add("content_size_differs", index_frame(words, BB, len(content) + 1, False) + frame, "content_size", "content_bytes = C.Size + 1 (N stays)")
    add("block_sums_flag_differs", forged(flags=1), "block_sums", "flag bit 0 in front of a frame without B.Checksum")
    add("block_sums_flag_missing", indexed(frame_s, BB, True, flags=0), "block_sums", "no flag bit 0 in front of a frame with B.Checksum",
        content=content_s)
    changed = list(words)
    changed[3] += 1
    add("size_word_changed", index_frame(changed, BB, len(content), False) + frame, "word", "word 3 one more")
    flipped = list(words)
    flipped[2] ^= STORED
    add("stored_bit_changed", index_frame(flipped, BB, len(content), False) + frame, "word", "bit 31 of word 2")
    # a foreign frame whose stored block in the middle is short: the words are the frame's own
    c0, c2 = compressed_block(BB, 10), compressed_block(BB, 12)
    short, tail = bytes(range(90)), bytes(range(200))
    fc = G.decode_block(c0) + short + G.decode_block(c2) + tail
    assert -(-len(fc) // BB) == 4
    foreign = G.frame([(c0, False), (short, True), (c2, False), (tail, True)], 4, content_size=len(fc))
    add("stored_block_short", indexed(foreign, BB, False), "stored_length", "a stored block of 90 bytes where 256 are due",
        content=fc, blocks=4)
    # a block of literals alone is longer than what it holds
    lit = G.sequence(G._text(33, 15))
    longer = G.frame([(lit, False)], 4, content_size=33)
    add("length_above_block_bytes", indexed(longer, 33, False), "length", "a block of 35 bytes for 33 bytes of content",
        content=G.decode_block(lit), blocks=1)
    cut = indexed(frame, BB, False)
    cut = cut[:len(cut) - 4 - (words[-1] & ~STORED) - 4 - 20]
    add("lengths_beyond_the_buffer", cut, "offset", "the input ends inside block N - 2: the scan leaves it", sound=False)
    # three blocks listed, a fourth stands where the EndMark is due
    c3 = compressed_block(50, 13)
    c4 = compressed_block(50, 14)
    more_content = G.decode_block(c0) + G.decode_block(c2) + G.decode_block(c3) + G.decode_block(c4)
    more = G.frame([(c0, False), (c2, False), (c3, False), (c4, False)], 4, content_size=len(more_content))
    assert -(-len(more_content) // BB) == 3
    add("no_end_mark", index_frame(size_words(more)[:3], BB, len(more_content), False) + more, "end_mark",
        "a frame of four blocks, short ones at its end, behind an index of three", content=more_content, blocks=4)
    add("index_then_skippable", index_frame(words, BB, len(content), False) + G.skippable(b"between", 2) + frame, "no_frame",
        "a skippable frame between the index and its frame")
    add("index_then_end", index_frame(words, BB, len(content), False), "no_frame", "nothing behind the index", content=b"", blocks=0)
    b1 = compressed_block(BB, 20)
    b2 = G.sequence(b"", BB, 40) + G.sequence(G._text(60, 21))
    lc = G.decode_block(b1) + G.decode_block(b2, G.decode_block(b1))
    linked = G.frame([(b1, False), (b2, False)], 4, True, content_size=len(lc))
    add("linked_frame", index_frame(size_words(linked), BB, len(lc), False) + linked, "frame_form", "a linked frame",
        content=lc, blocks=2)
    with_sum = G.frame(G_blocks(frame), 4, content_sum=True, content_size=len(content), content=content)
    add("content_checksum", index_frame(words, BB, len(content), False) + with_sum, "frame_form", "a frame with C.Checksum")
    # short blocks in the middle behind words that are right: only the decode can tell
    parts = [G._text(1000, 31), G._text(500, 32), G._text(1000, 33)]
    made = liblz4_short_interior_frame(parts)
    if made is None:   # (without liblz4: the same form by hand)
        hb = [compressed_block(1000, 31), compressed_block(500, 32), compressed_block(1000, 33)]
        parts = [G.decode_block(b) for b in hb]
        made = G.frame([(b, False) for b in hb], 4, content_size=2500)
    assert all(not w & STORED for w in size_words(made)) and len(size_words(made)) == 3
    add("short_interior_blocks", indexed(made, 1000, False), "ok", "blocks of 1000, 500, 1000 bytes behind an index of block_bytes 1000",
        content=b"".join(parts), blocks=3, device_refuses=True)
    second, second_content = written_form(BB, "scc", 33, False, 40)
    add("two_frames", indexed(frame, BB, False) + G.skippable(b"a foreign frame", 7) + indexed(second, BB, False), "ok",
        "two indexed frames, a skippable frame of another magic between them", content=content + second_content, blocks=n + 3)
    return out


def G_blocks(frame: bytes):
    f, = G.parse(frame)
    return [(p, stored) for p, stored, _ in f["blocks"]]
