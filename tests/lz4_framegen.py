"""LZ4 frames in pure Python for the tests of the LZ4 manager's frame methods (hipcomp/lz4.hpp): XXH32, a frame
writer and parser, an LZ4 block writer / decoder that knows a history (linked blocks), and a planner of frames --
legal ones of every form the reader takes and hostile ones for every refusal it owes, by name, with truncations at
every structural boundary.  tests/test_lz4_framegen_cpu.py holds all of it to liblz4's LZ4F_decompress."""
import ctypes
import struct
from dataclasses import dataclass, field

MAGIC = 0x184D2204
LEGACY_MAGIC = 0x184C2102
SKIPPABLE = 0x184D2A50
BLOCK_MAX = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
SUCCESS, NOT_SUPPORTED, CANNOT_DECOMPRESS, BAD_CHECKSUM, CANNOT_VERIFY = 0, 11, 12, 13, 14
# csrc/lz4_frame.hpp, enum Reason
REASONS = {"ok": 0, "truncated": 1, "unknown_magic": 2, "legacy_magic": 3, "bad_version": 4, "reserved_bit": 5,
           "block_max_code": 6, "header_checksum": 7, "dict_id": 8, "block_too_large": 9, "missing_end_mark": 10,
           "decoded_too_large": 11, "bad_block": 12, "content_size": 13, "too_many_blocks": 14}
NOT_SUPPORTED_REASONS = ("legacy_magic", "dict_id")
# a frame of 2^32 blocks has 20 GiB at the least: the one refusal no test builds
UNPLANNED_REASONS = ("ok", "too_many_blocks")

P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
M = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def xxh32(data: bytes, seed: int = 0) -> int:
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M]
        while p + 16 <= n:
            for k, w in enumerate(struct.unpack_from("<4I", data, p)):
                v[k] = (_rotl((v[k] + w * P2) & M, 13) * P1) & M
            p += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, p)[0] * P3) & M, 17) * P4) & M
        p += 4
    while p < n:
        h = (_rotl((h + data[p] * P5) & M, 11) * P1) & M
        p += 1
    h ^= h >> 15
    h = (h * P2) & M
    h ^= h >> 13
    h = (h * P3) & M
    h ^= h >> 16
    return h


# ---- LZ4 blocks ------------------------------------------------------------------------------------------------
def _lsic(n):
    out = b""
    while n >= 255:
        out += b"\xff"
        n -= 255
    return out + bytes([n])


def sequence(literals: bytes, offset=None, match_len=None) -> bytes:
    """One sequence; without an offset the block's last one (literals only)."""
    ll = len(literals)
    head = _lsic(ll - 15) if ll >= 15 else b""
    if offset is None:
        return bytes([min(ll, 15) << 4]) + head + literals
    m = match_len - 4
    return (bytes([(min(ll, 15) << 4) | min(m, 15)]) + head + literals + struct.pack("<H", offset)
            + (_lsic(m - 15) if m >= 15 else b""))


def decode_block(block: bytes, history: bytes = b"") -> bytes:
    """The block's bytes; matches may reach into `history`.  ValueError where a decoder must refuse."""
    out = bytearray(history)
    c, end = 0, len(block)

    def code(n):
        nonlocal c
        while True:
            if c >= end:
                raise ValueError("length code runs out of the block")
            b = block[c]
            c += 1
            n += b
            if b != 255:
                return n
    while c < end:
        tok = block[c]
        c += 1
        lit = tok >> 4
        if lit == 15:
            lit = code(lit)
        if lit > end - c:
            raise ValueError("literals run out of the block")
        out += block[c:c + lit]
        c += lit
        if c >= end:
            break
        if end - c < 2:
            raise ValueError("no room for an offset")
        off = block[c] | (block[c + 1] << 8)
        c += 2
        ml = 4 + (tok & 15)
        if (tok & 15) == 15:
            ml = code(ml)
        if off == 0 or off > len(out):
            raise ValueError("match reaches before the first byte")
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out[len(history):])


# ---- frames ----------------------------------------------------------------------------------------------------
def descriptor(code, linked=False, block_sums=False, content_sum=False, content_size=None, dict_id=None,
               version=1, flg_reserved=0, bd_reserved=0, bad_hc=False) -> bytes:
    flg = (version << 6) | (0 if linked else 0x20) | (0x10 if block_sums else 0) | (0x08 if content_size is not None else 0) \
        | (0x04 if content_sum else 0) | (flg_reserved << 1) | (1 if dict_id is not None else 0)
    d = bytes([flg, ((code & 7) << 4) | bd_reserved])
    if content_size is not None:
        d += struct.pack("<Q", content_size)
    if dict_id is not None:
        d += struct.pack("<I", dict_id)
    hc = (xxh32(d) >> 8) & 0xFF
    return struct.pack("<I", MAGIC) + d + bytes([hc ^ (0x5A if bad_hc else 0)])


def data_block(payload: bytes, stored: bool, block_sums: bool) -> bytes:
    b = struct.pack("<I", len(payload) | (0x80000000 if stored else 0)) + payload
    return b + (struct.pack("<I", xxh32(payload)) if block_sums else b"")


def frame(blocks, code=4, linked=False, block_sums=False, content_sum=False, content_size=None, content=b"", **header):
    """blocks: [(payload, stored)]; content: what they decode to (for the content checksum)."""
    out = [descriptor(code, linked, block_sums, content_sum, content_size, **header)]
    out += [data_block(payload, stored, block_sums) for payload, stored in blocks]
    out.append(struct.pack("<I", 0))
    if content_sum:
        out.append(struct.pack("<I", xxh32(content)))
    return b"".join(out)


def skippable(payload: bytes, nibble: int = 0) -> bytes:
    return struct.pack("<II", SKIPPABLE + nibble, len(payload)) + payload


def written_frame(chunks, streams, chunk_bytes, block_sums) -> bytes:
    """The frame compress_frame owes for these chunks and the batched encoder's streams of them."""
    code = min(c for c in BLOCK_MAX if BLOCK_MAX[c] >= chunk_bytes)
    blocks = [(c, True) if len(s) >= len(c) else (s, False) for c, s in zip(chunks, streams)]
    return frame(blocks, code, block_sums=block_sums, content_size=sum(len(c) for c in chunks))


def parse(buf: bytes):
    """[{"linked", "block_sums", "content_sum", "content_size", "code", "blocks": [(payload, stored, sum or None)],
    "content_sum_value"}] of a sound input; skippable frames are stepped over."""
    frames, at = [], 0
    while at < len(buf):
        magic, = struct.unpack_from("<I", buf, at)
        if SKIPPABLE <= magic <= SKIPPABLE + 15:
            at += 8 + struct.unpack_from("<I", buf, at + 4)[0]
            continue
        assert magic == MAGIC, hex(magic)
        flg, bd = buf[at + 4], buf[at + 5]
        f = {"linked": not flg & 0x20, "block_sums": bool(flg & 0x10), "content_sum": bool(flg & 4), "content_size": None,
             "code": bd >> 4, "blocks": [], "content_sum_value": None}
        p = at + 6
        if flg & 8:
            f["content_size"], = struct.unpack_from("<Q", buf, p)
            p += 8
        assert buf[p] == (xxh32(buf[at + 4:p]) >> 8) & 0xFF
        p += 1
        while True:
            word, = struct.unpack_from("<I", buf, p)
            p += 4
            if word & 0x7FFFFFFF == 0:
                break
            n = word & 0x7FFFFFFF
            payload = buf[p:p + n]
            p += n
            s = None
            if f["block_sums"]:
                s, = struct.unpack_from("<I", buf, p)
                p += 4
            f["blocks"].append((payload, bool(word >> 31), s))
        if f["content_sum"]:
            f["content_sum_value"], = struct.unpack_from("<I", buf, p)
            p += 4
        frames.append(f)
        at = p
    return frames


def decode(buf: bytes, block_decoder=None) -> bytes:
    """The content of a sound input.  block_decoder(payload, capacity) -> bytes decodes the blocks of
    independent-block frames (the tests pass the oracle's); linked frames and the default use decode_block."""
    out = bytearray()
    for f in parse(buf):
        content = bytearray()
        for payload, stored, s in f["blocks"]:
            if s is not None:
                assert s == xxh32(payload)
            if stored:
                content += payload
            elif f["linked"] or block_decoder is None:
                content += decode_block(payload, bytes(content) if f["linked"] else b"")
            else:
                content += block_decoder(payload, BLOCK_MAX[f["code"]])
        if f["content_size"] is not None:
            assert f["content_size"] == len(content)
        if f["content_sum_value"] is not None:
            assert f["content_sum_value"] == xxh32(bytes(content))
        out += content
    return bytes(out)


# ---- the planner -----------------------------------------------------------------------------------------------
@dataclass
class Plan:
    name: str
    data: bytes
    content: bytes = b""            # legal plans: what the input decodes to
    reason: str = "ok"              # why the reader refuses it (REASONS)
    blocks: int = 0                 # legal plans: data blocks
    flipped: str = ""               # "block" / "content": a checksum that does not fit -- BadChecksum if verified
    bare: bool = False              # a frame carries no checksum at all
    truncated_at: str = ""          # the structural boundary a truncation cuts at
    liblz4_differs: str = ""        # why LZ4F_decompress's verdict is another one (the documented differences)
    notes: list = field(default_factory=list)

    @property
    def liblz4_accepts(self) -> bool:
        """LZ4F_decompress takes the input whole and without an error."""
        return (self.reason == "ok" and not self.flipped) or self.name == "dict_id"

    def status(self, policy: int) -> int:
        """hipcompStatus_t decompress_frame owes under the ChecksumPolicy."""
        verifies = policy in (2, 3, 4)
        if self.flipped and verifies:
            return BAD_CHECKSUM
        if self.reason != "ok":
            return NOT_SUPPORTED if self.reason in NOT_SUPPORTED_REASONS else CANNOT_DECOMPRESS
        if policy == 4 and self.bare:
            return CANNOT_VERIFY
        return SUCCESS


def _text(n, salt=0):
    words = [b"frame", b"block", b"lz4", b"wave", b"lane", b"offset", b"token", b"literal", b"match", b"chain"]
    out, k = bytearray(), salt
    while len(out) < n:
        k = (k * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[k % len(words)] + b" "
    return bytes(out[:n])


def _pieces():
    """Blocks made by hand and what they decode to."""
    a = _text(300, 1)
    # block 1: literals, a match inside itself, the last literals
    b1 = sequence(a[:40], 40, 20) + sequence(a[60:72])
    c1 = decode_block(b1)
    return a, b1, c1


def legal_plans():
    a, b1, c1 = _pieces()
    plans = []

    def add(name, data, content, blocks, bare, **kw):
        plans.append(Plan(name, data, content=content, blocks=blocks, bare=bare, **kw))
    add("no_bytes", b"", b"", 0, False)
    add("only_skippable", skippable(b"xyz", 3), b"", 0, False)
    for sums in (False, True):
        add("empty_frame" + ("_content_sum" if sums else ""), frame([], content_sum=sums, content_size=0), b"", 0, not sums)
    for code in (4, 5, 6, 7):
        add("code_%d" % code, frame([(b1, False)], code), c1, 1, True)
    raw = bytes(range(256)) * 2
    # independent blocks: compressed, stored, a short one in the middle, every header option
    for bs in (False, True):
        for cs in (False, True):
            for size in (False, True):
                content = c1 + raw + c1
                add("independent%s%s%s" % ("_bsum" if bs else "", "_csum" if cs else "", "_size" if size else ""),
                    frame([(b1, False), (raw, True), (b1, False)], 4, False, bs, cs, len(content) if size else None, content),
                    content, 3, not (bs or cs))
    # linked blocks: block 2 reaches into block 1 (to the frame's very first byte), block 3 is stored, block 4
    # reaches through block 3 into block 2 and into the stored block alone
    b2 = sequence(b"", len(c1), 30) + sequence(b"-tail")
    c2 = decode_block(b2, c1)
    st = _text(90, 7)
    b4 = sequence(b"xy", 2 + len(st) + 10, 24) + sequence(b"z", 50, 40) + sequence(b"final")
    c4 = decode_block(b4, c1 + c2 + st)
    content = c1 + c2 + st + c4
    for bs, cs, size in ((False, False, False), (True, True, True), (False, True, False)):
        add("linked%s%s%s" % ("_bsum" if bs else "", "_csum" if cs else "", "_size" if size else ""),
            frame([(b1, False), (b2, False), (st, True), (b4, False)], 4, True, bs, cs, len(content) if size else None, content),
            content, 4, not (bs or cs))
    # an overlapping match across the block boundary: period 3 out of the previous block's tail
    b5 = sequence(b"", 3, 200) + sequence(b"endend")
    add("linked_overlap", frame([(b1, False), (b5, False)], 5, True), c1 + decode_block(b5, c1), 2, True)
    # long runs: literal and match lengths beyond a wave's 64 lanes, with length codes of several bytes
    lits = _text(700, 3)
    b6 = sequence(lits, 700, 600) + sequence(b"", 1300, 1299) + sequence(b"#####")
    c6 = decode_block(b6)
    add("linked_long_runs", frame([(b6, False), (sequence(b"", len(c6), 300) + sequence(b"12345"), False)], 4, True, True, True,
                                  None, c6 + c6[:300] + b"12345"), c6 + c6[:300] + b"12345", 2, False)
    # frames back to back, skippable ones before, between and behind; the second is linked and stands on its own
    f1 = frame([(b1, False)], 4, content_size=len(c1))
    f2 = frame([(b1, False), (b2, False)], 6, True, content_size=len(c1 + c2))
    add("two_frames_skippable", skippable(b"", 0) + f1 + skippable(b"between", 15) + f2 + skippable(b"!" * 40, 1),
        c1 + c1 + c2, 3, True)
    add("frame_then_empty_frame", f1 + frame([], 4, content_sum=True), c1, 1, True)
    return plans


def hostile_plans():
    a, b1, c1 = _pieces()
    good = frame([(b1, False)], 4, content_size=len(c1))
    plans = []

    def add(name, data, reason, **kw):
        plans.append(Plan(name, data, reason=reason, **kw))
    add("unknown_magic", b"\x05\x22\x4d\x18" + good[4:], "unknown_magic")
    add("unknown_magic_behind_a_frame", good + b"LZ4!" + good[4:], "unknown_magic")
    add("legacy_magic", struct.pack("<I", LEGACY_MAGIC) + struct.pack("<I", len(b1)) + b1, "legacy_magic",
        liblz4_differs="refused by both; here as hipcompErrorNotSupported")
    add("dict_id", frame([(b1, False)], 4, dict_id=0x1234), "dict_id",
        liblz4_differs="LZ4F_decompress decodes a frame with a dictionary id that uses none of it")
    for v in (0, 2, 3):
        add("version_%d" % v, frame([(b1, False)], 4, version=v), "bad_version")
    add("reserved_flg", frame([(b1, False)], 4, flg_reserved=1), "reserved_bit")
    add("reserved_bd_high", frame([(b1, False)], 4, bd_reserved=0x80), "reserved_bit")
    add("reserved_bd_low", frame([(b1, False)], 4, bd_reserved=0x01), "reserved_bit")
    for code in (0, 3):
        add("block_max_code_%d" % code, frame([(b1, False)], code), "block_max_code")
    add("header_checksum", frame([(b1, False)], 4, bad_hc=True), "header_checksum")
    # a size word above the block maximum (the bytes are there)
    big = bytes(65537)
    add("block_too_large", frame([(big, True)], 4), "block_too_large")
    add("block_size_runs_out", good[:15] + struct.pack("<I", 5000) + good[19:], "truncated")
    add("missing_end_mark", good[:-4], "missing_end_mark")
    add("end_mark_cut", good[:-2], "missing_end_mark")
    # a block that decodes to one byte more than the block maximum
    fat = sequence(b"a", 1, 65530) + sequence(b"bbbbbb")
    assert len(decode_block(fat)) == 65537
    add("decoded_too_large", frame([(fat, False)], 4), "decoded_too_large")
    add("decoded_too_large_linked", frame([(b1, False), (fat, False)], 4, True), "decoded_too_large")
    # a match that reaches one byte before the frame's first byte: in the first frame (before the output buffer), and
    # in a second one (into the first frame's output, which is no history of its)
    early = sequence(b"abcdefgh", 9, 8) + sequence(b"tail!")
    add("match_before_frame_independent", frame([(early, False)], 4), "bad_block")
    add("match_before_frame_linked", frame([(early, False)], 4, True), "bad_block")
    b2 = sequence(b"", len(c1) + 1, 30) + sequence(b"-tail")
    add("match_before_frame_second_block", frame([(b1, False), (b2, False)], 4, True), "bad_block")
    add("match_into_the_frame_before", good + frame([(early, False)], 4, True), "bad_block")
    add("independent_block_reaches_back", frame([(b1, False), (sequence(b"", 10, 30) + sequence(b"-tail"), False)], 4), "bad_block")
    add("block_cut_inside_linked", frame([(b1, False), (b1[:-3], False)], 4, True), "bad_block",
        notes=["the last literals run out of the block"])
    for delta in (-1, 1):
        add("content_size_%+d" % delta, frame([(b1, False)], 4, content_size=len(c1) + delta), "content_size")
    add("content_size_linked", frame([(b1, False), (b1, True)], 4, True, content_size=len(c1)), "content_size")
    add("content_size_empty_frame", frame([], 4, content_size=1), "content_size")
    # checksums that do not fit: refused where they are verified
    sums = frame([(b1, False), (a[:100], True)], 4, False, True, True, None, c1 + a[:100])
    at = 7 + 4 + len(b1)
    add("flipped_block_checksum", sums[:at] + bytes([sums[at] ^ 1]) + sums[at + 1:], "ok", content=c1 + a[:100], blocks=2,
        flipped="block", liblz4_differs="LZ4F_decompress always verifies what is present")
    add("flipped_content_checksum", sums[:-1] + bytes([sums[-1] ^ 0x80]), "ok", content=c1 + a[:100], blocks=2,
        flipped="content", liblz4_differs="LZ4F_decompress always verifies what is present")
    lsum = frame([(b1, False), (sequence(b"", len(c1), 30) + sequence(b"-tail"), False)], 4, True, False, True, None, b"wrong")
    add("flipped_content_checksum_linked", lsum, "ok", content=c1 + decode_block(sequence(b"", len(c1), 30) + sequence(b"-tail"), c1),
        blocks=2, flipped="content", liblz4_differs="LZ4F_decompress always verifies what is present")
    add("flipped_content_checksum_empty_frame", frame([], 4, content_sum=True)[:-1] + b"\x00", "ok", flipped="content",
        liblz4_differs="LZ4F_decompress always verifies what is present")
    return plans


TRUNCATION_POINTS = ("after_magic", "after_flg", "after_bd", "inside_content_size", "before_hc", "inside_size_word",
                     "inside_block", "before_block_checksum", "before_end_mark", "before_content_checksum")


def truncation_plans():
    """One frame with everything in it, cut at every structural boundary."""
    a, b1, c1 = _pieces()
    content = c1 + a[:64]
    whole = frame([(b1, False), (a[:64], True)], 4, False, True, True, len(content), content)
    first = 15 + 4 + len(b1)          # where the first block's checksum stands
    second = first + 4 + 4 + 64       # the second's
    cuts = {"after_magic": 4, "after_flg": 5, "after_bd": 6, "inside_content_size": 10, "before_hc": 14,
            "inside_size_word": 17, "inside_block": 15 + 4 + 7, "before_block_checksum": first,
            "before_end_mark": second + 4, "before_content_checksum": second + 8}
    assert second + 12 == len(whole) and tuple(cuts) == TRUNCATION_POINTS
    plans = [Plan("whole", whole, content=content, blocks=2)]
    for name, cut in cuts.items():
        reason = "missing_end_mark" if name in ("before_end_mark", "inside_size_word") else "truncated"
        plans.append(Plan("cut_" + name, whole[:cut], reason=reason, truncated_at=name))
    return plans


def all_plans():
    return legal_plans() + hostile_plans() + truncation_plans()


# ---- liblz4's frame decoder ------------------------------------------------------------------------------------
def load_lz4f():
    """The system liblz4 (ctypes) with its frame API, or None."""
    try:
        L = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    L.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    L.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    L.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p,
                                  ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    L.LZ4F_decompress.restype = ctypes.c_size_t
    L.LZ4F_isError.argtypes = [ctypes.c_size_t]
    L.LZ4F_isError.restype = ctypes.c_uint
    L.LZ4_versionNumber.restype = ctypes.c_int
    return L


def lz4f_decompress(L, buf: bytes):
    """(accepted, content): every frame of buf through LZ4F_decompress; accepted: no error, all input consumed,
    the last frame complete."""
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    out, at, hint = bytearray(), 0, 0
    src = ctypes.create_string_buffer(buf, len(buf)) if buf else ctypes.create_string_buffer(1)
    dst = ctypes.create_string_buffer(1 << 16)
    try:
        while at < len(buf):
            n_src, n_dst = ctypes.c_size_t(len(buf) - at), ctypes.c_size_t(len(dst))
            hint = L.LZ4F_decompress(ctx, dst, ctypes.byref(n_dst), ctypes.byref(src, at), ctypes.byref(n_src), None)
            if L.LZ4F_isError(hint):
                return False, bytes(out)
            out += dst.raw[:n_dst.value]
            at += n_src.value
            if n_src.value == 0 and n_dst.value == 0:
                break
        return hint == 0 and at == len(buf), bytes(out)
    finally:
        L.LZ4F_freeDecompressionContext(ctx)
