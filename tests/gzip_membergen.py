"""gzip members (RFC 1952), zlib streams (RFC 1950) and BGZF blocks built by hand around a Deflate stream, for
tests/test_gzip_frame_cpu.py and tests/test_gzip_gpu.py: every legal header form, the damaged ones, and zlib as the
arbiter.  Plain Python, no GPU needed to import."""
import struct
import zlib

GZIP, ZLIB, BGZF = 0, 1, 2
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
WBITS = {GZIP: 31, ZLIB: 15, BGZF: 31}
HEADER = {GZIP: 10, ZLIB: 2, BGZF: 18}
TRAILER = {GZIP: 8, ZLIB: 4, BGZF: 8}
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def raw_deflate(data: bytes, level=6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def gzip_header(flg=0, xlen=0, name=b"name.txt", comment=b"a comment", mtime=0x5F3759DF, xfl=2, os_=3, cm=8,
                hcrc_xor=0, name_nul=True) -> bytes:
    h = bytes([0x1F, 0x8B, cm, flg]) + struct.pack("<IBB", mtime, xfl, os_)
    if flg & FEXTRA:
        h += struct.pack("<H", xlen) + bytes((7 * k + 1) & 0xFF for k in range(xlen))
    if flg & FNAME:
        h += name + (b"\0" if name_nul else b"")
    if flg & FCOMMENT:
        h += comment + b"\0"
    if flg & FHCRC:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ hcrc_xor)
    return h


def gzip_trailer(data: bytes) -> bytes:
    return struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def gzip_member(data: bytes, level=6, stream=None, **header) -> bytes:
    return gzip_header(**header) + (raw_deflate(data, level) if stream is None else stream) + gzip_trailer(data)


def zlib_header(cinfo=7, flevel=2, fdict=0, fcheck_xor=0, cm=8) -> bytes:
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (fdict << 5)
    flg |= (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg ^ fcheck_xor])


def zlib_member(data: bytes, level=6, stream=None, **header) -> bytes:
    return (zlib_header(**header) + (raw_deflate(data, level) if stream is None else stream)
            + struct.pack(">I", zlib.adler32(data)))


def bgzf_block(data: bytes, level=6) -> bytes:
    stream = raw_deflate(data, level)
    total = 18 + len(stream) + 8
    return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", total - 1) + stream
            + gzip_trailer(data))


def wrap(wrapper: int, data: bytes, stream: bytes) -> bytes:
    """the plain member of `wrapper` around a given raw stream of `data`"""
    if wrapper == ZLIB:
        return zlib_member(data, stream=stream)
    if wrapper == BGZF:
        return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", 18 + len(stream) + 8 - 1)
                + stream + gzip_trailer(data))
    return gzip_member(data, stream=stream)


def legal_gzip_headers():
    """[(name, header keyword arguments)]: all 32 combinations of the five flags, FEXTRA with XLEN 0, 1 and 300"""
    out = []
    for flg in range(32):
        for xlen in ((0, 1, 300) if flg & FEXTRA else (0,)):
            out.append((f"flg{flg:02x}_xlen{xlen}", dict(flg=flg, xlen=xlen)))
    return out


def arbiter(member: bytes, wrapper: int):
    """-> the chunk if zlib takes `member` as exactly one whole member (eof, nothing unused), else None"""
    d = zlib.decompressobj(WBITS[wrapper])
    try:
        got = d.decompress(member)
    except zlib.error:
        return None
    return got if d.eof and d.unused_data == b"" else None


def stream_without_zero_byte():
    """(data, raw stream) whose stream holds no zero byte: behind an FNAME without its NUL no NUL follows"""
    for k in range(1, 4000):
        data = bytes((k * 31 + 7 * j * j + (k >> 3)) & 0xFF | 1 for j in range(24))
        s = raw_deflate(data, 9)
        if 0 not in s:
            return data, s
    raise AssertionError("no such stream found")


def damaged_gzip_headers(data: bytes):
    """[(name, member)] that RFC 1952 or this library's limits refuse at the header"""
    out = [(f"reserved_bit_{b}", gzip_member(data, flg=1 << b)) for b in (5, 6, 7)]
    out.append(("cm_7", gzip_member(data, cm=7)))
    out.append(("bad_id1", b"\x1e" + gzip_member(data)[1:]))
    out.append(("bad_id2", b"\x1f\x8a" + gzip_member(data)[2:]))
    for x in (1, 0x8000):
        out.append((f"wrong_fhcrc_{x:x}", gzip_member(data, flg=FHCRC | FNAME, hcrc_xor=x)))
    d0, s0 = stream_without_zero_byte()
    m = gzip_header(flg=FNAME, name=b"no_nul_here", name_nul=False) + s0
    trailer = gzip_trailer(d0)
    out.append(("fname_without_nul", m + trailer))
    h = gzip_header(flg=FEXTRA, xlen=0)
    out.append(("xlen_passes_the_end", h[:10] + struct.pack("<H", 60000) + raw_deflate(data) + gzip_trailer(data)))
    whole = gzip_member(data, flg=FEXTRA, xlen=5)
    out.append(("xlen_reaches_into_the_trailer",
                whole[:10] + struct.pack("<H", len(whole) - 12 - 7) + whole[12:]))
    return out


def damaged_zlib_headers(data: bytes):
    return [("fdict", zlib_member(data, fdict=1)), ("bad_fcheck", zlib_member(data, fcheck_xor=1)),
            ("cinfo_8", zlib_member(data, cinfo=8)), ("cm_7", zlib_member(data, cm=7))]


def header_model(member: bytes, wrapper: int):
    """The header rules of include/hipcomp/gzip.h written out once more: -> (taken?, where the payload starts).
    The payload ends where the trailer starts, TRAILER[wrapper] bytes in front of the member's end."""
    n = len(member)
    if wrapper == ZLIB:
        if n < 6:
            return False, 0
        cmf, flg = member[0], member[1]
        return (cmf & 15 == 8 and cmf >> 4 <= 7 and (cmf * 256 + flg) % 31 == 0 and not flg & 32), 2
    if n < 18 or member[:3] != b"\x1f\x8b\x08" or member[3] & 0xE0:
        return False, 0
    flg, at, limit = member[3], 10, n - 8
    if flg & FEXTRA:
        if at + 2 > limit:
            return False, 0
        at += 2 + struct.unpack_from("<H", member, at)[0]
        if at > limit:
            return False, 0
    for bit in (FNAME, FCOMMENT):
        if flg & bit:
            nul = member.find(b"\0", at, limit)
            if nul < 0:
                return False, 0
            at = nul + 1
    if flg & FHCRC:
        if at + 2 > limit or struct.unpack_from("<H", member, at)[0] != zlib.crc32(member[:at]) & 0xFFFF:
            return False, 0
        at += 2
    return True, at


OK, CANNOT, BAD_CHECKSUM = 0, 12, 13


def status_model(member: bytes, wrapper: int, capacity: int):
    """-> (status, decoded bytes or None) by the rule of include/hipcomp/gzip.h: a refused header or a stream the raw
    decoder refuses (illegal, cut short, or larger than the capacity) is CannotDecompress; a stream that decodes --
    bytes behind its final block are ignored -- with another checksum or ISIZE is BadChecksum."""
    taken, at = header_model(member, wrapper)
    if not taken:
        return CANNOT, None
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(member[at:len(member) - TRAILER[wrapper]])
    except zlib.error:
        return CANNOT, None
    if not d.eof or len(got) > capacity:
        return CANNOT, None
    if wrapper == ZLIB:
        same = struct.unpack(">I", member[-4:])[0] == zlib.adler32(got)
    else:
        same = struct.unpack("<II", member[-8:]) == (zlib.crc32(got), len(got) & 0xFFFFFFFF)
    return (OK, got) if same else (BAD_CHECKSUM, None)
