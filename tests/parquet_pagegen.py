"""Parquet column chunks as the Snappy manager reads them (hipcomp/snappy.hpp, decompress_parquet_pages;
hipcomp-core_amd/csrc/parquet_pages_plan.hpp has the rules): a Thrift compact-protocol writer and reader, the page rules
and the model of an item's result -- the restatement the tests compare the C++ with --, a raw Snappy block writer and
reader, the planned chunks (deterministic, a few hundred bytes each, every one with the verdict it is built to get) and
the generator of the pyarrow fixtures.

`python tests/parquet_pagegen.py` writes tests/golden/parquet_pages/<name>.chunks and <name>.json; it needs pyarrow.
The tests read only the committed files."""
import hashlib
import json
import os
import struct
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_pages")

SUCCESS, INVALID_VALUE, CANNOT_DECOMPRESS, BAD_CHECKSUM, CANNOT_VERIFY = 0, 10, 12, 13, 14
UNCOMPRESSED, SNAPPY = 0, 1                       # ParquetCodec
VERIFYING = (2, 3, 4)                             # ChecksumPolicy values that compare; 4 also wants every crc
T_TRUE, T_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, T_STRUCT = range(1, 13)
DATA_PAGE, INDEX_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = range(4)
HAS_CRC, VALUES_STORED = 1, 2
MAX_DEPTH = 8
PAGE_FIELDS = ("header_offset", "body_offset", "out_offset", "compressed_page_size", "uncompressed_page_size", "kind",
               "num_values", "encoding", "rep_levels_bytes", "def_levels_bytes", "num_nulls", "num_rows", "crc", "flags")
PAGE_STRUCT = struct.Struct("<QQQ12I")            # ParquetPageInfo: the fields above and the pad


# ---- Thrift compact protocol: the writer ---------------------------------------------------------------------------
def varint(u):
    out = bytearray()
    while u >= 0x80:
        out.append((u & 0x7F) | 0x80)
        u >>= 7
    out.append(u)
    return bytes(out)


def zigzag(n, bits=32):
    return ((n << 1) ^ (n >> (bits - 1))) & ((1 << bits) - 1)


class Raw:
    """a value given as the bytes that stand for it"""
    def __init__(self, data):
        self.data = bytes(data)


class LongId:
    """a field whose id is written in the long form whatever the delta"""
    def __init__(self, fid):
        self.fid = fid


def write_value(t, v, element):
    if isinstance(v, Raw):
        return v.data
    if t in (T_TRUE, T_FALSE):
        return (b"\x01" if t == T_TRUE else b"\x02") if element else b""
    if t == T_BYTE:
        return struct.pack("<b", v)
    if t in (T_I16, T_I32):
        return varint(zigzag(v, 32))
    if t == T_I64:
        return varint(zigzag(v, 64))
    if t == T_DOUBLE:
        return struct.pack("<d", v)
    if t == T_BINARY:
        return varint(len(v)) + bytes(v)
    if t in (T_LIST, T_SET):
        et, values = v[0], v[1]
        long_size = len(v) > 2 and v[2]
        head = bytes([0xF0 | et]) + varint(len(values)) if long_size or len(values) >= 15 else bytes([(len(values) << 4) | et])
        return head + b"".join(write_value(et, x, True) for x in values)
    if t == T_MAP:
        kt, vt, pairs = v
        if not pairs:
            return b"\x00"
        return varint(len(pairs)) + bytes([(kt << 4) | vt]) + b"".join(
            write_value(kt, k, True) + write_value(vt, x, True) for k, x in pairs)
    if t == T_STRUCT:
        return write_struct(v)
    raise ValueError(t)


def write_struct(fields):
    """fields: [(id or LongId, wire type, value)] in the order given"""
    out, last = bytearray(), 0
    for fid, t, v in fields:
        long_form = isinstance(fid, LongId)
        fid = fid.fid if long_form else fid
        delta = fid - last
        if long_form or not 0 < delta <= 15:
            out += bytes([t]) + varint(zigzag(fid, 32))
        else:
            out.append((delta << 4) | t)
        out += write_value(t, v, False)
        last = fid
    return bytes(out) + b"\x00"


# ---- the reader and the page rules: the restatement ----------------------------------------------------------------
class Refused(Exception):
    pass


class Reader:
    def __init__(self, data, pos, end):
        self.d, self.pos, self.end = data, pos, end

    def byte(self):
        if self.pos >= self.end:
            raise Refused("the header runs past the chunk")
        self.pos += 1
        return self.d[self.pos - 1]

    def step(self, n):
        if n > self.end - self.pos:
            raise Refused("the header runs past the chunk")
        self.pos += n

    def varint(self, most):
        v = 0
        for n in range(most):
            b = self.byte()
            v |= (b & 0x7F) << (7 * n)
            if not b & 0x80:
                return v
        raise Refused("a varint of more than %d bytes" % most)

    def i32(self):
        u = self.varint(5) & 0xFFFFFFFF
        v = (u >> 1) ^ -(u & 1)
        return v

    def size(self):
        u = self.varint(5) & 0xFFFFFFFF
        if u >> 31:
            raise Refused("a negative size")
        return u

    def field(self, last):
        """(id, type) or None at the stop byte"""
        h = self.byte()
        if h == 0:
            return None
        t = h & 15
        fid = (self.i32() if h >> 4 == 0 else last + (h >> 4)) & 0xFFFFFFFF
        if t == 0 or t > T_STRUCT:
            raise Refused("wire type %d" % t)
        return fid, t

    def skip(self, t, field, depth):
        """`depth` containers are open around the value"""
        if t == 0 or t > T_STRUCT:
            raise Refused("wire type %d" % t)
        if t in (T_TRUE, T_FALSE):
            self.step(0 if field else 1)
        elif t == T_BYTE:
            self.step(1)
        elif t in (T_I16, T_I32):
            self.varint(5)
        elif t == T_I64:
            self.varint(10)
        elif t == T_DOUBLE:
            self.step(8)
        elif t == T_BINARY:
            self.step(self.size())
        elif depth >= MAX_DEPTH:
            raise Refused("more than %d levels" % MAX_DEPTH)
        elif t == T_STRUCT:
            last = 0
            while True:
                f = self.field(last)
                if f is None:
                    break
                last = f[0]
                self.skip(f[1], True, depth + 1)
        elif t in (T_LIST, T_SET):
            h = self.byte()
            n = h >> 4
            if n == 15:
                n = self.size()
            if h & 15 == 0 or h & 15 > T_STRUCT:
                raise Refused("element type %d" % (h & 15))
            for _ in range(n):
                self.skip(h & 15, False, depth + 1)
        else:
            n = self.size()
            if n:
                kv = self.byte()
                for x in (kv >> 4, kv & 15):
                    if x == 0 or x > T_STRUCT:
                        raise Refused("element type %d" % x)
                for _ in range(n):
                    self.skip(kv >> 4, False, depth + 1)
                    self.skip(kv & 15, False, depth + 1)

    def ints(self, depth):
        """the i32 fields 1..7 of a struct and its bool field 7"""
        got, last = {}, 0
        while True:
            f = self.field(last)
            if f is None:
                return got
            last, t = f
            if t == T_I32 and 1 <= last <= 7:
                got[last] = self.i32()
            elif t in (T_TRUE, T_FALSE) and last == 7:
                got["flag7"] = t == T_TRUE
            else:
                self.skip(t, True, depth)


def parse_page(chunk, at, codec):
    """(page dict or None where the page is stepped over, where the next page starts); Refused"""
    r = Reader(chunk, at, len(chunk))
    top, structs, last = {}, {}, 0
    while True:
        f = r.field(last)
        if f is None:
            break
        last, t = f
        if t == T_I32 and 1 <= last <= 4:
            top[last] = r.i32()
        elif t == T_STRUCT and last in (5, 7, 8):
            structs[last] = r.ints(2)
        else:
            r.skip(t, True, 1)
    if not all(k in top for k in (1, 2, 3)):
        raise Refused("a field among 1-3 is missing")
    kind, usize, csize = top[1] & 0xFFFFFFFF, top[2], top[3]
    if usize < 0 or csize < 0:
        raise Refused("a negative size")
    if csize > len(chunk) - r.pos:
        raise Refused("the body runs past the chunk")
    nxt = r.pos + csize
    if kind == INDEX_PAGE or kind > DATA_PAGE_V2:
        return None, nxt
    mine = structs.get({DATA_PAGE: 5, DICTIONARY_PAGE: 7, DATA_PAGE_V2: 8}[kind])
    if mine is None:
        raise Refused("the struct of the page's kind is missing")
    stored = codec == UNCOMPRESSED
    p = dict.fromkeys(PAGE_FIELDS, 0)
    p.update(header_offset=at, body_offset=r.pos, compressed_page_size=csize, uncompressed_page_size=usize, kind=kind,
             num_values=mine.get(1, 0))
    if kind == DATA_PAGE_V2:
        p.update(num_nulls=mine.get(2, 0), num_rows=mine.get(3, 0), encoding=mine.get(4, 0), def_levels_bytes=mine.get(5, 0),
                 rep_levels_bytes=mine.get(6, 0))
        stored = stored or not mine.get("flag7", True)
    else:
        p.update(encoding=mine.get(2, 0))
    if min(p["num_values"], p["num_nulls"], p["num_rows"], p["rep_levels_bytes"], p["def_levels_bytes"]) < 0:
        raise Refused("a negative count or level length")
    levels = p["rep_levels_bytes"] + p["def_levels_bytes"]
    if levels > csize or levels > usize:
        raise Refused("the levels are larger than the page")
    if stored and csize != usize:
        raise Refused("a stored part of another length than its uncompressed length")
    p["encoding"] &= 0xFFFFFFFF
    p["crc"] = top[4] & 0xFFFFFFFF if 4 in top else 0
    p["flags"] = (HAS_CRC if 4 in top else 0) | (VALUES_STORED if stored else 0)
    return p, nxt


def walk(chunk, codec):
    """the listed pages of a chunk, out_offset filled in; Refused"""
    pages, pos, out = [], 0, 0
    while pos < len(chunk):
        p, pos = parse_page(chunk, pos, codec)
        if p is not None:
            p["out_offset"] = out
            out += p["uncompressed_page_size"]
            pages.append(p)
    return pages


def page_row(p):
    return PAGE_STRUCT.pack(*[p[k] for k in PAGE_FIELDS], 0)


# ---- raw Snappy blocks ---------------------------------------------------------------------------------------------
def snappy_literals(data):
    """a block of literals only"""
    out = bytearray(varint(len(data)))
    for at in range(0, len(data), 60):
        part = data[at:at + 60]
        out.append((len(part) - 1) << 2)
        out += part
    return bytes(out)


def snappy_repeat(pattern, times):
    """pattern * times: the pattern as a literal, the rest as copies with a two-byte offset"""
    assert 4 <= len(pattern) <= 60 and times >= 1
    left = len(pattern) * (times - 1)
    out = bytearray(varint(len(pattern) * times)) + bytes([(len(pattern) - 1) << 2]) + pattern
    while left:
        n = min(left, 64)
        out += bytes([((n - 1) << 2) | 2]) + struct.pack("<H", len(pattern))
        left -= n
    return bytes(out)


def snappy_decode(block):
    """the content of a raw Snappy block; ValueError"""
    n, shift, pos = 0, 0, 0
    while True:
        if pos >= len(block) or shift > 28:
            raise ValueError("preamble")
        b = block[pos]
        pos += 1
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out = bytearray()
    while pos < len(block):
        tag = block[pos]
        pos += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                extra = ln - 59
                if pos + extra > len(block):
                    raise ValueError("literal")
                ln = int.from_bytes(block[pos:pos + extra], "little")
                pos += extra
            ln += 1
            if pos + ln > len(block):
                raise ValueError("literal")
            out += block[pos:pos + ln]
            pos += ln
            continue
        if pos + (1, 2, 4)[kind - 1] > len(block):
            raise ValueError("copy")
        if kind == 1:
            ln, off = ((tag >> 2) & 7) + 4, ((tag >> 5) << 8) | block[pos]
            pos += 1
        elif kind == 2:
            ln, off = (tag >> 2) + 1, int.from_bytes(block[pos:pos + 2], "little")
            pos += 2
        else:
            ln, off = (tag >> 2) + 1, int.from_bytes(block[pos:pos + 4], "little")
            pos += 4
        if off == 0 or off > len(out):
            raise ValueError("copy")
        if off >= ln:
            out += out[len(out) - off:len(out) - off + ln]
        else:
            for _ in range(ln):
                out.append(out[-off])
    if len(out) != n:
        raise ValueError("size")
    return bytes(out)


def decode_page(chunk, p):
    """the decoded body of a listed page; ValueError"""
    body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
    if p["flags"] & VALUES_STORED:
        return body
    levels = p["rep_levels_bytes"] + p["def_levels_bytes"]
    want = p["uncompressed_page_size"] - levels
    if want == 0:
        return body[:levels]
    values = snappy_decode(body[levels:])
    if len(values) != want:
        raise ValueError("size")
    return body[:levels] + values


# ---- the model of an item's result ---------------------------------------------------------------------------------
def model(chunk, codec, policy, capacity=None, table_capacity=None):
    """(status, the output or b"", the listed pages or []) of one item"""
    failed = lambda status: (status, b"", [])
    try:
        pages = walk(chunk, codec)
    except Refused:
        return failed(CANNOT_DECOMPRESS)
    total = sum(p["uncompressed_page_size"] for p in pages)
    if table_capacity is not None and len(pages) > table_capacity:
        return failed(INVALID_VALUE)
    if capacity is not None and total > capacity:
        return failed(CANNOT_DECOMPRESS)
    if policy in VERIFYING:
        for p in pages:
            body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
            if p["flags"] & HAS_CRC and zlib.crc32(body) != p["crc"]:
                return failed(BAD_CHECKSUM)
    try:
        out = b"".join(decode_page(chunk, p) for p in pages)
    except ValueError:
        return failed(CANNOT_DECOMPRESS)
    bare = any(not p["flags"] & HAS_CRC for p in pages)
    return (CANNOT_VERIFY if policy == 4 and bare else SUCCESS), out, pages


# ---- pages, built --------------------------------------------------------------------------------------------------
def signed32(u):
    return u - (1 << 32) if u >> 31 else u


def make_page(kind, body, usize, crc="right", num_values=7, encoding=0, v2=None, extra=(), inner_extra=(), kind_struct=True,
              sizes=None, drop=()):
    """header + body.  v2: (num_nulls, num_rows, def bytes, rep bytes, is_compressed or None).  crc: "right", None,
    or the word.  sizes: (uncompressed, compressed) as written, numbers or Raw.  drop: top-level field ids left out."""
    csize = len(body)
    if sizes:
        usize, csize = sizes
    fields = [(1, T_I32, kind), (2, T_I32, usize), (3, T_I32, csize)]
    if crc is not None:
        fields.append((4, T_I32, signed32(zlib.crc32(body) if crc == "right" else crc)))
    if kind_struct:
        if kind == DATA_PAGE_V2:
            nulls, rows, dl, rl, comp = v2
            inner = [(1, T_I32, num_values), (2, T_I32, nulls), (3, T_I32, rows), (4, T_I32, encoding), (5, T_I32, dl), (6, T_I32, rl)]
            if comp is not None:
                inner.append((7, T_TRUE if comp else T_FALSE, None))
            fields.append((8, T_STRUCT, inner + list(inner_extra)))
        elif kind == DICTIONARY_PAGE:
            fields.append((7, T_STRUCT, [(1, T_I32, num_values), (2, T_I32, encoding)] + list(inner_extra)))
        else:
            fields.append(({DATA_PAGE: 5, INDEX_PAGE: 6}.get(kind, 5), T_STRUCT,
                           [(1, T_I32, num_values), (2, T_I32, encoding), (3, T_I32, 3), (4, T_I32, 3)] + list(inner_extra)))
    fields = [f for f in fields if f[0] not in drop] + list(extra)
    return write_struct(fields) + body


def nested(levels):
    """a struct of `levels` structs one inside the other, the innermost holding an i32"""
    v = [(1, T_I32, 5)]
    for _ in range(levels - 1):
        v = [(1, T_STRUCT, v)]
    return v


def lists(n, innermost=(T_BYTE, [1])):
    """the value of a list that is `n` lists deep, `innermost` being the last of them"""
    v = innermost
    for _ in range(n - 1):
        v = (T_LIST, [v])
    return v


class Plan:
    def __init__(self, name, data, codec=SNAPPY, note=""):
        self.name, self.data, self.codec, self.note = name, bytes(data), codec, note

    def result(self, policy, capacity=None, table_capacity=None):
        return model(self.data, self.codec, policy, capacity, table_capacity)


def all_plans():
    text = b"The walk of Thrift page headers on the device. " * 3
    ramp = bytes(range(40))
    lit, rep = snappy_literals(text), snappy_repeat(ramp, 9)
    good = [make_page(DICTIONARY_PAGE, lit, len(text), num_values=3, encoding=2),
            make_page(DATA_PAGE, rep, 360, num_values=90, encoding=8),
            make_page(DATA_PAGE, snappy_literals(ramp), 40, num_values=5)]
    plans = [Plan("empty_chunk", b""), Plan("three_pages", b"".join(good)), Plan("dictionary_alone", good[0])]
    one = make_page(DATA_PAGE, snappy_literals(ramp), 40)
    header = len(one) - len(snappy_literals(ramp))
    plans += [Plan("cut_%02d" % n, one[:n], note="a header cut at byte %d" % n) for n in range(1, header + 1)]
    plans.append(Plan("body_cut", one[:-1]))
    # sizes
    six = Raw(bytes([0x80 | (zigzag(40) & 0x7F), 0x80, 0x80, 0x80, 0x80, 0x00]))
    five = Raw(bytes([0x80 | (zigzag(40) & 0x7F), 0x80, 0x80, 0x80, 0x00]))
    body = snappy_literals(ramp)
    plans += [Plan("varint_six_bytes", make_page(DATA_PAGE, body, 40, sizes=(six, len(body)))),
              Plan("varint_five_bytes", make_page(DATA_PAGE, body, 40, sizes=(five, len(body)))),
              Plan("negative_uncompressed", make_page(DATA_PAGE, body, 40, sizes=(-1, len(body)))),
              Plan("negative_compressed", make_page(DATA_PAGE, body, 40, sizes=(40, -1))),
              Plan("negative_num_values", make_page(DATA_PAGE, body, 40, num_values=-1)),
              Plan("body_one_past_the_end", make_page(DATA_PAGE, body, 40, sizes=(40, len(body) + 1))),
              Plan("missing_field_2", make_page(DATA_PAGE, body, 40, drop=(2,))),
              Plan("missing_field_1", make_page(DATA_PAGE, body, 40, drop=(1,))),
              Plan("missing_kind_struct", make_page(DATA_PAGE, body, 40, kind_struct=False)),
              Plan("other_kinds_struct", write_struct([(1, T_I32, DATA_PAGE), (2, T_I32, 40), (3, T_I32, len(body)),
                                                       (7, T_STRUCT, [(1, T_I32, 7), (2, T_I32, 0)])]) + body)]
    # V2
    levels = bytes([3, 0, 0, 0, 5, 9]) + bytes([2, 1, 1])
    v2 = (1, 4, 3, 6, None)
    plans += [Plan("v2", make_page(DATA_PAGE_V2, levels + rep, 9 + 360, v2=v2)),
              Plan("v2_says_compressed", make_page(DATA_PAGE_V2, levels + rep, 9 + 360, v2=(1, 4, 3, 6, True))),
              Plan("v2_not_compressed", make_page(DATA_PAGE_V2, levels + text, 9 + len(text), v2=(1, 4, 3, 6, False))),
              Plan("v2_not_compressed_other_length", make_page(DATA_PAGE_V2, levels + text, 10 + len(text), v2=(1, 4, 3, 6, False))),
              Plan("v2_empty_values", make_page(DATA_PAGE_V2, levels, 9, v2=v2)),
              Plan("v2_empty_values_empty_block", make_page(DATA_PAGE_V2, levels + b"\x00", 9, v2=v2)),
              Plan("v2_levels_above_compressed", make_page(DATA_PAGE_V2, levels, 400, v2=(1, 4, 4, 6, None))),
              Plan("v2_levels_above_uncompressed", make_page(DATA_PAGE_V2, levels + rep, 8, v2=v2)),
              Plan("v2_negative_levels", make_page(DATA_PAGE_V2, levels + rep, 369, v2=(1, 4, -3, 6, None))),
              Plan("v2_values_without_block", make_page(DATA_PAGE_V2, levels, 9 + 40, v2=v2))]
    # every wire type, to be stepped over
    every = [(9, T_TRUE, None), (10, T_FALSE, None), (11, T_BYTE, -3), (12, T_I16, -300), (13, T_I32, 1 << 30),
             (14, T_I64, -(1 << 62)), (15, T_DOUBLE, 2.5), (16, T_BINARY, b"min and max"),
             (17, T_LIST, (T_I32, [1, -2, 3])), (18, T_LIST, (T_STRUCT, [[(1, T_I32, 1)], [(2, T_BINARY, b"x")], []])),
             (19, T_LIST, (T_TRUE, [True] * 20)), (20, T_LIST, (T_BYTE, [1, 2], True)), (21, T_SET, (T_BINARY, [b"a", b""])),
             (22, T_MAP, (T_I32, T_BINARY, [(1, b"one"), (2, b"two")])), (23, T_MAP, (T_I32, T_I32, [])),
             (24, T_MAP, (T_BINARY, T_STRUCT, [(b"k", [(1, T_LIST, (T_DOUBLE, [1.0, 2.0]))])])),
             (25, T_STRUCT, [(1, T_STRUCT, [(3, T_I64, 7)]), (2, T_TRUE, None)]), (LongId(26), T_I32, 9),
             (1000, T_I32, 1), (LongId(-5 & 0x7FFF), T_BINARY, b"far"), (40000, T_LIST, (T_I64, list(range(16))))]
    stats = [(5, T_STRUCT, [(1, T_BINARY, b"\xff" * 9), (2, T_BINARY, b""), (3, T_I64, 0), (5, T_BINARY, b"zz")])] + every[:8]
    plans += [Plan("every_wire_type", make_page(DATA_PAGE, rep, 360, extra=every)),
              Plan("every_wire_type_inside", make_page(DATA_PAGE, rep, 360, inner_extra=stats)),
              Plan("long_form_ids", write_struct([(LongId(1), T_I32, 0), (LongId(2), T_I32, 40), (LongId(3), T_I32, len(body)),
                                                  (LongId(5), T_STRUCT, [(LongId(1), T_I32, 7), (LongId(2), T_I32, 0)])]) + body),
              Plan("wire_type_0", make_page(DATA_PAGE, body, 40, extra=[(9, 0, Raw(b""))])),
              Plan("wire_type_13", make_page(DATA_PAGE, body, 40, extra=[(9, 13, Raw(b"\x00" * 16))])),
              Plan("element_type_13", make_page(DATA_PAGE, body, 40, extra=[(9, T_LIST, Raw(b"\x1d\x00"))])),
              Plan("i64_of_eleven_bytes", make_page(DATA_PAGE, body, 40, extra=[(9, T_I64, Raw(b"\x80" * 10 + b"\x00"))])),
              Plan("i64_of_ten_bytes", make_page(DATA_PAGE, body, 40, extra=[(9, T_I64, Raw(b"\x80" * 9 + b"\x01"))])),
              Plan("binary_past_the_end", make_page(DATA_PAGE, body, 40, extra=[(9, T_BINARY, Raw(varint(5000)))])),
              Plan("negative_list_size", make_page(DATA_PAGE, body, 40, extra=[(9, T_LIST, Raw(b"\xf5" + varint(0xFFFFFFFF)))])),
              # the page header is level 1: a field of it that is `n` structs deep opens levels 2 .. n + 1
              Plan("nesting_at_the_limit", make_page(DATA_PAGE, body, 40, extra=[(9, T_STRUCT, nested(7))])),
              Plan("nesting_beyond_the_limit", make_page(DATA_PAGE, body, 40, extra=[(9, T_STRUCT, nested(8))])),
              Plan("nesting_inside_at_the_limit", make_page(DATA_PAGE, body, 40, inner_extra=[(5, T_STRUCT, nested(6))])),
              Plan("nesting_inside_beyond_the_limit", make_page(DATA_PAGE, body, 40, inner_extra=[(5, T_STRUCT, nested(7))])),
              # two structs (levels 2 and 3), then lists of lists: the list of bytes is level 8, or 9
              Plan("list_at_the_limit", make_page(DATA_PAGE, body, 40, extra=[
                  (9, T_STRUCT, [(1, T_STRUCT, [(1, T_LIST, lists(5))])])])),
              Plan("list_beyond_the_limit", make_page(DATA_PAGE, body, 40, extra=[
                  (9, T_STRUCT, [(1, T_STRUCT, [(1, T_LIST, lists(6))])])])),
              Plan("map_at_the_limit", make_page(DATA_PAGE, body, 40, extra=[
                  (9, T_STRUCT, [(1, T_STRUCT, [(1, T_LIST, lists(4, (T_MAP, [(T_I32, T_I32, [(1, 2)])])))])])])),
              Plan("map_beyond_the_limit", make_page(DATA_PAGE, body, 40, extra=[
                  (9, T_STRUCT, [(1, T_STRUCT, [(1, T_LIST, lists(5, (T_MAP, [(T_I32, T_I32, [(1, 2)])])))])])]))]
    # pages that are stepped over
    index = make_page(INDEX_PAGE, b"index bytes", 11, crc=None)
    seven = make_page(7, b"a page of a kind to come", 24, crc=12345, kind_struct=False)
    plans += [Plan("stepped_over_between", good[0] + index + good[1] + seven + good[2]),
              Plan("stepped_over_alone", index + seven), Plan("stepped_over_cut", good[0] + index[:-1])]
    # checksums
    plans += [Plan("no_crc", good[0] + make_page(DATA_PAGE, rep, 360, crc=None)),
              Plan("wrong_crc", good[0] + make_page(DATA_PAGE, rep, 360, crc=zlib.crc32(rep) ^ 0x100)),
              Plan("wrong_crc_and_damaged", make_page(DATA_PAGE, rep[:-3] + b"\xfe\xff\xff", 360, crc=1))]
    # Snappy blocks
    damaged = varint(44) + bytes([3 << 2]) + b"abcd" + bytes([(39 << 2) | 2]) + struct.pack("<H", 100)
    plans += [Plan("preamble_one_above", make_page(DATA_PAGE, varint(361) + rep[2:], 360)),
              Plan("preamble_one_below", make_page(DATA_PAGE, varint(359) + rep[2:], 360)),
              Plan("header_one_above", make_page(DATA_PAGE, rep, 361)),
              Plan("header_one_below", make_page(DATA_PAGE, rep, 359)),
              Plan("damaged_block", make_page(DATA_PAGE, damaged, 44)),
              Plan("damaged_block_behind_good", good[0] + make_page(DATA_PAGE, damaged, 44)),
              Plan("block_cut", make_page(DATA_PAGE, rep[:-1], 360)),
              Plan("empty_block", make_page(DATA_PAGE, b"", 40))]
    # trailing bytes
    plans += [Plan("trailing_byte", b"".join(good) + b"\x15"), Plan("trailing_stop", b"".join(good) + b"\x00"),
              Plan("trailing_header", b"".join(good) + one[:header])]
    # the UNCOMPRESSED codec
    plans += [Plan("stored_pages", make_page(DICTIONARY_PAGE, text, len(text)) + make_page(DATA_PAGE, ramp, 40), UNCOMPRESSED),
              Plan("stored_v2", make_page(DATA_PAGE_V2, levels + text, 9 + len(text), v2=v2), UNCOMPRESSED),
              Plan("stored_other_length", make_page(DATA_PAGE, ramp, 41), UNCOMPRESSED),
              Plan("stored_empty_page", make_page(DATA_PAGE, b"", 0), UNCOMPRESSED),
              Plan("stored_wrong_crc", make_page(DATA_PAGE, ramp, 40, crc=7), UNCOMPRESSED)]
    assert len({p.name for p in plans}) == len(plans)
    return plans


def text_chunk(text, page_bytes, compress):
    """`text` cut into V1 data pages of page_bytes bytes, a CRC each (what the timing script reads)"""
    out = bytearray()
    for at in range(0, len(text), page_bytes):
        part = text[at:at + page_bytes]
        out += make_page(DATA_PAGE, compress(part), len(part), num_values=len(part))
    return bytes(out)


# ---- the pyarrow fixtures ------------------------------------------------------------------------------------------
def load_fixture(name):
    """(the bytes of <name>.chunks, the manifest)"""
    with open(os.path.join(GOLDEN, name + ".chunks"), "rb") as f:
        blob = f.read()
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return blob, json.load(f)


def fixture_names():
    return sorted(n[:-5] for n in os.listdir(GOLDEN) if n.endswith(".json"))


def manifest_of(blob, chunks):
    """the restatement's manifest: chunks = [{offset, length, codec, num_values}]"""
    done = []
    for c in chunks:
        chunk = blob[c["offset"]:c["offset"] + c["length"]]
        pages = walk(chunk, c["codec"])
        rows = []
        for p in pages:
            row = {k: p[k] for k in PAGE_FIELDS}
            row["sha256"] = hashlib.sha256(decode_page(chunk, p)).hexdigest()
            rows.append(row)
        done.append(dict(offset=c["offset"], length=c["length"], codec=c["codec"], num_values=c["num_values"], pages=rows))
    return done


def _generate():
    import io

    import pyarrow as pa
    import pyarrow.parquet as pq

    rows = 3600
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta"]
    table = pa.table({
        "ramp": pa.array(range(1000, 1000 + rows), pa.int64()),
        "word": pa.array([None if i % 11 == 0 else words[(i * i) % 7] for i in range(rows)], pa.string()),
        "level": pa.array([((i * 37) % 23) * 0.25 for i in range(rows)], pa.float64()),
        "runs": pa.array([[(i + k) % 9 for k in range(i % 4)] for i in range(rows)], pa.list_(pa.int32())),
    })
    big = pa.table({"cycle": pa.array([i % 100 for i in range(20000)], pa.int64())})
    kinds = {"v1_snappy": (table, dict(data_page_version="1.0", compression="snappy", data_page_size=4096,
                                       use_dictionary=["word", "level"], row_group_size=rows // 2)),
             "v2_snappy": (table, dict(data_page_version="2.0", compression="snappy", data_page_size=4096,
                                       use_dictionary=["word", "level"], row_group_size=rows // 2)),
             "v1_none": (table, dict(data_page_version="1.0", compression="none", data_page_size=4096,
                                     use_dictionary=["word", "level"], row_group_size=rows // 2)),
             "big_page": (big, dict(data_page_version="1.0", compression="snappy", use_dictionary=False))}
    os.makedirs(GOLDEN, exist_ok=True)
    snappy = pa.Codec("snappy")
    for name, (tab, opts) in kinds.items():
        sink = io.BytesIO()
        pq.write_table(tab, sink, write_page_checksum=True, write_batch_size=200, **opts)
        data = sink.getvalue()
        meta = pq.ParquetFile(io.BytesIO(data)).metadata
        blob, chunks = bytearray(), []
        for g in range(meta.num_row_groups):
            for c in range(meta.num_columns):
                col = meta.row_group(g).column(c)
                start = col.dictionary_page_offset if col.has_dictionary_page and col.dictionary_page_offset else col.data_page_offset
                codec = {"SNAPPY": SNAPPY, "UNCOMPRESSED": UNCOMPRESSED}[col.compression]
                chunks.append(dict(offset=len(blob), length=col.total_compressed_size, codec=codec, num_values=col.num_values))
                blob += data[start:start + col.total_compressed_size]
        blob = bytes(blob)
        assert len(blob) < 65536, (name, len(blob))
        manifest = manifest_of(blob, chunks)
        # what pyarrow says of the same bytes: the walk ends at the chunk's end (manifest_of would have refused), the
        # values add up, the CRCs are zlib's, and pyarrow's own Snappy decodes every compressed part to the same bytes
        for c in manifest:
            chunk = blob[c["offset"]:c["offset"] + c["length"]]
            assert sum(p["num_values"] for p in c["pages"] if p["kind"] != DICTIONARY_PAGE) == c["num_values"], name
            for p in c["pages"]:
                body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
                assert p["flags"] & HAS_CRC and zlib.crc32(body) == p["crc"], name
                levels = p["rep_levels_bytes"] + p["def_levels_bytes"]
                want = p["uncompressed_page_size"] - levels
                if p["flags"] & VALUES_STORED or want == 0:
                    decoded = body if p["flags"] & VALUES_STORED else body[:levels]
                else:
                    decoded = body[:levels] + snappy.decompress(body[levels:], decompressed_size=want).to_pybytes()
                assert hashlib.sha256(decoded).hexdigest() == p["sha256"], name
        if name == "big_page":
            assert max(p["uncompressed_page_size"] for c in manifest for p in c["pages"]) > 2 * 65536
        with open(os.path.join(GOLDEN, name + ".chunks"), "wb") as f:
            f.write(blob)
        with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
            json.dump(dict(pyarrow=pa.__version__, chunks=manifest), f, indent=1)
            f.write("\n")
        print(name, len(blob), "bytes,", len(manifest), "chunks,", sum(len(c["pages"]) for c in manifest), "pages,",
              sorted({p["kind"] for c in manifest for p in c["pages"]}))


if __name__ == "__main__":
    _generate()
