"""Parquet DELTA_BINARY_PACKED streams as the Cascaded manager reads them (hipcomp/cascaded.hpp, decode_parquet_delta;
hipcomp-core_amd/csrc/parquet_delta_plan.hpp has the rules; INTEGRATION.md, "Parquet DELTA_BINARY_PACKED values and string
offsets in the Cascaded manager", the contract): the decoder with exactly those rules -- the restatement the tests compare
the C++ with --, two writers (an encoder of values, and a builder that is told every width), the planned streams
(deterministic, every one built to meet a rule or an edge of the kernel) and the reader of the pyarrow fixtures of
tests/golden/parquet_delta/ (make_fixtures.py there writes them; the tests read only the committed files)."""
import json
import os
import random
import struct

import parquet_hybridgen as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_delta")

SUCCESS, CANNOT_DECOMPRESS = 0, 12
VALUES, OFFSETS = 0, 1                 # ParquetDeltaOutput
INT, LONGLONG = 4, 8                   # the element's bytes (hipcompType_t 4 and 6 in the drivers)
HIPCOMP_TYPE = {INT: 4, LONGLONG: 6}
LETTER = {INT: "I", LONGLONG: "Q"}


class Refused(Exception):
    pass


# ---- the restatement -------------------------------------------------------------------------------------------------
def read_varint(data, pos, end):
    v = n = 0
    while True:
        if n == 10:
            raise Refused("a varint of more than 10 bytes")
        if pos >= end:
            raise Refused("the stream ends in a varint")
        b = data[pos]
        pos += 1
        if n == 9 and b > 1:
            raise Refused("a varint of more than 64 bits")
        v |= (b & 0x7F) << (7 * n)
        n += 1
        if not b & 0x80:
            return v, pos


def unzigzag(u):
    return (u >> 1) ^ -(u & 1)


def read_stream_header(data):
    """(block size, miniblocks per block, total count, first value, where the header ends)"""
    n = len(data)
    block, pos = read_varint(data, 0, n)
    miniblocks, pos = read_varint(data, pos, n)
    total, pos = read_varint(data, pos, n)
    first, pos = read_varint(data, pos, n)
    if block >> 32 or miniblocks >> 32 or total >> 32:
        raise Refused("a header field that does not fit 32 bits")
    if block == 0 or block % 128:
        raise Refused("the block size")
    if miniblocks == 0 or block % miniblocks:
        raise Refused("the miniblock count")
    if block // miniblocks % 32:
        raise Refused("the values per miniblock")
    return block, miniblocks, total, unzigzag(first), pos


def decode(data, wanted, capacity, output, element, trace=None):
    """(the elements, the consumed bytes, the total count) of an item; Refused.  wanted None: device_num_values is null.
    trace: a list that takes (what, first byte, behind the last byte) of every part of the stream that is read."""
    n, bits = len(data), 8 * element
    block, miniblocks, total, first, pos = read_stream_header(data)
    if trace is not None:
        trace.append(("header", 0, pos))
    if total + (output == OFFSETS) > capacity:
        raise Refused("more elements than the capacity")
    if wanted is not None and wanted != total:
        raise Refused("the total is not the count the caller holds")
    per = block // miniblocks
    mask = (1 << (32 if output == OFFSETS else bits)) - 1   # lengths are INT32 whatever the offsets are
    values = [first & mask] if total else []
    left = max(total - 1, 0)
    while left:
        at = pos
        min_delta, pos = read_varint(data, pos, n)
        min_delta = unzigzag(min_delta)
        if n - pos < miniblocks:
            raise Refused("the stream ends in the width bytes")
        if trace is not None:
            trace += [("min_delta", at, pos), ("widths", pos, pos + miniblocks)]
        widths, pos = pos, pos + miniblocks
        in_block = min(left, block)
        for m in range(-(-in_block // per)):        # the miniblocks that hold a wanted value
            w = data[widths + m]
            if w > bits:
                raise Refused("a width above the element's bits")
            size = per * w // 8
            if size > n - pos:
                raise Refused("the stream ends in a needed miniblock")
            if trace is not None:
                trace.append(("miniblock", pos, pos + size))
            packed = int.from_bytes(data[pos:pos + size], "little")
            for k in range(min(per, in_block - m * per)):
                values.append((values[-1] + min_delta + ((packed >> (k * w)) & ((1 << w) - 1))) & mask)
            pos += size
        left -= in_block
    if output == VALUES:
        return values, pos, total
    offsets = [0]
    for v in values:
        if v >> 31:
            raise Refused("a negative length")
        offsets.append(offsets[-1] + v)
    if element == INT and offsets[-1] > (1 << 31) - 1:
        raise Refused("the lengths' sum does not fit the offsets")
    if offsets[-1] > n - pos:
        raise Refused("the lengths' sum runs past the item")
    return offsets, pos, total


def model(data, wanted, capacity, output, element):
    """what the call says of an item: (status, the output bytes, consumed, count)"""
    try:
        out, consumed, total = decode(data, wanted, capacity, output, element)
    except Refused:
        return CANNOT_DECOMPRESS, b"", 0, 0
    return SUCCESS, struct.pack("<%d%s" % (len(out), LETTER[element]), *out), consumed, total


# ---- the writers -------------------------------------------------------------------------------------------------------
def varint(u, pad=0):
    """`pad` more bytes than needed: 0x80 ... 0x00 behind the value"""
    out = bytearray()
    while True:
        out.append((u & 0x7F) | (0x80 if u >> 7 or pad else 0))
        u >>= 7
        if not u:
            break
    for k in range(pad):
        out.append(0x80 if k + 1 < pad else 0)
    return bytes(out)


def zigzag(v):
    """of a signed value of up to 64 bits"""
    return ((v << 1) ^ (v >> 63)) & ((1 << 64) - 1)


def stream_header(block, miniblocks, total, first):
    return varint(block) + varint(miniblocks) + varint(total) + varint(zigzag(first))


def pack(deltas, width, per):
    bits = 0
    for k, d in enumerate(deltas):
        assert d < (1 << width) or width == 0 and d == 0
        bits |= d << (k * width)
    return bits.to_bytes(per * width // 8, "little")


def a_block(min_delta, widths, deltas, per, unneeded=()):
    """deltas: a list per needed miniblock (the last padded with zeros here); unneeded: the width bytes behind them"""
    return varint(zigzag(min_delta)) + bytes(widths) + bytes(unneeded) + b"".join(pack(d, w, per) for d, w in zip(deltas, widths))


def signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def encode(values, block, miniblocks, bits, unneeded=0):
    """the stream a writer makes of the values (signed or unsigned, of `bits` bits): wrapping deltas, the least width"""
    per = block // miniblocks
    out = bytearray(stream_header(block, miniblocks, len(values), signed(values[0], bits) if values else 0))
    deltas = [signed(b - a, bits) for a, b in zip(values, values[1:])]
    for at in range(0, len(deltas), block):
        mine = deltas[at:at + block]
        least = min(mine)
        rest = [(d - least) & ((1 << bits) - 1) for d in mine]
        minis = [rest[k:k + per] for k in range(0, len(rest), per)]
        widths = [max(d.bit_length() for d in mini) for mini in minis]
        out += a_block(least, widths, minis, per, [unneeded] * (miniblocks - len(minis)))
    return bytes(out)


def build(rng, block, miniblocks, total, width_of, bits, first=None, min_delta_of=None, unneeded=255):
    """a stream whose miniblock m of block b has width_of(b, m) bits of random deltas"""
    per = block // miniblocks
    out = bytearray(stream_header(block, miniblocks, total, signed(rng.getrandbits(bits), bits) if first is None else first))
    left, b = max(total - 1, 0), 0
    while left:
        in_block = min(left, block)
        needed = -(-in_block // per)
        widths = [width_of(b, m) for m in range(needed)]
        minis = [[rng.getrandbits(w) if w else 0 for _ in range(min(per, in_block - m * per))] for m, w in enumerate(widths)]
        least = signed(rng.getrandbits(bits), bits) if min_delta_of is None else min_delta_of(b)
        out += a_block(least, widths, minis, per, [unneeded] * (miniblocks - needed))
        left -= in_block
        b += 1
    return bytes(out)


# ---- the planned streams -----------------------------------------------------------------------------------------------
class Plan:
    """an item.  wanted None: the call's device_num_values is null.  cap: "E" (exactly the elements the stream's header
    asks for), "S" (one short of them) or a number."""

    def __init__(self, name, data, output=VALUES, element=LONGLONG, wanted=None, cap="E"):
        self.name, self.data, self.output, self.element, self.wanted, self.cap = name, bytes(data), output, element, wanted, cap

    def capacity(self):
        if not isinstance(self.cap, str):
            return self.cap
        try:
            exact = min(read_stream_header(self.data)[2], 1 << 16) + (self.output == OFFSETS)
        except Refused:
            exact = 8
        return max(exact - 1, 0) if self.cap == "S" else exact

    def model(self):
        return model(self.data, self.wanted, self.capacity(), self.output, self.element)

    def short(self):
        return Plan(self.name + "_capacity_short", self.data, self.output, self.element, self.wanted, "S")


SHAPES = ((128, 4), (128, 2), (384, 4), (128, 1))            # 32, 64, 96 and 128 values per miniblock
MORE_SHAPES = ((256, 8), (1024, 8), (256, 2), (384, 2), (1024, 1), (1024, 4), (256, 4))
WIDTHS = {INT: (0, 1, 7, 8, 9, 31, 32), LONGLONG: (0, 1, 7, 8, 9, 31, 32, 33, 57, 63, 64)}


def _strings(rng, lengths):
    return rng.randbytes(sum(lengths))


def all_plans():
    rng = random.Random(20241028)
    plans = []

    def add(name, data, output=VALUES, element=LONGLONG, **kw):
        plans.append(Plan(name, data, output, element, **kw))

    def add_lengths(name, lengths, block, miniblocks, behind=0, **kw):
        """a DELTA_LENGTH_BYTE_ARRAY page of the lengths, in both offset types; behind: bytes more (or fewer) than their sum"""
        data = encode(lengths, block, miniblocks, 32)
        body = _strings(rng, [max(sum(v for v in lengths if v > 0) + behind, 0)])
        for element in (INT, LONGLONG):
            add("%s_offsets_e%d" % (name, element), data + body, OFFSETS, element, **kw)

    # the sizes: totals around a step, a miniblock, a block and two blocks, in every shape; random widths
    for block, miniblocks in SHAPES + MORE_SHAPES:
        totals = (0, 1, 2, 31, 32, 33, 63, 64, 65, 66, block - 1, block, block + 1, block + 2, 2 * block + 1, 2 * block + 2)
        if (block, miniblocks) in MORE_SHAPES:
            totals = (block + 2, 2 * block + 1)
        for total in totals:
            for element in (INT, LONGLONG):
                pool = WIDTHS[element]
                data = build(rng, block, miniblocks, total, lambda b, m: pool[rng.randrange(len(pool))], 8 * element)
                add("size_%d_%d_%d_e%d" % (block, miniblocks, total, element), data, VALUES, element,
                    wanted=total if total % 2 else None)
            add_lengths("size_%d_%d_%d" % (block, miniblocks, total), [rng.randrange(0, 9) for _ in range(total)], block, miniblocks,
                        wanted=total if total % 2 else None)
    # the widths: every miniblock of two blocks and a step at one width; the same in one miniblock of four
    for element in (INT, LONGLONG):
        for w in WIDTHS[element] + (8 * element + 1, 255):
            for block, miniblocks in ((128, 4), (256, 4), (384, 4)):
                add("width_%d_%d_%d_e%d" % (w, block, miniblocks, element),
                    build(rng, block, miniblocks, 2 * block + 70, lambda b, m: w, 8 * element), VALUES, element)
            add("width_%d_in_one_miniblock_e%d" % (w, element),
                build(rng, 128, 4, 300, lambda b, m: w if (b, m) == (1, 2) else 3, 8 * element), VALUES, element)
            # ... of a miniblock that holds no wanted value: its width byte is stepped over
            add("width_%d_unneeded_e%d" % (w, element), build(rng, 128, 4, 128 + 40, lambda b, m: 5, 8 * element, unneeded=w),
                VALUES, element)
    # lengths whose deltas need 1 to 32 bits (Offsets runs the delta layer in 32 bits under both offset types)
    for w in (1, 7, 8, 9, 12, 16):
        add_lengths("lengths_below_2_%d" % w, [rng.getrandbits(w) for _ in range(6 if w > 12 else 20 if w > 9 else 200)], 128, 4)
    for element in (INT, LONGLONG):
        for w in (33, 64):   # a width above 32 in a stream of lengths: refused with 4-byte offsets, truncated with 8-byte ones
            data = stream_header(128, 4, 3, 5) + a_block(0, [w], [[(1 << 32) + 3, (1 << (w - 1)) + 4]], 32, [0, 0, 0])
            add("lengths_width_%d_e%d" % (w, element), data + b"x" * (5 + 8 + 12), OFFSETS, element)
    # the arithmetic: extreme first values and minimum deltas, sums that wrap, varints with more bits than the element
    for element in (INT, LONGLONG):
        bits = 8 * element
        low, high = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        for block, miniblocks in ((128, 4), (256, 4)):
            add("alternating_ends_%d_e%d" % (block, element), encode([(low, high)[i % 2] for i in range(block + 70)], block, miniblocks, bits),
                VALUES, element)
            add("ends_and_noise_%d_e%d" % (block, element),
                encode([(low, high, rng.getrandbits(bits))[i % 3] for i in range(block + 70)], block, miniblocks, bits), VALUES, element)
        for name, least in (("lowest", -(1 << 63)), ("highest", (1 << 63) - 1), ("minus_one", -1)):
            add("min_delta_%s_e%d" % (name, element),
                build(rng, 128, 4, 200, lambda b, m: bits, bits, first=least, min_delta_of=lambda b: least), VALUES, element)
        add("first_value_of_64_bits_e%d" % element, build(rng, 128, 2, 70, lambda b, m: 9, bits, first=(1 << 62) + 12345), VALUES, element)
    # the varints: longer than needed, as long as can be, too long, too large
    good = build(rng, 128, 4, 150, lambda b, m: 6, 64, first=7, min_delta_of=lambda b: -3)
    rest = good[len(stream_header(128, 4, 150, 7)):]
    behind = rest[len(varint(zigzag(-3))):]
    for name, head in (("padded_block_size", varint(128, 1) + varint(4) + varint(150) + varint(14)),
                       ("padded_to_10_bytes", varint(128, 8) + varint(4, 9) + varint(150, 8) + varint(14, 9)),
                       ("block_size_of_11_bytes", varint(128, 9) + varint(4) + varint(150) + varint(14)),
                       ("miniblocks_of_11_bytes", varint(128) + varint(4, 10) + varint(150) + varint(14)),
                       ("total_of_11_bytes", varint(128) + varint(4) + varint(150, 9) + varint(14)),
                       ("first_of_11_bytes", varint(128) + varint(4) + varint(150) + varint(14, 10)),
                       ("first_tenth_byte_2", varint(128) + varint(4) + varint(150) + b"\x8e" + b"\x80" * 8 + b"\x02"),
                       ("first_tenth_byte_1", varint(128) + varint(4) + varint(150) + b"\x8e" + b"\x80" * 8 + b"\x01"),
                       ("block_size_2_32", varint((1 << 32) + 128) + varint(4) + varint(150) + varint(14)),
                       ("miniblocks_2_32", varint(128) + varint((1 << 32) + 4) + varint(150) + varint(14)),
                       ("total_2_32", varint(128) + varint(4) + varint((1 << 32) + 150) + varint(14)),
                       ("block_size_0", varint(0) + varint(4) + varint(150) + varint(14)),
                       ("block_size_64", varint(64) + varint(2) + varint(150) + varint(14)),
                       ("block_size_192", varint(192) + varint(2) + varint(150) + varint(14)),
                       ("miniblocks_0", varint(128) + varint(0) + varint(150) + varint(14)),
                       ("miniblocks_3", varint(128) + varint(3) + varint(150) + varint(14)),
                       ("miniblocks_8_of_16", varint(128) + varint(8) + varint(150) + varint(14)),
                       ("miniblocks_8_of_48", varint(384) + varint(8) + varint(150) + varint(14))):
        for element in (INT, LONGLONG):
            add("%s_e%d" % (name, element), head + rest, VALUES, element)
    add("min_delta_padded", stream_header(128, 4, 150, 7) + varint(zigzag(-3), 3) + behind)
    add("min_delta_of_11_bytes", stream_header(128, 4, 150, 7) + varint(zigzag(-3), 10) + behind)
    add("min_delta_tenth_byte_2", stream_header(128, 4, 150, 7) + b"\x85" + b"\x80" * 8 + b"\x02" + behind)
    # the header alone: totals of 0 and 1 have no block, whatever follows; the first value is parsed all the same
    for element in (INT, LONGLONG):
        for output in (VALUES, OFFSETS):
            for total in (0, 1):
                add("header_alone_%d_o%d_e%d" % (total, output, element), stream_header(128, 4, total, 5) + b"hello", output, element)
                add("header_alone_%d_first_cut_o%d_e%d" % (total, output, element), stream_header(128, 4, total, 5)[:-1], output, element)
                add("header_alone_%d_first_too_long_o%d_e%d" % (total, output, element),
                    varint(128) + varint(4) + varint(total) + varint(10, 10), output, element)
            add("header_alone_1_negative_o%d_e%d" % (output, element), stream_header(128, 4, 1, -5) + b"hello", output, element)
    # the cuts: at every structural place of a stream of two blocks and a step, and the last miniblock a byte short
    for element, output in ((INT, VALUES), (LONGLONG, VALUES), (INT, OFFSETS), (LONGLONG, OFFSETS)):
        if output == VALUES:
            data = build(rng, 128, 4, 128 * 2 + 40, lambda b, m: (9, 0, 17, 8 * element)[(b + m) % 4], 8 * element,
                         first=-(1 << 40), min_delta_of=lambda b: -(1 << 20))
        else:
            data = encode([rng.randrange(0, 300) for _ in range(128 * 2 + 40)], 128, 4, 32)
        trace = []
        values, consumed, total = decode(data + bytes(1 << 17), None, 1 << 20, output, element, trace)
        assert consumed == len(data)
        tail = _strings(rng, [values[-1]]) if output == OFFSETS else b""
        cuts = set()
        for what, lo, hi in trace:
            cuts |= {lo, hi - 1} | ({lo + 1} if what == "header" else set())
        for cut in sorted(c for c in cuts if c < len(data)):
            add("cut_at_%d_o%d_e%d" % (cut, output, element), data[:cut], output, element)
        add("cut_nowhere_o%d_e%d" % (output, element), data + tail, output, element)
        add("trailing_bytes_o%d_e%d" % (output, element), data + tail + b"\xff" * 9, output, element)
        # the count the caller holds, the capacity
        for wanted in (total - 1, total, total + 1, 0):
            add("wanted_%d_of_%d_o%d_e%d" % (wanted, total, output, element), data + tail, output, element, wanted=wanted)
        add("capacity_one_short_o%d_e%d" % (output, element), data + tail, output, element, cap="S")
        add("capacity_of_the_total_o%d_e%d" % (output, element), data + tail, output, element, cap=total)
        add("wanted_0_holds_0_o%d_e%d" % (output, element), stream_header(128, 4, 0, 0), output, element, wanted=0)
        add("wanted_0_holds_0_no_capacity_o%d_e%d" % (output, element), stream_header(128, 4, 0, 0), output, element, wanted=0, cap=0)
    # a miniblock that holds no wanted value has no bytes, but the block has its width byte
    data = build(rng, 128, 4, 128 + 40, lambda b, m: 0 if b else 5, 64)   # (width 0: the stream ends with the width bytes)
    add("unneeded_width_bytes_there", data)
    add("unneeded_width_byte_cut", data[:-1])
    # Offsets: a negative length first, in the first step, behind it, in the second block; the sums
    for where in (0, 1, 63, 64, 65, 127, 128, 129, 200):
        lengths = [rng.randrange(0, 9) for _ in range(260)]
        lengths[where] = -1 - (where % 3)
        add_lengths("negative_length_at_%d" % where, lengths, 128, 4)
    add_lengths("lowest_length", [3, -(1 << 31), 4], 128, 4)
    add_lengths("sum_2_31", [1 << 30, 1 << 30], 128, 4, behind=-(1 << 31) + 64)
    add_lengths("sum_2_31_behind_a_block", [0] * 130 + [(1 << 31) - 1, 1], 128, 4, behind=-(1 << 31) + 64)
    add_lengths("largest_length_no_bytes", [(1 << 31) - 1], 128, 4, behind=-(1 << 31) + 1 + 64)
    add_lengths("sum_is_the_bytes_behind", [rng.randrange(0, 9) for _ in range(300)], 128, 4)
    add_lengths("sum_one_above_the_bytes_behind", [rng.randrange(1, 9) for _ in range(300)], 128, 4, behind=-1)
    add_lengths("sum_below_the_bytes_behind", [rng.randrange(0, 9) for _ in range(300)], 128, 4, behind=5)
    add_lengths("empty_strings", [0] * 200, 128, 4)
    assert len({p.name for p in plans}) == len(plans)
    return plans


# ---- the pyarrow fixtures ------------------------------------------------------------------------------------------
def fixture_names():
    return sorted(n[:-5] for n in os.listdir(GOLDEN) if n.endswith(".json"))


def load_fixture(name):
    with open(os.path.join(GOLDEN, name + ".bin"), "rb") as f:
        blob = f.read()
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return blob, json.load(f)


class Page:
    """a data page of a fixture: `levels` a parquet_hybridgen Plan (width 1, the ones counted), `plan` the value stream with
    the non-null count as its wanted count, and what the table pyarrow was given says they hold"""


def fixture_pages():
    pages = []
    for name in fixture_names():
        blob, manifest = load_fixture(name)
        form = H.LENGTH_PREFIXED if manifest["data_page_version"] == "1.0" else H.BARE
        for k, p in enumerate(manifest["pages"]):
            cut = lambda key: blob[p[key][0]:p[key][0] + p[key][1]]
            g = Page()
            g.name, g.version, g.column = "%s_%d" % (name, k), name[:2], manifest["column"]
            g.block_size, g.miniblocks = p["block_size"], p["miniblocks"]
            g.want_levels = list(cut("expected_levels"))
            g.levels = H.Plan(g.name + "_levels", cut("level_stream"), p["num_values"], 1, form=form, element=H.UCHAR, match=1)
            assert len(g.want_levels) == p["num_values"] and g.want_levels.count(1) == p["non_null"]
            if manifest["element_bytes"]:
                g.plan = Plan(g.name, cut("value_stream"), VALUES, manifest["element_bytes"], wanted=p["non_null"])
                g.want = list(struct.unpack("<%d%s" % (p["non_null"], LETTER[g.plan.element]), cut("expected_values")))
                g.want_bytes = None
            else:
                g.plan = Plan(g.name, cut("value_stream"), OFFSETS, INT, wanted=p["non_null"])
                g.want = list(struct.unpack("<%dI" % (p["non_null"] + 1), cut("expected_offsets")))
                g.want_bytes = cut("expected_bytes")
            pages.append(g)
    return pages
