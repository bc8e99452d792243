"""Parquet RLE / bit-packed hybrid streams as the Cascaded manager reads them (hipcomp/cascaded.hpp,
decode_parquet_hybrid; hipcomp-core_amd/csrc/parquet_hybrid_plan.hpp has the rules; INTEGRATION.md, "Parquet levels and
dictionary indices in the Cascaded manager", the contract): the decoder with exactly those rules -- the restatement the
tests compare the C++ with --, a writer of runs, the planned streams (deterministic, every one built to meet an edge of
the kernel) and the reader of the pyarrow fixtures of tests/golden/parquet_hybrid/ (make_fixtures.py there writes them;
the tests read only the committed files)."""
import json
import os
import random
import struct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_hybrid")

SUCCESS, CANNOT_DECOMPRESS = 0, 12
BARE, LENGTH_PREFIXED, WIDTH_PREFIXED = 0, 1, 2    # ParquetHybridForm
UCHAR, USHORT, UINT = 1, 2, 4                      # the element's bytes (hipcompType_t 1, 3, 5 in the drivers)
HIPCOMP_TYPE = {UCHAR: 1, USHORT: 3, UINT: 5}


class Refused(Exception):
    pass


# ---- the restatement -------------------------------------------------------------------------------------------------
def read_header(data, pos, end):
    v = n = 0
    while True:
        if n == 5:
            raise Refused("a header of more than 5 bytes")
        if pos >= end:
            raise Refused("the stream ends in a header")
        b = data[pos]
        pos += 1
        v |= (b & 0x7F) << (7 * n)
        n += 1
        if not b & 0x80:
            break
    if v >> 32:
        raise Refused("a header that does not fit 32 bits")
    return v, pos


def next_run(data, pos, end, bit_width, wanted):
    """(values of the run that are wanted, where the run ends)"""
    h, pos = read_header(data, pos, end)
    count = h >> 1
    if count == 0:
        raise Refused("a run of nothing")
    room = end - pos
    if h & 1:
        take = min(count * 8, wanted)
        if (take * bit_width + 7) // 8 > room:
            raise Refused("the bit-packed values run past the stream")
        bits = int.from_bytes(data[pos:pos + (take * bit_width + 7) // 8], "little")
        mask = (1 << bit_width) - 1
        return [(bits >> (k * bit_width)) & mask for k in range(take)], pos + min(count * bit_width, room)
    vb = (bit_width + 7) // 8
    if vb > room:
        raise Refused("the RLE value runs past the stream")
    return [int.from_bytes(data[pos:pos + vb], "little")] * min(count, wanted), pos + vb


def decode(data, form, bit_width, wanted, capacity, element):
    """(the values, the consumed bytes) of an item; Refused"""
    n, pos, end = len(data), 0, len(data)
    if wanted > capacity:
        raise Refused("more values than the capacity")
    if form == LENGTH_PREFIXED:
        if n < 4:
            raise Refused("a cut length prefix")
        length = int.from_bytes(data[:4], "little")
        if length > n - 4:
            raise Refused("the length prefix runs past the item")
        pos, end = 4, 4 + length
    elif form == WIDTH_PREFIXED:
        if n == 0:
            if wanted:
                raise Refused("no width byte")
            return [], 0
        bit_width, pos = data[0], 1
    if bit_width > 32 or bit_width > 8 * element:
        raise Refused("the width")
    values = []
    while len(values) < wanted:
        got, pos = next_run(data, pos, end, bit_width, wanted - len(values))
        values += got
    return [v & ((1 << (8 * element)) - 1) for v in values], end if form == LENGTH_PREFIXED else pos


def model(data, form, bit_width, wanted, capacity, element, match=None):
    """what the call says of an item: (status, the output bytes, consumed, matches)"""
    try:
        values, consumed = decode(data, form, bit_width, wanted, capacity, element)
    except Refused:
        return CANNOT_DECOMPRESS, b"", 0, 0
    out = struct.pack("<%d%s" % (len(values), {1: "B", 2: "H", 4: "I"}[element]), *values)
    return SUCCESS, out, consumed, 0 if match is None else values.count(match)


# ---- the writer ------------------------------------------------------------------------------------------------------
def varint(u):
    out = bytearray()
    while True:
        out.append((u & 0x7F) | (0x80 if u >> 7 else 0))
        u >>= 7
        if not u:
            return bytes(out)


def rle(count, value, bit_width):
    return varint(count << 1) + value.to_bytes((bit_width + 7) // 8, "little")


def packed(values, bit_width, groups=None):
    """a bit-packed run of the values, padded with zeros to whole groups (or to `groups` of them)"""
    groups = (len(values) + 7) // 8 if groups is None else groups
    bits = 0
    for k, v in enumerate(values):
        assert v < (1 << bit_width) or bit_width == 0 and v == 0
        bits |= v << (k * bit_width)
    return varint((groups << 1) | 1) + bits.to_bytes(groups * bit_width, "little")


# ---- the planned streams -----------------------------------------------------------------------------------------------
class Plan:
    """an item: `cap` is "E" (exactly the wanted values) or "S" (one short)"""

    def __init__(self, name, data, wanted, bit_width=0, form=BARE, element=UINT, match=0, cap="E"):
        self.name, self.data, self.wanted, self.bit_width = name, bytes(data), wanted, bit_width
        self.form, self.element, self.match, self.cap = form, element, match, cap

    def capacity(self):
        return max(self.wanted - 1, 0) if self.cap == "S" else self.wanted

    def model(self):
        return model(self.data, self.form, self.bit_width, self.wanted, self.capacity(), self.element, self.match)


def _values(rng, n, bit_width):
    return [rng.getrandbits(bit_width) if bit_width else 0 for _ in range(n)]


def _smallest(bit_width):
    return UCHAR if bit_width <= 8 else USHORT if bit_width <= 16 else UINT


def all_plans():
    rng = random.Random(20240607)
    plans = []

    def add(name, data, wanted, bit_width=0, **kw):
        plans.append(Plan(name, data, wanted, bit_width, **kw))

    # every width: a group, an RLE run, 9 groups, an RLE run, 63 groups -- in the smallest element that holds it and in
    # UINT, bare and behind its width byte
    for w in (0, 1, 7, 8, 9, 16, 17, 24, 25, 31, 32):
        top = (1 << w) - 1
        v = _values(rng, 8 + 72 + 504, w)
        v[3], v[80] = top, top
        data = packed(v[:8], w) + rle(70, top, w) + packed(v[8:80], w) + rle(5, v[1], w) + packed(v[80:], w)
        total = 8 + 70 + 72 + 5 + 504
        for element in sorted({_smallest(w), UINT}):
            add("w%d_e%d_bare" % (w, element), data, total, w, element=element, match=top)
            add("w%d_e%d_width_byte" % (w, element), bytes([w]) + data, total, form=WIDTH_PREFIXED, element=element, match=v[1])
        add("w%d_level_prefixed" % w, struct.pack("<I", len(data)) + data, total, w, form=LENGTH_PREFIXED, match=top)
    # bit-packed runs of 1, 8, 9, 63 groups; headers of 2 and 3 bytes
    for groups in (1, 8, 9, 63, 64, 8192):
        for w in (1, 5, 12):
            v = _values(rng, groups * 8, w)
            data = packed(v, w)
            assert len(varint((groups << 1) | 1)) == (1 if groups < 64 else 2 if groups < 8192 else 3)
            add("packed_%d_groups_w%d" % (groups, w), data, groups * 8, w, element=_smallest(w), match=v[-1])
    # RLE runs of 1, 63, 64, 65 and 2^31 - 1 values, the last clipped by the wanted count
    for count in (1, 63, 64, 65, 200, 16384):
        add("rle_%d" % count, rle(count, 5, 3), count, 3, element=UCHAR, match=5)
        add("rle_%d_ushort_odd_start" % count, rle(1, 9, 11) + rle(count, 1500, 11), count + 1, 11, element=USHORT, match=1500)
    for element in (UCHAR, USHORT, UINT):
        add("rle_2_31_clipped_e%d" % element, rle((1 << 31) - 1, 201, 8) + rle(3, 1, 8), 333, 8, element=element, match=201)
    add("rle_2_31_then_more", rle(3, 2, 8) + rle((1 << 31) - 1, 7, 8), 1000, 8, element=UCHAR, match=7)
    # the wanted count ends inside a group, and 63, 64 and 65 values into a run
    v = _values(rng, 1024, 6)
    for wanted in (1, 5, 13, 63, 64, 65, 127, 128, 129, 1023):
        add("packed_wants_%d" % wanted, packed(v, 6), wanted, 6, element=UCHAR, match=v[0])
        add("rle_wants_%d" % wanted, rle(5000, 33, 6), wanted, 6, element=UCHAR, match=33)
        add("second_run_wants_%d" % wanted, rle(3, 1, 6) + packed(v, 6), 3 + wanted, 6, element=USHORT, match=1)
    # a header varint across the edge of the 64-byte window that begins with the stream, and an RLE value across it
    data = b"".join(rle(2, k, 8) for k in range(30)) + rle(64, 77, 8)
    assert len(data) == 63
    add("header_across_window", data + rle(100, 99, 8) + rle(2, 3, 8), 60 + 64 + 100 + 2, 8, element=UCHAR, match=99)
    add("packed_header_across_window", data + packed(_values(rng, 512, 8), 8) + rle(2, 3, 8), 60 + 64 + 512 + 2, 8, element=UCHAR)
    data = b"".join(rle(2, 1000 + k, 16) for k in range(19)) + rle(64, 77, 16)
    assert len(data) == 61
    add("value_across_window", data + rle(100, 0xBEEF, 16) + rle(2, 3, 16), 38 + 64 + 100 + 2, 16, element=USHORT, match=0xBEEF)
    data = bytes([16]) + b"".join(rle(2, 1000 + k, 16) for k in range(20))
    assert len(data) == 61
    add("value_across_window_behind_width_byte", data + rle(100, 0xBEEF, 16) + rle(2, 3, 16), 40 + 100 + 2,
        form=WIDTH_PREFIXED, element=USHORT, match=0xBEEF)
    # many short runs: the windows fall wherever the runs leave them
    for w in (1, 9, 20):
        parts, total = [], 0
        for k in range(120):
            if rng.random() < 0.5:
                c = rng.randrange(1, 9)
                parts.append(rle(c, rng.getrandbits(w), w))
            else:
                c = 8 * rng.randrange(1, 4)
                parts.append(packed(_values(rng, c, w), w))
            total += c
        add("short_runs_w%d" % w, b"".join(parts), total, w, match=1)
        add("short_runs_w%d_prefixed" % w, struct.pack("<I", len(b"".join(parts))) + b"".join(parts), total - 3, w,
            form=LENGTH_PREFIXED, element=_smallest(w), match=1)
    # a final run cut short: with exactly the bytes of the values wanted, and with one byte too few
    for w in (1, 7, 12, 25, 32):
        v = _values(rng, 24, w)
        whole = rle(4, v[0], w) + packed(v, w)
        for wanted in (9, 17, 23):
            need = len(rle(4, v[0], w)) + 1 + (wanted * w + 7) // 8
            add("cut_w%d_wants_%d_enough" % (w, wanted), whole[:need], 4 + wanted, w, match=v[0])
            add("cut_w%d_wants_%d_one_short" % (w, wanted), whole[:need - 1], 4 + wanted, w, match=v[0])
        add("cut_w%d_then_more_wanted" % w, whole[:-1], 4 + 24, w)
    # bytes behind the last run used
    add("trailing_bytes", rle(10, 3, 2) + b"\xff\xff\xff\xff\xff\xff", 10, 2, element=UCHAR, match=3)
    add("trailing_runs", rle(10, 3, 2) + rle(0, 0, 2) + b"\x01", 10, 2, element=UCHAR, match=3)
    add("trailing_behind_clipped_packed", packed(_values(rng, 16, 4), 4) + b"\x00\x01", 9, 4, element=UCHAR)
    # an RLE value with bits above the width: stored as read, truncated to the element
    add("rle_value_above_width", rle(7, 0xFF, 3), 7, 3, element=UCHAR, match=0xFF)
    add("rle_value_above_width_ushort", rle(7, 0xFFFF, 9), 7, 9, element=USHORT, match=0xFFFF)
    add("rle_value_above_width_uint", rle(7, 0xFFFFFF, 17), 7, 17, element=UINT, match=0xFFFFFF)
    # no values wanted: no run is read
    add("none_wanted_bare", b"\x00\x00", 0, 1)
    add("none_wanted_bare_empty", b"", 0, 1)
    add("none_wanted_bare_width_33", b"", 0, 33)
    add("none_wanted_prefixed", struct.pack("<I", 2) + b"\x00\x00\x07", 0, 1, form=LENGTH_PREFIXED)
    add("none_wanted_prefix_too_long", struct.pack("<I", 4) + b"\x00\x00\x07", 0, 1, form=LENGTH_PREFIXED)
    add("none_wanted_prefix_cut", b"\x00\x00\x00", 0, 1, form=LENGTH_PREFIXED)
    add("none_wanted_width_byte", b"\x05\x00", 0, form=WIDTH_PREFIXED)
    add("none_wanted_width_byte_40", b"\x28", 0, form=WIDTH_PREFIXED)
    add("none_wanted_no_width_byte", b"", 0, form=WIDTH_PREFIXED)
    # the length prefix: shorter than the item, equal to it, longer than it, cut
    runs = rle(40, 1, 1) + packed(_values(rng, 40, 1), 1) + rle(9, 0, 1)
    add("prefix_equal", struct.pack("<I", len(runs)) + runs, 89, 1, form=LENGTH_PREFIXED, element=UCHAR, match=1)
    add("prefix_shorter", struct.pack("<I", len(runs)) + runs + b"\x03\x09\x09", 89, 1, form=LENGTH_PREFIXED, element=UCHAR, match=1)
    add("prefix_longer", struct.pack("<I", len(runs) + 1) + runs, 89, 1, form=LENGTH_PREFIXED, element=UCHAR, match=1)
    add("prefix_cuts_the_runs", struct.pack("<I", len(runs) - 2) + runs, 89, 1, form=LENGTH_PREFIXED, element=UCHAR, match=1)
    add("prefix_cuts_the_runs_fewer_wanted", struct.pack("<I", len(runs) - 2) + runs, 80, 1, form=LENGTH_PREFIXED, element=UCHAR, match=1)
    add("prefix_of_3_bytes", b"\x02\x00\x00", 1, 1, form=LENGTH_PREFIXED)
    add("prefix_of_2_to_the_32", b"\xff\xff\xff\xff" + runs, 89, 1, form=LENGTH_PREFIXED)
    # the width: above 32, above the element's bits
    add("width_33", rle(5, 1, 33), 5, 33)
    add("width_2_to_the_31", rle(5, 1, 8), 5, 1 << 31)
    add("width_9_in_uchar", rle(5, 1, 9), 5, 9, element=UCHAR)
    add("width_17_in_ushort", rle(5, 1, 17), 5, 17, element=USHORT)
    add("width_byte_33", b"\x21" + rle(5, 1, 33), 5, form=WIDTH_PREFIXED)
    add("width_byte_255", b"\xff" + rle(5, 1, 8), 5, form=WIDTH_PREFIXED)
    add("width_byte_9_in_uchar", b"\x09" + rle(5, 1, 9), 5, form=WIDTH_PREFIXED, element=UCHAR)
    add("width_byte_17_in_ushort", b"\x11" + rle(5, 1, 17), 5, form=WIDTH_PREFIXED, element=USHORT)
    add("width_byte_16_ends_early", b"\x10" + rle(5, 1, 16) + packed(_values(rng, 8, 16), 16)[:-1], 13, form=WIDTH_PREFIXED, element=USHORT)
    add("width_byte_8_rle_of_0", b"\x08" + rle(5, 1, 8) + rle(0, 1, 8), 6, form=WIDTH_PREFIXED, element=UCHAR)
    add("prefixed_ushort_header_cut", struct.pack("<I", 4) + rle(5, 1, 9) + b"\x80", 6, 9, form=LENGTH_PREFIXED, element=USHORT)
    add("prefixed_uchar_ends_early", struct.pack("<I", 2) + rle(5, 1, 8) + rle(5, 1, 8), 6, 8, form=LENGTH_PREFIXED, element=UCHAR)
    add("no_width_byte_values_wanted", b"", 5, form=WIDTH_PREFIXED)
    add("width_byte_alone", b"\x04", 5, form=WIDTH_PREFIXED)
    # the refusals with the damage in the first run and in the last run
    good = rle(70, 2, 4) + packed(_values(rng, 72, 4), 4)
    damaged = {
        "header_6_bytes": b"\x82\x80\x80\x80\x80\x00" + b"\x01",
        "header_33_bits": b"\x82\x80\x80\x80\x10" + b"\x01",
        "header_cut": b"\x82\x80",
        "rle_of_0": rle(0, 1, 4),
        "packed_of_0_groups": b"\x01",
        "rle_value_cut": b"\x0a",
        "packed_bytes_cut": packed(_values(rng, 16, 4), 4)[:-4],   # (9 values are wanted of it: 5 bytes, 4 are there)
        "ends_early": b"",
    }
    for name, bad in damaged.items():
        add("first_" + name, bad, 9, 4, element=UCHAR)
        add("last_" + name, good + bad, 142 + 9, 4, element=UCHAR, match=2)
        add("behind_last_" + name, good + bad, 142, 4, element=UCHAR, match=2)
    add("header_32_bits", b"\xfe\xff\xff\xff\x0f\x09", 100, 4, element=UCHAR, match=9)
    add("rle_value_cut_w32", b"\x0a\x01\x02\x03", 5, 32)
    add("rle_value_cut_w9", rle(3, 1, 9) + b"\x0a\x01", 8, 9, element=USHORT)
    # more values than the capacity
    add("capacity_one_short", rle(10, 1, 1), 10, 1, element=UCHAR, cap="S")
    add("capacity_one_short_packed", packed(_values(rng, 640, 9), 9), 640, 9, element=USHORT, cap="S")
    add("capacity_one_short_width_byte", b"\x01" + rle(10, 1, 1), 10, form=WIDTH_PREFIXED, cap="S")
    assert len({p.name for p in plans}) == len(plans)
    return plans


# ---- the pyarrow fixtures ------------------------------------------------------------------------------------------
def fixture_names():
    return sorted(n[:-5] for n in os.listdir(GOLDEN) if n.endswith(".json"))


def load_fixture(name):
    """(the bytes of <name>.bin, the manifest): per page the level stream and the index stream as they lie in the file,
    and what they hold according to the table pyarrow was given (levels: a byte each; indices: 4 bytes each)"""
    with open(os.path.join(GOLDEN, name + ".bin"), "rb") as f:
        blob = f.read()
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return blob, json.load(f)


def fixture_pages():
    """[(name, levels Plan, its expected values, indices Plan, its expected values)], a page each"""
    pages = []
    for name in fixture_names():
        blob, manifest = load_fixture(name)
        form = LENGTH_PREFIXED if manifest["data_page_version"] == "1.0" else BARE
        for k, p in enumerate(manifest["pages"]):
            cut = lambda key: blob[p[key][0]:p[key][0] + p[key][1]]
            levels = list(cut("expected_levels"))
            indices = list(struct.unpack("<%dI" % (p["expected_indices"][1] // 4), cut("expected_indices")))
            assert len(levels) == p["num_values"] and len(indices) == levels.count(1) == p["non_null"]
            pages.append(("%s_%d" % (name, k),
                          Plan("%s_%d_levels" % (name, k), cut("level_stream"), p["num_values"], 1, form=form, element=UCHAR, match=1),
                          levels,
                          Plan("%s_%d_indices" % (name, k), cut("index_stream"), p["non_null"], form=WIDTH_PREFIXED,
                               element=_smallest(p["index_bit_width"]), match=indices[0] if indices else 0),
                          indices))
    return pages
