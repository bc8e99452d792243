"""A Parquet page's dense values placed in rows as the Cascaded manager does it (hipcomp/cascaded.hpp,
place_parquet_values, place_parquet_booleans and place_parquet_strings; hipcomp-core_amd/csrc/parquet_plain_plan.hpp has
the rules; INTEGRATION.md, "PLAIN Parquet values placed in rows in the Cascaded manager", the contract): the three calls
with exactly those rules -- the restatement the tests compare the C++ with --, the planned items (deterministic, every
one built to meet an edge of the kernels or a rule that refuses) and the reader of the pyarrow fixtures of
tests/golden/parquet_plain/ (make_fixtures.py there writes them; the tests read only the committed files)."""
import json
import os
import random
import struct

import parquet_deltagen as D
import parquet_dictgen as G
import parquet_hybridgen as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_plain")

SUCCESS, CANNOT_DECOMPRESS = 0, 12
MAX_OFFSET = (1 << 31) - 1
FILL = 0xA5                                       # what the drivers fill an output with before the call
VALUES, BOOLEANS, STRINGS = "V", "B", "S"
PLAIN, SPLIT = 0, 1                               # hipcomp::ParquetValueLayout
LENGTH_PREFIXED, PACKED = 0, 1                    # hipcomp::ParquetStringLayout
Refused = G.Refused
bitmap = G.bitmap


# ---- the restatement -------------------------------------------------------------------------------------------------
def valid_rows(num_values, levels, max_level):
    """the rows' validity, after the rules of the levels; Refused"""
    if levels is None:
        return [True] * num_values
    if any(v > max_level for v in levels):
        raise Refused("a level above the maximum")
    valid = [v == max_level for v in levels]
    if valid.count(True) != num_values:
        raise Refused("the valid rows are not the values")
    return valid


def _behind(src, start):
    if start > len(src):
        raise Refused("a start above the bytes")
    return src[start:]


def place_values(src, start, num_values, levels, max_level, capacity, value_bytes, layout):
    """(the rows' values, the validity bitmap); Refused"""
    rows = num_values if levels is None else len(levels)
    if rows > capacity:
        raise Refused("more rows than the capacity")
    body = _behind(src, start)
    if num_values * value_bytes > len(body):
        raise Refused("the source does not hold its values")
    valid = valid_rows(num_values, levels, max_level)
    out, j = bytearray(), 0
    for v in valid:
        if not v:
            out += bytes(value_bytes)
        elif layout == PLAIN:
            out += body[j * value_bytes:(j + 1) * value_bytes]
        else:
            out += bytes(body[b * num_values + j] for b in range(value_bytes))
        j += v
    return bytes(out), bitmap(valid)


def place_booleans(src, start, num_values, levels, max_level, capacity):
    """(the values bitmap, the validity bitmap); Refused"""
    rows = num_values if levels is None else len(levels)
    if rows > capacity:
        raise Refused("more rows than the capacity")
    body = _behind(src, start)
    if (num_values + 7) // 8 > len(body):
        raise Refused("the source does not hold its bits")
    valid = valid_rows(num_values, levels, max_level)
    bits, j = [], 0
    for v in valid:
        bits.append(bool(v and (body[j >> 3] >> (j & 7)) & 1))
        j += v
    return bitmap(bits), bitmap(valid)


def place_strings(src, start, offsets, num_values, levels, max_level, offset_capacity, byte_capacity, layout):
    """(the rows + 1 offsets, the bytes, the validity bitmap); Refused.  Only offsets[0, num_values] are looked at."""
    rows = num_values if levels is None else len(levels)
    if rows + 1 > offset_capacity:
        raise Refused("more offsets than the capacity")
    body = _behind(src, start)
    valid = valid_rows(num_values, levels, max_level)
    total = 0
    for k in range(num_values):
        a, b = offsets[k], offsets[k + 1]
        if a < 0 or a > b or (4 * (k + 1) if layout == LENGTH_PREFIXED else 0) + b > len(body):
            raise Refused("an offset")
        total += b - a
        if total > byte_capacity or total > MAX_OFFSET:
            raise Refused("the bytes")
    out_offsets, out, j = [0], bytearray(), 0
    for v in valid:
        if v:
            at = (4 * (j + 1) if layout == LENGTH_PREFIXED else 0) + offsets[j]
            out += body[at:at + offsets[j + 1] - offsets[j]]
            j += 1
        out_offsets.append(len(out))
    return out_offsets, bytes(out), bitmap(valid)


def _padded(data, size):
    assert len(data) <= size
    return data + bytes([FILL]) * (size - len(data))


def _i32(values):
    return struct.pack("<%di" % len(values), *values)


# ---- an item of a call -------------------------------------------------------------------------------------------------
class Item:
    """src, start, num_values, levels (None: dense), max_level, and: VALUES capacity, value_bytes, layout; BOOLEANS
    capacity; STRINGS offsets (the array as it is handed over), offset_capacity, byte_capacity, layout."""

    def __init__(self, kind, name, **kw):
        self.kind, self.name = kind, name
        self.levels, self.max_level, self.start, self.value_bytes, self.layout = None, 0, 0, 0, 0
        self.__dict__.update(kw)
        self.src = bytes(self.src)
        self.levels = None if self.levels is None else bytes(self.levels)
        self.rows = self.num_values if self.levels is None else len(self.levels)
        if kind == STRINGS:
            self.offsets = list(self.offsets)
            assert self.num_values == 0 or len(self.offsets) > self.num_values, "the offsets the contract asks for"

    def call(self):
        """what has to be the same in all items of one call"""
        return (self.kind, self.value_bytes, self.layout, self.levels is not None)

    def sizes(self):
        """the bytes of every output, as the drivers lay them out"""
        if self.kind == VALUES:
            return [self.capacity * self.value_bytes, (self.rows + 7) // 8]
        if self.kind == BOOLEANS:
            return [(self.capacity + 7) // 8, (self.rows + 7) // 8]
        return [4 * self.offset_capacity, self.byte_capacity, (self.rows + 7) // 8]

    def model(self):
        """(status, the count the call reports, every output: the whole of it, FILL where nothing is written)"""
        try:
            if self.kind == VALUES:
                got, count = list(place_values(self.src, self.start, self.num_values, self.levels, self.max_level, self.capacity,
                                               self.value_bytes, self.layout)), 0
            elif self.kind == BOOLEANS:
                got, count = list(place_booleans(self.src, self.start, self.num_values, self.levels, self.max_level, self.capacity)), 0
            else:
                offsets, data, valid = place_strings(self.src, self.start, self.offsets, self.num_values, self.levels, self.max_level,
                                                     self.offset_capacity, self.byte_capacity, self.layout)
                got, count = [_i32(offsets), data, valid], len(data)
        except Refused:
            return CANNOT_DECOMPRESS, 0, [bytes([FILL]) * s for s in self.sizes()]
        return SUCCESS, count, [_padded(g, s) for g, s in zip(got, self.sizes())]

    def line(self, blob):
        """the item's line of a driver's list; its arrays are appended to `blob`"""
        def put(data):
            at = len(blob)
            blob.extend(data)
            return at
        words = [self.kind, put(self.src), len(self.src), self.start, self.num_values, int(self.levels is not None),
                 put(self.levels or b""), self.rows, self.max_level]
        if self.kind == VALUES:
            words += [self.capacity, self.value_bytes, self.layout]
        elif self.kind == BOOLEANS:
            words += [self.capacity]
        else:
            words += [put(_i32(self.offsets)), len(self.offsets), self.offset_capacity, self.byte_capacity, self.layout]
        return " ".join(str(w) for w in words)

    def but(self, name, **kw):
        fields = {k: v for k, v in self.__dict__.items() if k not in ("kind", "name", "rows")}
        fields.update(kw)
        return Item(self.kind, name, **fields)


def split(dense, value_bytes):
    """the BYTE_STREAM_SPLIT body of dense values"""
    n = len(dense) // value_bytes
    return bytes(dense[k * value_bytes + b] for b in range(value_bytes) for k in range(n))


# ---- the planned items -------------------------------------------------------------------------------------------------
ROWS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1003)
VALUE_BYTES = (1, 2, 3, 4, 5, 8, 12, 16, 64)
LAYOUT_NAME = {PLAIN: "plain", SPLIT: "split"}
STRING_LAYOUT_NAME = {LENGTH_PREFIXED: "prefixed", PACKED: "packed"}
# name -> the rows that are null
PATTERNS = {"all_valid": lambda r, n: False, "all_null": lambda r, n: True, "alternating": lambda r, n: r % 2 == 1,
            "last_row_alone_valid": lambda r, n: r != n - 1, "last_row_alone_null": lambda r, n: r == n - 1}


def _levels(rows, nulls):
    """a level of 1 but in the rows `nulls` says"""
    return bytes(0 if nulls(r, rows) else 1 for r in range(rows))


def _refusals_of_the_rows(it, prefix, suffix, capacity, counts=True):
    """the refusals every call shares, of an item with levels whose last step holds valid rows: each in the last step"""
    n = it.num_values
    last_valid = max(r for r in range(it.rows) if it.levels[r] == 1)
    last_null = max(r for r in range(it.rows) if it.levels[r] == 0)
    name = lambda what: "%s_%s%s" % (prefix, what, suffix)
    return [it.but(name("capacity_one_short"), **{capacity: getattr(it, capacity) - 1}),
            it.but(name("source_one_byte_short"), src=it.src[:-1]),
            it.but(name("start_one_above_the_bytes"), start=len(it.src) + 1),
            it.but(name("level_above_the_maximum_in_the_last_row"), levels=it.levels[:-1] + b"\2"),
            it.but(name("one_valid_row_more"), levels=it.levels[:last_null] + b"\1" + it.levels[last_null + 1:]),
            it.but(name("one_valid_row_fewer"), levels=it.levels[:last_valid] + b"\0" + it.levels[last_valid + 1:]),
            it.but(name("no_values_and_a_valid_row"), num_values=0, levels=bytes(it.rows - 1) + b"\1")] + ([
                it.but(name("one_value_more"), num_values=n + 1), it.but(name("one_value_fewer"), num_values=n - 1)] if counts else [])


def all_plans():
    rng = random.Random(30)
    plans = []
    blob = lambda n: bytes(rng.getrandbits(8) for _ in range(n))

    # -- place_parquet_values
    def values(name, rows, value_bytes, layout, nulls=None, start=0, **kw):
        levels = None if nulls is None else _levels(rows, nulls)
        there = rows if levels is None else levels.count(1)
        dense = blob(there * value_bytes)
        item = Item(VALUES, "values_%s_%s_w%d" % (name, LAYOUT_NAME[layout], value_bytes),
                    src=blob(start) + (dense if layout == PLAIN else split(dense, value_bytes)), start=start, num_values=there,
                    levels=levels, max_level=1, capacity=rows, value_bytes=value_bytes, layout=layout)
        plans.append(item.but(item.name, **kw) if kw else item)
        return plans[-1]
    for layout in (PLAIN, SPLIT):
        for w in VALUE_BYTES:
            suffix = "_%s_w%d" % (LAYOUT_NAME[layout], w)
            for rows in ROWS:
                values("%d_rows_dense" % rows, rows, w, layout, start=rows % 5)
                values("%d_rows_alternating" % rows, rows, w, layout, nulls=PATTERNS["alternating"], start=(rows + 2) % 5)
            for what, nulls in PATTERNS.items():
                if what != "alternating":
                    values("130_rows_" + what, 130, w, layout, nulls=nulls)
            values("null_at_63_64_127", 129, w, layout, nulls=lambda r, n: r in (63, 64, 127))
            values("valid_at_63_64_127", 129, w, layout, nulls=lambda r, n: r not in (63, 64, 127))
            it = values("every_fourth_null", 131, w, layout, nulls=lambda r, n: r % 4 == 0, start=3)
            plans.extend(_refusals_of_the_rows(it, "values", suffix, "capacity"))
            plans.append(it.but("values_bytes_behind_the_values" + suffix, src=it.src + blob(3), capacity=140))
            plans.append(it.but("values_start_at_the_end_all_null" + suffix, start=len(it.src), num_values=0, levels=bytes(131)))
            # (and with no start, for the calls without device_value_starts)
            flat = values("no_start_every_third_null", 70, w, layout, nulls=lambda r, n: r % 3 == 1)
            plans.append(flat.but("values_no_start_capacity_one_short" + suffix, capacity=69))
            plans.append(flat.but("values_no_start_source_one_byte_short" + suffix, src=flat.src[:-1]))
            flat = values("no_start_dense", 70, w, layout)
            plans.append(flat.but("values_no_start_dense_capacity_one_short" + suffix, capacity=69))
            plans.append(flat.but("values_no_start_dense_source_one_byte_short" + suffix, src=flat.src[:-1]))
            dense = values("dense_exact", 129, w, layout, start=1)
            plans.append(dense.but("values_dense_capacity_one_short" + suffix, capacity=128))
            plans.append(dense.but("values_dense_source_one_byte_short" + suffix, src=dense.src[:-1]))
            plans.append(dense.but("values_dense_start_one_above_the_bytes" + suffix, start=len(dense.src) + 1))
            plans.append(dense.but("values_dense_one_value_more" + suffix, num_values=130, capacity=130))
            plans.append(dense.but("values_dense_one_value_fewer" + suffix, num_values=128))
    deep = values("maximum_level_3", 130, 4, PLAIN, nulls=lambda r, n: r % 4 != 3)
    plans[-1] = deep.but(deep.name, levels=bytes(r % 4 for r in range(130)), max_level=3)
    plans.append(plans[-1].but("values_maximum_level_3_a_level_of_4_plain_w4", levels=bytes(r % 4 for r in range(129)) + b"\4"))
    plans.append(deep.but("values_maximum_level_300_plain_w4", levels=bytes(130), max_level=300, num_values=0))
    plans.append(deep.but("values_no_rows_and_no_source_plain_w4", levels=b"", num_values=0, src=b"", capacity=0))
    plans.append(deep.but("values_all_null_and_no_source_plain_w4", levels=bytes(130), num_values=0, src=b""))

    # -- place_parquet_booleans
    def booleans(name, rows, nulls=None, start=0, **kw):
        levels = None if nulls is None else _levels(rows, nulls)
        there = rows if levels is None else levels.count(1)
        item = Item(BOOLEANS, "booleans_" + name, src=blob(start + (there + 7) // 8), start=start, num_values=there, levels=levels,
                    max_level=1, capacity=rows)
        plans.append(item.but(item.name, **kw) if kw else item)
        return plans[-1]
    for rows in ROWS:
        booleans("%d_rows_dense" % rows, rows, start=rows % 3)
        booleans("%d_rows_alternating" % rows, rows, nulls=PATTERNS["alternating"], start=(rows + 1) % 3)
        booleans("%d_rows_every_third_null" % rows, rows, nulls=lambda r, n: r % 3 == 1)
    for what, nulls in PATTERNS.items():
        booleans("130_rows_" + what, 130, nulls=nulls)
    booleans("null_at_63_64_127", 129, nulls=lambda r, n: r in (63, 64, 127))
    it = booleans("every_fourth_null", 131, nulls=lambda r, n: r % 4 == 0, start=3)      # 98 bits: 13 bytes, 6 bits to spare
    plans.extend(_refusals_of_the_rows(it, "booleans", "", "capacity", counts=False))
    plans.append(it.but("booleans_seven_values_more", num_values=it.num_values + 7))    # (past the last byte's spare bits)
    plans.append(it.but("booleans_capacity_to_spare_and_bytes_behind", capacity=150, src=it.src + blob(2)))
    plans.append(it.but("booleans_all_bits_set", src=it.src[:3] + b"\xff" * 13))
    plans.append(it.but("booleans_no_bit_set", src=it.src[:3] + bytes(13)))
    plans.append(it.but("booleans_start_at_the_end_all_null", start=len(it.src), num_values=0, levels=bytes(131)))
    flat = booleans("no_start_every_fifth_null", 70, nulls=lambda r, n: r % 5 == 1)
    plans.append(flat.but("booleans_no_start_capacity_one_short", capacity=69))
    plans.append(flat.but("booleans_no_start_source_one_byte_short", src=flat.src[:-1]))
    dense = booleans("dense_exact", 129, start=1)
    plans.append(dense.but("booleans_dense_capacity_one_short", capacity=128))
    plans.append(dense.but("booleans_dense_source_one_byte_short", src=dense.src[:-1]))
    plans.append(dense.but("booleans_dense_start_one_above_the_bytes", start=len(dense.src) + 1))
    plans.append(dense.but("booleans_dense_eight_values_more", num_values=137, capacity=137))
    plans.append(dense.but("booleans_dense_set_bits_behind_the_values", src=dense.src[:-1] + bytes([dense.src[-1] | 0xFE])))

    # -- place_parquet_strings
    def strings(name, words, layout, nulls=None, start=0, **kw):
        """`words`: the value of every row; those of the valid rows are the values"""
        rows = len(words)
        levels = None if nulls is None else _levels(rows, nulls)
        there = [w for r, w in enumerate(words) if levels is None or levels[r]]
        body = G.byte_array_body(there) if layout == LENGTH_PREFIXED else b"".join(there)
        item = Item(STRINGS, "strings_%s_%s" % (name, STRING_LAYOUT_NAME[layout]), src=blob(start) + body, start=start,
                    offsets=G.offsets_of(there), num_values=len(there), levels=levels, max_level=1, offset_capacity=rows + 1,
                    byte_capacity=sum(len(w) for w in there), layout=layout)
        plans.append(item.but(item.name, **kw) if kw else item)
        return plans[-1]
    short = lambda n: [blob(rng.choice((0, 1, 2, 3, 5, 8, 13))) for _ in range(n)]
    long_ones = [blob(n) for n in (1, 63, 64, 65, 300)]
    mixed = lambda n: [long_ones[r % 7] if r % 7 < 5 and r % 3 == 0 else w for r, w in enumerate(short(n))]
    for layout in (LENGTH_PREFIXED, PACKED):
        suffix = "_" + STRING_LAYOUT_NAME[layout]
        for rows in ROWS:
            strings("%d_rows_dense" % rows, short(rows), layout, start=rows % 4)
            strings("%d_rows_alternating" % rows, mixed(rows), layout, nulls=PATTERNS["alternating"], start=(rows + 1) % 4)
        for what, nulls in PATTERNS.items():
            strings("130_rows_" + what, mixed(130), layout, nulls=nulls)
        strings("all_empty", [b""] * 129, layout, nulls=lambda r, n: r % 3 == 1)
        strings("all_empty_dense", [b""] * 129, layout)
        strings("null_at_63_64_127", mixed(129), layout, nulls=lambda r, n: r in (63, 64, 127))
        strings("a_step_of_empty_rows_between_two_of_bytes", [long_ones[r % 5] if r < 64 or r >= 128 else b"" for r in range(192)], layout)
        strings("300_bytes_in_rows_63_and_64", [long_ones[4] if r in (63, 64) else w for r, w in enumerate(short(130))], layout)
        strings("300_bytes_in_every_row", [long_ones[4]] * 70, layout, nulls=lambda r, n: r % 9 == 0)
        strings("lengths_1_63_64_65_300_in_turn", [long_ones[r % 5] for r in range(131)], layout, nulls=lambda r, n: r % 11 == 3)
        it = strings("every_fourth_null", mixed(131), layout, nulls=lambda r, n: r % 4 == 0, start=3)
        n, off = it.num_values, it.offsets
        plans.extend(_refusals_of_the_rows(it, "strings", suffix, "offset_capacity", counts=False))
        plans.append(it.but("strings_bytes_one_short" + suffix, byte_capacity=it.byte_capacity - 1))
        plans.append(it.but("strings_no_byte_capacity" + suffix, byte_capacity=0))
        plans.append(it.but("strings_capacities_to_spare_and_bytes_behind" + suffix, byte_capacity=it.byte_capacity + 9,
                            offset_capacity=it.offset_capacity + 2, src=it.src + blob(5)))
        plans.append(it.but("strings_one_value_fewer" + suffix, num_values=n - 1))
        plans.append(it.but("strings_one_value_more" + suffix, num_values=n + 1, offsets=off + [off[-1]]))
        plans.append(it.but("strings_the_last_offset_falls" + suffix, offsets=off[:-1] + [off[-2] - 1], byte_capacity=20000))
        plans.append(it.but("strings_an_offset_falls" + suffix, offsets=off[:40] + [off[39] - 1] + off[41:], byte_capacity=20000))
        plans.append(it.but("strings_a_negative_offset" + suffix, offsets=[-1] + off[1:], byte_capacity=20000))
        plans.append(it.but("strings_the_lowest_offset_last" + suffix, offsets=off[:-1] + [-(1 << 31)], byte_capacity=20000))
        plans.append(it.but("strings_the_last_end_one_past_the_body" + suffix, offsets=off[:-1] + [off[-1] + 1], byte_capacity=20000))
        plans.append(it.but("strings_the_last_end_at_the_end_of_the_body" + suffix, offsets=off[:-1] + [off[-1] + 1], src=it.src + b"\x77",
                            byte_capacity=20000))
        plans.append(it.but("strings_the_highest_offset_last" + suffix, offsets=off[:-1] + [MAX_OFFSET], byte_capacity=20000))
        # a byte total of 2^31 from the offsets alone: -1 first, 2^31 - 1 last; refused before any byte of the body is read
        plans.append(it.but("strings_a_byte_total_of_2_31" + suffix, offsets=[-1] + off[1:-1] + [MAX_OFFSET], byte_capacity=20000))
        plans.append(it.but("strings_no_body" + suffix, src=b"", start=0))
        plans.append(it.but("strings_start_at_the_end_all_null" + suffix, start=len(it.src), num_values=0, levels=bytes(131), byte_capacity=0))
        plans.append(it.but("strings_all_null_and_no_offsets" + suffix, num_values=0, levels=bytes(131), offsets=[], byte_capacity=0))
        for what, nulls in (("every_third_null", lambda r, n: r % 3 == 1), ("dense", None)):
            flat = strings("no_start_" + what, mixed(70), layout, nulls=nulls)
            plans.append(flat.but("strings_no_start_%s_bytes_one_short%s" % (what, suffix), byte_capacity=flat.byte_capacity - 1))
            plans.append(flat.but("strings_no_start_%s_offsets_one_short%s" % (what, suffix), offset_capacity=flat.offset_capacity - 1))
        dense = strings("dense_exact", mixed(129), layout, start=1)
        plans.append(dense.but("strings_dense_bytes_one_short" + suffix, byte_capacity=dense.byte_capacity - 1))
        plans.append(dense.but("strings_dense_offsets_one_short" + suffix, offset_capacity=dense.offset_capacity - 1))
        plans.append(dense.but("strings_dense_source_one_byte_short" + suffix, src=dense.src[:-1]))
        plans.append(dense.but("strings_dense_start_one_above_the_bytes" + suffix, start=len(dense.src) + 1))
        plans.append(dense.but("strings_dense_no_values_and_no_offsets" + suffix, num_values=0, offsets=[], byte_capacity=0, offset_capacity=1))
    # packed offsets need not begin at 0: the values' bytes are body[off[0], off[n])
    shifted = strings("offsets_from_7", mixed(70), PACKED, nulls=lambda r, n: r % 5 == 0)
    plans[-1] = shifted.but(shifted.name, src=blob(7) + shifted.src, offsets=[o + 7 for o in shifted.offsets])
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
    """a data page of a fixture: `page`, the level stream and the values section as they lie in the file, one behind the
    other; `levels`, a parquet_hybridgen Plan of the level stream (width 1, the ones counted); `encoding`: plain, split,
    boolean, rle_boolean (a 4-byte length, then hybrid runs of width 1: decode_parquet_hybrid's, then values of 1 byte),
    delta (DELTA_BINARY_PACKED: decode_parquet_delta's, then values of 8 bytes), prefixed (PLAIN BYTE_ARRAY) or packed
    (DELTA_LENGTH_BYTE_ARRAY); and what the table pyarrow was given says the rows hold: want_values (value_bytes each,
    zeros where null), want_bits, or want_offsets and want_bytes, and want_validity"""

    def dense(self):
        """(source, start, offsets or None) by the restatements of the earlier calls.  A V1 page's source is the whole
        page and the start the bytes of its levels; a V2 page's is the values section."""
        if self.encoding == "rle_boolean":
            got, _ = H.decode(self.values, H.LENGTH_PREFIXED, 1, self.non_null, self.non_null, H.UCHAR)
            return bytes(got), 0, None
        if self.encoding == "delta":
            got, _, _ = D.decode(self.values, self.non_null, self.non_null, D.VALUES, D.LONGLONG)
            return struct.pack("<%dQ" % len(got), *got), 0, None
        if self.encoding == "prefixed":
            return self.values, 0, G.index_dictionary(self.values, self.non_null, self.non_null + 1)
        if self.encoding == "packed":
            offsets, consumed, _ = D.decode(self.values, self.non_null, self.non_null + 1, D.OFFSETS, D.INT)
            return self.values, consumed, offsets
        if self.version == "v1":
            return self.page, len(self.levels.data), None
        return self.values, 0, None

    def item(self):
        """the placing of the page, its levels decoded by the restatement of decode_parquet_hybrid"""
        levels, _ = H.decode(self.levels.data, self.levels.form, 1, self.rows, self.rows, H.UCHAR)
        src, start, offsets = self.dense()
        common = dict(src=src, start=start, num_values=self.non_null, levels=bytes(levels), max_level=1)
        if self.encoding == "boolean":
            return Item(BOOLEANS, self.name, capacity=self.rows, **common)
        if offsets is not None:
            return Item(STRINGS, self.name, offsets=offsets, offset_capacity=self.rows + 1, byte_capacity=len(self.want_bytes),
                        layout=LENGTH_PREFIXED if self.encoding == "prefixed" else PACKED, **common)
        return Item(VALUES, self.name, capacity=self.rows, value_bytes=self.value_bytes, layout=SPLIT if self.encoding == "split" else PLAIN,
                    **common)


def fixture_pages():
    pages = []
    for name in fixture_names():
        blob, manifest = load_fixture(name)
        form = H.LENGTH_PREFIXED if manifest["data_page_version"] == "1.0" else H.BARE
        cut = lambda where: blob[where[0]:where[0] + where[1]]
        for k, p in enumerate(manifest["pages"]):
            g = Page()
            g.name, g.version, g.column, g.encoding = "%s_%d" % (name, k), name[:2], manifest["column"], manifest["encoding"]
            g.value_bytes = manifest["value_bytes"]
            g.rows, g.non_null = p["num_values"], p["non_null"]
            g.want_levels, g.want_validity = cut(p["expected_levels"]), cut(p["expected_validity"])
            assert p["values"][0] == p["level_stream"][0] + p["level_stream"][1], "the values lie behind the levels"
            g.values, g.page = cut(p["values"]), cut([p["level_stream"][0], p["level_stream"][1] + p["values"][1]])
            g.levels = H.Plan(g.name + "_levels", cut(p["level_stream"]), g.rows, 1, form=form, element=H.UCHAR, match=1)
            if "expected_values" in p:
                g.want_values = cut(p["expected_values"])
            elif "expected_bits" in p:
                g.want_bits = cut(p["expected_bits"])
            else:
                g.want_offsets = list(struct.unpack("<%di" % (g.rows + 1), cut(p["expected_offsets"])))
                g.want_bytes = cut(p["expected_bytes"])
            pages.append(g)
    return pages
