"""A Parquet dictionary's entries gathered to rows as the Cascaded manager does it (hipcomp/cascaded.hpp,
index_parquet_dictionary, gather_parquet_dictionary and gather_parquet_dictionary_strings;
hipcomp-core_amd/csrc/parquet_dict_plan.hpp has the rules; INTEGRATION.md, "Parquet dictionary entries gathered to rows
in the Cascaded manager", the contract): the three calls with exactly those rules -- the restatement the tests compare the
C++ with --, the planned items (deterministic, every one built to meet an edge of the kernels or a rule that refuses)
and the reader of the pyarrow fixtures of tests/golden/parquet_dict/ (make_fixtures.py there writes them; the tests
read only the committed files)."""
import json
import os
import random
import struct

import parquet_hybridgen as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_dict")

SUCCESS, CANNOT_DECOMPRESS = 0, 12
MAX_OFFSET = (1 << 31) - 1
FILL = 0xA5                                       # what the drivers fill an output with before the call
INDEX, FIXED, STRINGS = "I", "F", "S"


class Refused(Exception):
    pass


# ---- the restatement -------------------------------------------------------------------------------------------------
def index_dictionary(body, entries, capacity):
    """the entries + 1 offsets of a PLAIN BYTE_ARRAY dictionary page body; Refused"""
    if entries + 1 > capacity:
        raise Refused("more offsets than the capacity")
    offsets, n = [0], len(body)
    for k in range(entries):
        pos = 4 * k + offsets[-1]
        if n - pos < 4:
            raise Refused("the body ends inside a length word")
        length = int.from_bytes(body[pos:pos + 4], "little")
        if length > n - pos - 4:
            raise Refused("a length runs past the body")
        if offsets[-1] + length > MAX_OFFSET:
            raise Refused("a sum above 2^31 - 1")
        offsets.append(offsets[-1] + length)
    return offsets


def valid_rows(indices, num_indices, levels, max_level, dict_entries):
    """the rows' validity, after the rules of the levels and the indices; Refused"""
    if levels is None:
        valid = [True] * num_indices
    else:
        if any(v > max_level for v in levels):
            raise Refused("a level above the maximum")
        valid = [v == max_level for v in levels]
        if valid.count(True) != num_indices:
            raise Refused("the valid rows are not the indices")
    if any(i >= dict_entries for i in indices[:num_indices]):
        raise Refused("an index outside the dictionary")
    return valid


def bitmap(valid):
    return sum(v << i for i, v in enumerate(valid)).to_bytes((len(valid) + 7) // 8, "little")


def gather(body, dict_entries, indices, num_indices, levels, max_level, capacity, entry_bytes):
    """(the rows' entries, the validity bitmap); Refused"""
    rows = num_indices if levels is None else len(levels)
    if rows > capacity:
        raise Refused("more rows than the capacity")
    if dict_entries * entry_bytes > len(body):
        raise Refused("the dictionary does not hold its entries")
    valid = valid_rows(indices, num_indices, levels, max_level, dict_entries)
    out, j = bytearray(), 0
    for v in valid:
        if v:
            out += body[indices[j] * entry_bytes:(indices[j] + 1) * entry_bytes]
            j += 1
        else:
            out += bytes(entry_bytes)
    return bytes(out), bitmap(valid)


def gather_strings(body, dict_entries, dict_offsets, indices, num_indices, levels, max_level, offset_capacity, byte_capacity):
    """(the rows + 1 offsets, the bytes, the validity bitmap); Refused"""
    rows = num_indices if levels is None else len(levels)
    if rows + 1 > offset_capacity:
        raise Refused("more offsets than the capacity")
    valid = valid_rows(indices, num_indices, levels, max_level, dict_entries)
    for k in indices[:num_indices]:
        a, b = dict_offsets[k], dict_offsets[k + 1]
        if a < 0 or a > b or 4 * (k + 1) + b > len(body):
            raise Refused("an offset of the dictionary")
    total = sum(dict_offsets[k + 1] - dict_offsets[k] for k in indices[:num_indices])
    if total > byte_capacity or total > MAX_OFFSET:
        raise Refused("the bytes")
    offsets, out, j = [0], bytearray(), 0
    for v in valid:
        if v:
            k = indices[j]
            j += 1
            out += body[4 * (k + 1) + dict_offsets[k]:4 * (k + 1) + dict_offsets[k + 1]]
        offsets.append(len(out))
    return offsets, bytes(out), bitmap(valid)


def _padded(data, size):
    assert len(data) <= size
    return data + bytes([FILL]) * (size - len(data))


def _i32(values):
    return struct.pack("<%di" % len(values), *values)


# ---- an item of a call -------------------------------------------------------------------------------------------------
class Item:
    """kind INDEX: body, entries, capacity.  FIXED and STRINGS: body, dict_entries, indices, num_indices (the array has
    that many), levels (None: dense), max_level, and capacity, entry_bytes or dict_offsets, offset_capacity,
    byte_capacity."""

    def __init__(self, kind, name, **kw):
        self.kind, self.name = kind, name
        self.levels, self.max_level = None, 0
        self.__dict__.update(kw)
        self.body = bytes(self.body)
        if kind != INDEX:
            self.indices = list(self.indices)
            self.num_indices = kw.get("num_indices", len(self.indices))
            assert len(self.indices) == self.num_indices
            self.levels = None if self.levels is None else bytes(self.levels)
            self.rows = self.num_indices if self.levels is None else len(self.levels)

    def call(self):
        """what has to be the same in all items of one call"""
        if self.kind == INDEX:
            return (INDEX, 0, False)
        return (self.kind, self.entry_bytes if self.kind == FIXED else 0, self.levels is not None)

    def sizes(self):
        """the bytes of every output, as the drivers lay them out"""
        if self.kind == INDEX:
            return [4 * self.capacity]
        if self.kind == FIXED:
            return [self.capacity * self.entry_bytes, (self.rows + 7) // 8]
        return [4 * self.offset_capacity, self.byte_capacity, (self.rows + 7) // 8]

    def model(self):
        """(status, the count the call reports, every output: the whole of it, FILL where nothing is written)"""
        try:
            if self.kind == INDEX:
                offsets = index_dictionary(self.body, self.entries, self.capacity)
                got, count = [_i32(offsets)], self.entries
            elif self.kind == FIXED:
                got, count = list(gather(self.body, self.dict_entries, self.indices, self.num_indices, self.levels, self.max_level,
                                         self.capacity, self.entry_bytes)), 0
            else:
                offsets, data, valid = gather_strings(self.body, self.dict_entries, self.dict_offsets, self.indices, self.num_indices,
                                                      self.levels, self.max_level, self.offset_capacity, self.byte_capacity)
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
        words = [self.kind, put(self.body), len(self.body)]
        if self.kind == INDEX:
            return " ".join(str(w) for w in words + [self.entries, self.capacity])
        words.append(self.dict_entries)
        if self.kind == STRINGS:
            words += [put(_i32(self.dict_offsets)), len(self.dict_offsets)]
        words += [put(struct.pack("<%dI" % len(self.indices), *self.indices)), self.num_indices, int(self.levels is not None),
                  put(self.levels or b""), self.rows, self.max_level]
        words += [self.capacity, self.entry_bytes] if self.kind == FIXED else [self.offset_capacity, self.byte_capacity]
        return " ".join(str(w) for w in words)

    def but(self, name, **kw):
        fields = {k: v for k, v in self.__dict__.items() if k not in ("kind", "name", "rows")}
        fields.update(kw)
        if "indices" in kw and "num_indices" not in kw:
            fields["num_indices"] = len(kw["indices"])
        return Item(self.kind, name, **fields)


def byte_array_body(entries, behind=b""):
    return b"".join(struct.pack("<I", len(e)) + e for e in entries) + behind


def offsets_of(entries):
    out = [0]
    for e in entries:
        out.append(out[-1] + len(e))
    return out


# ---- the planned items -------------------------------------------------------------------------------------------------
ROWS = (0, 1, 7, 8, 9, 63, 64, 65, 128, 129)
ENTRY_BYTES = (1, 2, 3, 4, 5, 8, 12, 16, 64)


def _levels(rows, nulls):
    """a level of 1 but in the rows `nulls` says"""
    return bytes(0 if nulls(r) else 1 for r in range(rows))


def all_plans():
    rng = random.Random(29)
    plans = []
    blob = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    words = lambda n: [blob(rng.choice((0, 1, 2, 3, 5, 8, 13))) for _ in range(n)]

    # -- index_parquet_dictionary
    def index(name, entries, count=None, capacity=None, behind=b"", cut=0):
        body = byte_array_body(entries, behind)
        count = len(entries) if count is None else count
        plans.append(Item(INDEX, "index_" + name, body=body[:len(body) - cut], entries=count, capacity=count + 1 if capacity is None else capacity))
    for n in (0, 1, 2, 63, 64, 65, 128, 129, 200):
        index("%d_entries" % n, words(n))
        index("%d_entries_capacity_one_short" % n, words(n), capacity=n)
    index("all_empty", [b""] * 70)
    index("lengths_1_63_64_65_300", [blob(n) for n in (1, 63, 64, 65, 300, 0, 7)])
    index("bytes_behind_the_last_entry", words(9), behind=blob(11))
    index("bytes_behind_that_are_no_entry", words(9), behind=b"\xff\xff\xff")
    index("fewer_entries_than_the_body_holds", words(9), count=5)
    index("more_entries_than_the_body_holds", words(9), count=10)
    index("one_more_entry_behind_3_bytes", words(9), count=10, behind=b"\0\0\0")
    index("one_more_empty_entry", words(9), count=10, behind=b"\0\0\0\0")
    for cut in (1, 2, 3):
        index("cut_%d_inside_the_last_length_word" % cut, words(66) + [b""], cut=cut)
    index("cut_inside_the_last_entry", words(5) + [blob(9)], cut=1)
    index("cut_inside_an_entry_of_300", words(70) + [blob(300)], cut=299)
    index("nothing_of_1_entry", [], count=1)
    index("length_2_31", [], count=1, behind=struct.pack("<I", 1 << 31) + blob(40))
    index("length_2_32_less_1", words(3), count=4, behind=struct.pack("<I", 0xFFFFFFFF) + blob(40))
    index("length_one_above_the_body", words(3), count=4, behind=struct.pack("<I", 41) + blob(40))
    index("length_to_the_end_of_the_body", words(3), count=4, behind=struct.pack("<I", 40) + blob(40))
    index("no_capacity", [], capacity=0)

    # -- gather_parquet_dictionary
    def fixed(name, rows, entry_bytes, nulls=None, entries=37, **kw):
        body = blob(entries * entry_bytes)
        levels = None if nulls is None else _levels(rows, nulls)
        there = rows if levels is None else levels.count(1)
        item = Item(FIXED, "fixed_%s_e%d" % (name, entry_bytes), body=body, dict_entries=entries,
                    indices=[rng.randrange(entries) for _ in range(there)], levels=levels, max_level=1, capacity=rows,
                    entry_bytes=entry_bytes)
        plans.append(item.but(item.name, **kw) if kw else item)
        return plans[-1]
    for e in ENTRY_BYTES:
        for rows in ROWS:
            fixed("%d_rows_dense" % rows, rows, e)
            fixed("%d_rows_every_third_null" % rows, rows, e, nulls=lambda r: r % 3 == 1)
        fixed("all_valid", 129, e, nulls=lambda r: False)
        fixed("all_null", 129, e, nulls=lambda r: True)
        fixed("null_at_63_64_127", 129, e, nulls=lambda r: r in (63, 64, 127))
        fixed("valid_at_63_64_127", 129, e, nulls=lambda r: r not in (63, 64, 127))
        fixed("1_entry", 70, e, nulls=lambda r: r % 5 == 0, entries=1)
        it = fixed("capacity_one_short", 65, e, nulls=lambda r: r % 4 == 0, capacity=64)
        it = fixed("index_of_the_last_entry", 66, e, nulls=lambda r: r % 4 == 0)
        plans[-1] = it.but(it.name, indices=it.indices[:-1] + [it.dict_entries - 1])
        plans.append(it.but("fixed_index_of_the_entries_in_the_last_row_e%d" % e, indices=it.indices[:-1] + [it.dict_entries]))
        plans.append(it.but("fixed_index_of_the_entries_in_the_first_row_e%d" % e, indices=[it.dict_entries] + it.indices[1:]))
        plans.append(it.but("fixed_index_2_32_less_1_e%d" % e, indices=it.indices[:20] + [0xFFFFFFFF] + it.indices[21:]))
        plans.append(it.but("fixed_one_index_more_e%d" % e, indices=it.indices + [0]))
        plans.append(it.but("fixed_one_index_fewer_e%d" % e, indices=it.indices[:-1]))
        plans.append(it.but("fixed_no_index_e%d" % e, indices=[]))
        plans.append(it.but("fixed_dictionary_one_byte_short_e%d" % e, body=it.body[:-1]))
        plans.append(it.but("fixed_dictionary_with_bytes_behind_e%d" % e, body=it.body + blob(3)))
        plans.append(it.but("fixed_level_above_the_maximum_in_the_last_row_e%d" % e, levels=it.levels[:-1] + b"\2"))
        plans.append(it.but("fixed_level_above_the_maximum_e%d" % e, levels=it.levels[:7] + b"\xff" + it.levels[8:]))
        plans.append(it.but("fixed_no_entries_e%d" % e, dict_entries=0))
        dense = fixed("dense_index_of_the_entries_in_the_last_row", 129, e)
        plans[-1] = dense.but(dense.name, indices=dense.indices[:-1] + [dense.dict_entries])
        plans.append(dense.but("fixed_dense_capacity_one_short_e%d" % e, capacity=128))
        plans.append(dense.but("fixed_dense_capacity_to_spare_e%d" % e, capacity=140))
    deep = fixed("maximum_level_3", 130, 4, nulls=lambda r: False)
    plans[-1] = deep.but(deep.name, levels=bytes(r % 4 for r in range(130)), max_level=3, indices=deep.indices[:32])
    plans.append(plans[-1].but("fixed_maximum_level_3_a_level_of_4_e4", levels=bytes(r % 4 for r in range(129)) + b"\4"))
    plans.append(deep.but("fixed_maximum_level_300_e4", levels=bytes(130), max_level=300, indices=[]))
    plans.append(deep.but("fixed_all_null_and_no_dictionary_e4", levels=bytes(130), indices=[], dict_entries=0, body=b""))
    plans.append(deep.but("fixed_no_rows_and_no_dictionary_e4", levels=b"", indices=[], dict_entries=0, body=b"", capacity=0))

    # -- gather_parquet_dictionary_strings
    def strings(name, entries, picks, nulls=None, **kw):
        """`picks`: the entry of every row; those of the valid rows are the indices"""
        rows = len(picks)
        levels = None if nulls is None else _levels(rows, nulls)
        indices = [k for r, k in enumerate(picks) if levels is None or levels[r]]
        total = sum(len(entries[k]) for k in indices)
        item = Item(STRINGS, "strings_" + name, body=byte_array_body(entries), dict_entries=len(entries), dict_offsets=offsets_of(entries),
                    indices=indices, levels=levels, max_level=1, offset_capacity=rows + 1, byte_capacity=total)
        plans.append(item.but(item.name, **kw) if kw else item)
        return plans[-1]
    short = words(30)
    mixed = short + [blob(n) for n in (1, 63, 64, 65, 300)]
    third = lambda r: r % 3 == 1
    for rows in ROWS:
        strings("%d_rows_dense" % rows, short, [rng.randrange(30) for _ in range(rows)])
        strings("%d_rows_every_third_null" % rows, mixed, [rng.randrange(35) for _ in range(rows)], nulls=third)
    strings("all_empty", [b""] * 5, [r % 5 for r in range(129)], nulls=third)
    strings("all_empty_dense", [b""] * 5, [r % 5 for r in range(129)])
    strings("all_null", mixed, [34] * 129, nulls=lambda r: True)
    strings("all_valid", mixed, [r % 35 for r in range(129)], nulls=lambda r: False)
    strings("null_at_63_64_127", mixed, [r % 35 for r in range(129)], nulls=lambda r: r in (63, 64, 127))
    strings("a_step_of_empty_rows_between_two_of_bytes", mixed, [30 + r % 5 if r < 64 or r >= 128 else 0 for r in range(192)],
            body=byte_array_body([b""] + mixed[1:]), dict_offsets=offsets_of([b""] + mixed[1:]),
            byte_capacity=sum(len(mixed[30 + r % 5]) for r in range(192) if r < 64 or r >= 128))
    strings("300_bytes_in_rows_63_and_64", mixed, [34 if r in (63, 64) else r % 30 for r in range(130)])
    strings("300_bytes_in_every_row", mixed, [34] * 70, nulls=lambda r: r % 9 == 0)
    strings("lengths_1_63_64_65_300_in_turn", mixed, [30 + r % 5 for r in range(131)], nulls=lambda r: r % 11 == 3)
    strings("1_entry", [blob(65)], [0] * 70, nulls=third)
    it = strings("capacities_exact", mixed, [(11 * r) % 35 for r in range(131)], nulls=third)
    plans.append(it.but("strings_bytes_one_short", byte_capacity=it.byte_capacity - 1))
    plans.append(it.but("strings_bytes_to_spare", byte_capacity=it.byte_capacity + 9, offset_capacity=it.offset_capacity + 2))
    plans.append(it.but("strings_offsets_one_short", offset_capacity=it.offset_capacity - 1))
    plans.append(it.but("strings_no_byte_capacity", byte_capacity=0))
    plans.append(it.but("strings_index_of_the_entries_in_the_last_row", indices=it.indices[:-1] + [35]))
    plans.append(it.but("strings_index_of_the_last_entry_in_the_last_row", indices=it.indices[:-1] + [34],
                        byte_capacity=it.byte_capacity + 300))
    plans.append(it.but("strings_one_index_more", indices=it.indices + [0]))
    plans.append(it.but("strings_one_index_fewer", indices=it.indices[:-1]))
    plans.append(it.but("strings_level_above_the_maximum", levels=it.levels[:64] + b"\2" + it.levels[65:]))
    plans.append(it.but("strings_dictionary_of_0_entries", dict_entries=0))
    plans.append(it.but("strings_dictionary_of_0_entries_all_null", dict_entries=0, levels=bytes(131), indices=[], byte_capacity=0))
    dense = strings("dense_capacities_exact", mixed, [(11 * r) % 35 for r in range(131)])
    plans.append(dense.but("strings_dense_bytes_one_short", byte_capacity=dense.byte_capacity - 1))
    plans.append(dense.but("strings_dense_offsets_one_short", offset_capacity=dense.offset_capacity - 1))
    # the dictionary's offsets are not trusted: entry 17 is damaged; an item that uses it is refused, one that does not is not
    off = offsets_of(mixed)
    uses = [(11 * r) % 35 for r in range(131)]                  # (every entry, in valid rows)
    spares = [k if k not in (16, 17, 18) else 3 for k in uses]
    damage = {"decreases": off[:18] + [off[17] - 1] + off[19:], "negative": off[:17] + [-1] + off[18:],
              "lowest": off[:17] + [-(1 << 31)] + off[18:], "highest": off[:18] + [MAX_OFFSET] + off[19:]}
    for what, offsets in damage.items():
        strings("offset_%s_used" % what, mixed, uses, nulls=third, dict_offsets=offsets)
        strings("offset_%s_unused" % what, mixed, spares, nulls=third, dict_offsets=offsets)
    body = byte_array_body(mixed)
    strings("last_offset_one_byte_past_the_body_used", mixed, uses, nulls=third, dict_offsets=off[:-1] + [off[-1] + 1],
            byte_capacity=20000)
    strings("last_offset_at_the_end_of_the_body_used", mixed, uses, nulls=third, body=body + b"\x77", dict_offsets=off[:-1] + [off[-1] + 1],
            byte_capacity=20000)
    strings("body_one_byte_short_last_entry_used", mixed, uses, nulls=third, body=body[:-1])
    strings("body_one_byte_short_last_entry_unused", mixed, [k if k != 34 else 2 for k in uses], nulls=third, body=body[:-1])
    strings("no_body", mixed, uses, nulls=third, body=b"")
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
    """a data page of a fixture: `levels` and `index` parquet_hybridgen Plans (the levels of width 1 with the ones counted,
    the indices width-prefixed), the dictionary page's body and entries, and what the table pyarrow was given says the
    rows hold: want_values (entry_bytes each, zeros where null) or want_offsets and want_bytes, and want_validity"""

    def item(self):
        """the gather of the page, its levels and indices decoded by the restatement of decode_parquet_hybrid"""
        levels, _ = H.decode(self.levels.data, self.levels.form, 1, self.rows, self.rows, H.UCHAR)
        indices, _ = H.decode(self.index.data, H.WIDTH_PREFIXED, 0, self.non_null, self.non_null, H.UINT)
        common = dict(body=self.dictionary, dict_entries=self.dict_entries, indices=indices, levels=bytes(levels), max_level=1)
        if self.entry_bytes:
            return Item(FIXED, self.name, capacity=self.rows, entry_bytes=self.entry_bytes, **common)
        return Item(STRINGS, self.name, dict_offsets=index_dictionary(self.dictionary, self.dict_entries, self.dict_entries + 1),
                    offset_capacity=self.rows + 1, byte_capacity=len(self.want_bytes), **common)


def fixture_pages():
    pages = []
    for name in fixture_names():
        blob, manifest = load_fixture(name)
        form = H.LENGTH_PREFIXED if manifest["data_page_version"] == "1.0" else H.BARE
        cut = lambda where: blob[where[0]:where[0] + where[1]]
        for k, p in enumerate(manifest["pages"]):
            g = Page()
            g.name, g.version, g.column, g.entry_bytes = "%s_%d" % (name, k), name[:2], manifest["column"], manifest["entry_bytes"]
            g.dictionary, g.dict_entries = cut(manifest["dictionary"]), manifest["dictionary_entries"]
            g.rows, g.non_null = p["num_values"], p["non_null"]
            g.want_levels, g.want_validity = cut(p["expected_levels"]), cut(p["expected_validity"])
            g.levels = H.Plan(g.name + "_levels", cut(p["level_stream"]), g.rows, 1, form=form, element=H.UCHAR, match=1)
            g.index = H.Plan(g.name + "_indices", cut(p["index_stream"]), g.non_null, form=H.WIDTH_PREFIXED, element=H.UINT)
            if g.entry_bytes:
                g.want_values = cut(p["expected_values"])
            else:
                g.want_offsets = list(struct.unpack("<%di" % (g.rows + 1), cut(p["expected_offsets"])))
                g.want_bytes = cut(p["expected_bytes"])
            pages.append(g)
    return pages
