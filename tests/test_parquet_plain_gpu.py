"""A Parquet page's dense values placed in rows (hipcomp/cascaded.hpp: place_parquet_values, place_parquet_booleans and
place_parquet_strings of the Cascaded manager; INTEGRATION.md, "PLAIN Parquet values placed in rows in the Cascaded
manager", has the contract), through tests/parquet_plain_driver.cpp, a C++ program written against include/ and linked
to libhipcomp.so.  The driver works through a list of cases per process, each process under a timeout; it puts guard
bytes on both sides of every output.

Fixtures: every page of tests/golden/parquet_plain/ (pyarrow's V1 and V2 pages of nullable PLAIN, BYTE_STREAM_SPLIT,
DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY columns) gives the fixture's values, bits, or offsets and bytes, and its
bitmap -- pinned to the table pyarrow was given.  Planned items: every one of parquet_plaingen's, alone and in one batch,
gives what the restatement says; a refused item leaves its outputs and guards untouched.  Isolation: in batches of 1, 3,
65 and 300 items with refused items first, in the middle and last, capacities exact and one short, every item's result
is its one-item result.  Odd addresses: sources, bitmaps and string bytes 1, 3 and 7 bytes behind an aligned address, the
other outputs at the stated alignment and no better.  Each nullable array null in turn.  The chained use on V1 and V2
pages: the levels, then the earlier call the encoding needs, then the place call, with no host round trip between."""
import os
import struct
import subprocess

import pytest

import parquet_deltagen as D
import parquet_dictgen as DG
import parquet_plaingen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
FILL = bytes([G.FILL])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("parquet_plain") / "parquet_plain_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "parquet_plain_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


class Case:
    """the items of one call: one kind, one value_bytes, one layout, all with levels or all dense"""

    def __init__(self, items, align=0, nulls=0, ones=0):
        assert len({p.call() for p in items}) == 1
        self.items, self.align, self.nulls, self.ones = items, align, nulls, ones
        self.kind, self.value_bytes, self.layout, self.has_levels = items[0].call()


def _run_cases(driver, tmp, cases, timeout=300):
    """name -> (per-item words, per-item outputs: the whole capacity of each)"""
    blob, lines = bytearray(), []
    for name, c in cases.items():
        lines.append("case %s %d %d %d %d %d %d %s %d" % (c.kind, c.value_bytes, c.layout, c.has_levels, c.align, c.nulls, c.ones,
                                                          tmp / (name + ".out"), len(c.items)))
        lines += [p.line(blob) for p in c.items]
    (tmp / "pool.bin").write_bytes(bytes(blob))
    (tmp / "cases.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "batch", str(tmp / "pool.bin"), str(tmp / "cases.list")], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, results, at = _words(r.stdout), {}, 0
    for name, c in cases.items():
        items, case = words[at:at + len(c.items)], words[at + len(c.items)]
        at += len(c.items) + 1
        assert [w["item"] for w in items] == list(range(len(c.items))) and case == {"case": len(c.items)}
        got, outs, pos = (tmp / (name + ".out")).read_bytes(), [], 0
        for p in c.items:
            mine = []
            for size in p.sizes():
                mine.append(got[pos:pos + size])
                pos += size
            outs.append(mine)
        assert pos == len(got)
        results[name] = (items, outs)
    assert at == len(words)
    return results


_MODEL = {}


def _model(p):
    if id(p) not in _MODEL:
        _MODEL[id(p)] = (p, p.model())
    return _MODEL[id(p)][1]


def _check_case(c, result):
    items, outs = result
    for p, w, got in zip(c.items, items, outs):
        status, count, want = _model(p)
        if c.nulls & 2:
            want = want[:-1] + [FILL * len(want[-1])]
        assert w["guards"] == 1, ("bytes outside an output were written", p.name, w)
        assert w["status"] == status, (p.name, w)
        assert got == want, (p.name, "an output: a refused item's is untouched, an accepted one's is untouched behind what it writes")
        assert w["count"] == (-1 if c.nulls & 1 or p.kind != G.STRINGS else count), (p.name, w)
        if c.ones:
            assert (w["one_status"], w["one_count"], w["eq_one"]) == (w["status"], w["count"], 1), (p.name, w)


def _by_call(items):
    groups = {}
    for p in items:
        groups.setdefault(p.call(), []).append(p)
    return groups


def _name(call):
    return "%s_w%d_y%d_l%d" % call


@pytest.fixture(scope="module")
def plans():
    return G.all_plans()


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


# ---- 1. the fixtures --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(driver, pages, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_plain_fixtures")
    items = [g.item() for g in pages]
    cases = {_name(call): Case(mine) for call, mine in _by_call(items).items()}
    return cases, _run_cases(driver, tmp, cases), dict(zip((p.name for p in items), pages))


def test_fixtures(fixtures):
    cases, results, want = fixtures
    seen = set()
    for name, c in cases.items():
        _check_case(c, results[name])
        for p, w, outs in zip(c.items, *results[name]):
            g = want[p.name]
            assert w["status"] == G.SUCCESS, p.name
            if g.encoding == "boolean":
                assert outs == [g.want_bits, g.want_validity], p.name
            elif p.kind == G.VALUES:
                assert outs == [g.want_values, g.want_validity], p.name
            else:
                assert outs[0] == struct.pack("<%di" % (g.rows + 1), *g.want_offsets) and outs[1] == g.want_bytes, p.name
                assert outs[2] == g.want_validity and w["count"] == len(g.want_bytes), p.name
            seen.add((g.version, g.column, g.encoding))
    assert len(want) >= 300 and len(seen) == 26
    assert {(c.kind, c.value_bytes, c.layout) for c in cases.values()} == {
        (G.VALUES, 4, G.PLAIN), (G.VALUES, 8, G.PLAIN), (G.VALUES, 4, G.SPLIT), (G.VALUES, 8, G.SPLIT), (G.VALUES, 12, G.PLAIN),
        (G.VALUES, 5, G.PLAIN), (G.VALUES, 16, G.PLAIN), (G.BOOLEANS, 0, 0), (G.STRINGS, 0, G.LENGTH_PREFIXED), (G.STRINGS, 0, G.PACKED)}


# ---- 2. the planned items -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned(driver, plans, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_plain_planned")
    cases = {_name(call): Case(mine, ones=1) for call, mine in _by_call(plans).items()}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


CALLS = [(G.BOOLEANS, 0, 0), (G.STRINGS, 0, G.LENGTH_PREFIXED), (G.STRINGS, 0, G.PACKED)]
CALLS += [(G.VALUES, w, layout) for w in G.VALUE_BYTES for layout in (G.PLAIN, G.SPLIT)]


@pytest.mark.parametrize("kind,value_bytes,layout", CALLS)
def test_planned_items(planned, kind, value_bytes, layout):
    """in one batch and alone"""
    cases, results = planned
    names = [n for n, c in cases.items() if (c.kind, c.value_bytes, c.layout) == (kind, value_bytes, layout)]
    assert len(names) == 2, "dense and with levels"
    for name in names:
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


def test_planned_refusals(planned):
    """one planned refusal for every rule, each in the last step of its item: no byte of its outputs is written"""
    cases, results = planned
    by_name = {p.name: (w, outs) for name, c in cases.items() for p, w, outs in zip(c.items, *results[name])}
    rules = ["capacity_one_short", "source_one_byte_short", "start_one_above_the_bytes", "level_above_the_maximum_in_the_last_row",
             "one_valid_row_more", "one_valid_row_fewer", "no_values_and_a_valid_row"]
    dense = ["dense_capacity_one_short", "dense_source_one_byte_short", "dense_start_one_above_the_bytes"]
    refused = ["booleans_" + r for r in rules + dense + ["seven_values_more", "dense_eight_values_more"]]
    accepted = ["booleans_every_fourth_null", "booleans_capacity_to_spare_and_bytes_behind", "booleans_all_bits_set", "booleans_no_bit_set",
                "booleans_start_at_the_end_all_null", "booleans_dense_set_bits_behind_the_values", "booleans_130_rows_all_null",
                "values_maximum_level_3_plain_w4", "values_maximum_level_300_plain_w4", "values_no_rows_and_no_source_plain_w4",
                "values_all_null_and_no_source_plain_w4", "strings_offsets_from_7_packed"]
    refused.append("values_maximum_level_3_a_level_of_4_plain_w4")
    for layout in ("plain", "split"):
        for w in G.VALUE_BYTES:
            tail = "_%s_w%d" % (layout, w)
            refused += ["values_%s%s" % (r, tail) for r in rules + dense + ["one_value_more", "one_value_fewer", "dense_one_value_more"]]
            accepted += ["values_%s%s" % (r, tail) for r in ("every_fourth_null", "bytes_behind_the_values", "start_at_the_end_all_null",
                                                              "dense_one_value_fewer", "130_rows_last_row_alone_valid",
                                                              "130_rows_last_row_alone_null", "0_rows_dense", "1003_rows_alternating")]
    for layout in ("prefixed", "packed"):
        tail = "_" + layout
        refused += ["strings_%s%s" % (r, tail) for r in rules + [
            "bytes_one_short", "no_byte_capacity", "one_value_fewer", "one_value_more", "the_last_offset_falls", "an_offset_falls",
            "a_negative_offset", "the_lowest_offset_last", "the_last_end_one_past_the_body", "the_highest_offset_last", "a_byte_total_of_2_31",
            "no_body", "dense_bytes_one_short", "dense_offsets_one_short", "dense_source_one_byte_short", "dense_start_one_above_the_bytes"]]
        accepted += ["strings_%s%s" % (r, tail) for r in (
            "every_fourth_null", "capacities_to_spare_and_bytes_behind", "the_last_end_at_the_end_of_the_body", "start_at_the_end_all_null",
            "all_null_and_no_offsets", "dense_no_values_and_no_offsets", "all_empty", "a_step_of_empty_rows_between_two_of_bytes",
            "300_bytes_in_rows_63_and_64", "130_rows_all_null", "1003_rows_alternating")]
    for k in refused:
        w, outs = by_name[k]
        assert (w["status"], w["count"]) == (G.CANNOT_DECOMPRESS, 0 if k.startswith("strings_") else -1), k
        assert all(set(o) <= {G.FILL} for o in outs), ("a refused item's output was written", k)
    for k in accepted:
        assert by_name[k][0]["status"] == G.SUCCESS, k


# ---- 3. isolation -------------------------------------------------------------------------------------------------
def _mixed(n, call, pool, no_starts=False):
    """n items of one call: refused ones first, in the middle, last and every fourth"""
    mine = [p for p in _by_call(pool)[call] if not (no_starts and p.start)]
    good = [p for p in mine if _model(p)[0] == G.SUCCESS]
    hostile = [p for p in mine if _model(p)[0] != G.SUCCESS]
    items, used = [], 0
    for i in range(n):
        if n > 1 and (i in (0, n // 2, n - 1) or i % 4 == 1):
            items.append(hostile[used % len(hostile)])
            used += 1
        else:
            items.append(good[(7 * i + 3) % len(good)])
    return items


ISOLATED = [(G.VALUES, 4, G.PLAIN, True), (G.VALUES, 8, G.SPLIT, False), (G.VALUES, 5, G.PLAIN, True), (G.VALUES, 12, G.SPLIT, True),
            (G.BOOLEANS, 0, 0, True), (G.STRINGS, 0, G.LENGTH_PREFIXED, True), (G.STRINGS, 0, G.PACKED, True), (G.STRINGS, 0, G.PACKED, False)]
ISOLATION = [(n,) + call for n in (1, 3, 65, 300) for call in ISOLATED]


@pytest.fixture(scope="module")
def isolation(driver, plans, pages, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_plain_isolation")
    pool = plans + [g.item() for g in pages]
    cases = {"n%d_%s" % (key[0], _name(key[1:])): Case(_mixed(key[0], key[1:], pool), ones=1) for key in ISOLATION}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("n,kind,value_bytes,layout,has_levels", ISOLATION)
def test_isolation(isolation, n, kind, value_bytes, layout, has_levels):
    """the planned items hold capacities that are exact and one short"""
    cases, results = isolation
    name = "n%d_%s" % (n, _name((kind, value_bytes, layout, has_levels)))
    _check_case(cases[name], results[name])
    if n >= 65:
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}
        assert any("one_short" in p.name for p in cases[name].items)


# ---- 4. odd addresses, 5. null arrays -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(driver, plans, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_plain_shapes")
    cases = {}
    for align in (1, 3, 7):
        for call, mine in _by_call(plans).items():
            cases["align_%d_%s" % (align, _name(call))] = Case(mine, align=align)
    for nulls in (1, 2, 3, 4, 7):
        for call in ((G.VALUES, 4, G.PLAIN, True), (G.VALUES, 3, G.SPLIT, False), (G.BOOLEANS, 0, 0, True), (G.STRINGS, 0, G.PACKED, True),
                     (G.STRINGS, 0, G.LENGTH_PREFIXED, False)):
            if call[0] == G.STRINGS or not nulls & 1 or nulls == 7:
                cases["nulls_%d_%s" % (nulls, _name(call))] = Case(_mixed(65, call, plans, no_starts=nulls & 4), nulls=nulls, ones=1)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("align", [1, 3, 7])
def test_odd_addresses(shapes, align):
    cases, results = shapes
    names = [k for k in cases if k.startswith("align_%d_" % align)]
    assert len(names) == 2 * (2 * len(G.VALUE_BYTES) + 3)
    for name in names:
        _check_case(cases[name], results[name])
        assert any(w["status"] == G.SUCCESS for w in results[name][0])


@pytest.mark.parametrize("nulls", [1, 2, 3, 4, 7])
def test_null_arrays(shapes, nulls):
    """1: no count array (device_out_byte_counts); 2: no device_validity_ptrs; 4: no device_value_starts; 3 and 7: none of
    them.  The levels' three arrays are null together in every dense case of the other tests."""
    cases, results = shapes
    names = [k for k in cases if k.startswith("nulls_%d_" % nulls)]
    assert len(names) == (2 if nulls in (1, 3) else 5)
    for name in names:
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


# ---- 6. the chained use ---------------------------------------------------------------------------------------------
CHAINS = [("int32", "plain"), ("double", "split"), ("int96", "plain"), ("decimal5", "plain"), ("boolean", "boolean"), ("delta", "delta"),
          ("strings", "prefixed"), ("strings", "packed")]


@pytest.mark.parametrize("version", ["v1", "v2"])
@pytest.mark.parametrize("column,encoding", CHAINS)
def test_levels_the_earlier_call_and_the_place_call_without_a_host_round_trip(driver, pages, version, column, encoding, tmp_path):
    """The levels with the count of the maximum level; that device array as the num_values of what follows.  Fixed-width
    values and booleans: a V1 page is handed over whole, the levels' consumed bytes as device_value_starts.  delta:
    decode_parquet_delta's values and value counts into place_parquet_values.  Strings: index_parquet_dictionary's
    offsets and entry counts, or decode_parquet_delta(Offsets)'s offsets, value counts and consumed bytes, into
    place_parquet_strings; every third page's values section is cut by one byte, the earlier call refuses it, its count
    is 0, and the place call refuses exactly the pages that have a valid row -- a page that is wholly null has none."""
    mine = [g for g in pages if (g.version, g.column, g.encoding) == (version, column, encoding)]
    assert len(mine) >= 4
    strings = column == "strings"
    kind = {"boolean": "B", "delta": "D", "prefixed": "S", "packed": "S"}.get(encoding, "V")
    layout = {"split": G.SPLIT, "packed": G.PACKED}.get(encoding, 0)
    damaged = [strings and k % 3 == 1 and len(g.values) > 0 for k, g in enumerate(mine)]   # (an all-null PLAIN page has no section)
    blob, lines = bytearray(), []
    for g, cut in zip(mine, damaged):
        lines.append("%d %d %d %d %d" % (len(blob), len(g.page), len(g.levels.data), g.rows, cut))
        blob += g.page
    (tmp_path / "pool.bin").write_bytes(bytes(blob))
    (tmp_path / "chain.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "chain", str(tmp_path / "pool.bin"), str(tmp_path / "chain.list"), str(tmp_path / "chain.out"),
                        str(mine[0].levels.form), kind, str(mine[0].value_bytes), str(layout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, got, pos = _words(r.stdout), (tmp_path / "chain.out").read_bytes(), 0
    assert len(words) == len(mine)
    refused = 0
    for g, w, cut in zip(mine, words, damaged):
        def take(size):
            nonlocal pos
            pos += size
            return got[pos - size:pos]
        assert (w["levels_status"], w["non_null"], w["guards"]) == (G.SUCCESS, g.non_null, 1), g.name
        assert take(g.rows) == g.want_levels, g.name
        if not strings:
            assert w["status"] == G.SUCCESS, g.name
            if kind == "D":
                assert (w["mid_status"], w["mid_count"]) == (G.SUCCESS, g.non_null), g.name
            if kind == "B":
                assert (take((g.rows + 7) // 8), take((g.rows + 7) // 8)) == (g.want_bits, g.want_validity), g.name
            else:
                assert (take(g.rows * g.value_bytes), take((g.rows + 7) // 8)) == (g.want_values, g.want_validity), g.name
            continue
        # what the earlier call makes of the cut section, by its restatement
        section = g.values[:len(g.values) - cut]
        if encoding == "prefixed":
            try:
                DG.index_dictionary(section, g.non_null, g.rows + 1)
                earlier = (G.SUCCESS, g.non_null)
            except DG.Refused:
                earlier = (G.CANNOT_DECOMPRESS, 0)
        else:
            status, _, _, count = D.model(section, g.non_null, g.rows + 1, D.OFFSETS, D.INT)
            earlier = (status, count)
        assert (w["mid_status"], w["mid_count"]) == earlier, g.name
        assert not cut or earlier == (G.CANNOT_DECOMPRESS, 0), g.name
        ok = earlier[0] == G.SUCCESS or g.non_null == 0
        assert w["status"] == (G.SUCCESS if ok else G.CANNOT_DECOMPRESS), g.name
        refused += not ok
        offsets, data, validity = take(4 * (g.rows + 1)), take(400 * g.rows), take((g.rows + 7) // 8)
        if ok:
            assert offsets == struct.pack("<%di" % (g.rows + 1), *g.want_offsets) and w["count"] == len(g.want_bytes), g.name
            assert data == g.want_bytes + FILL * (len(data) - len(g.want_bytes)) and validity == g.want_validity, g.name
        else:
            assert w["count"] == 0 and set(offsets + data + validity) == {G.FILL}, ("a refused page's output was written", g.name)
    assert pos == len(got)
    assert refused >= 3 if strings else refused == 0
    if encoding == "packed":
        assert any(cut and not g.non_null for g, cut in zip(mine, damaged)), "a wholly null page with a cut section"


# ---- 7. what throws before a launch -----------------------------------------------------------------------------------
def test_misuse(driver):
    r = subprocess.run([driver, "misuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    w = _words(r.stdout)[0]
    assert w["threw"] == 13 + 10 + 14, ("values: more than 2^20 items, value_bytes of 0 and 65, an unknown layout, six null arrays, the levels' "
                                        "arrays apart three ways; booleans: more than 2^20 items, six null arrays, the levels' arrays apart "
                                        "three ways; strings: more than 2^20 items, an unknown layout, nine null arrays, the levels' arrays "
                                        "apart three ways")
    assert w["nothing_launched"] == 1
    assert w["quiet"] == 3 and w["worked"] == 4, "no items: nothing to do; and the calls as they are meant"
