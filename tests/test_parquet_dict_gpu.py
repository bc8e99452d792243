"""A Parquet dictionary's entries gathered to rows (hipcomp/cascaded.hpp: index_parquet_dictionary,
gather_parquet_dictionary and gather_parquet_dictionary_strings of the Cascaded manager; INTEGRATION.md, "Parquet
dictionary entries gathered to rows in the Cascaded manager", has the contract), through tests/parquet_dict_driver.cpp, a
C++ program written against include/ and linked to libhipcomp.so.  The driver works through a list of cases per process,
each process under a timeout; it puts guard bytes on both sides of every output.

Fixtures: every page of tests/golden/parquet_dict/ (pyarrow's V1 and V2 pages of eight nullable dictionary-encoded
columns) gives the fixture's values, or its offsets and bytes, and its bitmap -- pinned to the table pyarrow was given.
Planned items: every one of parquet_dictgen's, alone and in one batch, gives what the restatement says; a refused item
leaves its outputs and guards untouched.  Isolation: in batches of 1, 3, 65 and 300 items with hostile items first, in the
middle and last, capacities exact and one short, every item's result is its one-item result.  Odd addresses:
dictionaries, validity arrays and string bytes 1, 3 and 7 bytes behind an aligned address, the other outputs at the
stated alignment and no better.  Each nullable array null in turn.  The chained use on V1 and V2 pages: levels, indices,
dictionary offsets and the gather with no host round trip between the calls."""
import os
import struct
import subprocess

import pytest

import parquet_dictgen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
FILL = bytes([G.FILL])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("parquet_dict") / "parquet_dict_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "parquet_dict_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


class Case:
    """the items of one call: one kind, one entry_bytes, all with levels or all dense"""

    def __init__(self, items, align=0, nulls=0, ones=0):
        assert len({p.call() for p in items}) == 1
        self.items, self.align, self.nulls, self.ones = items, align, nulls, ones
        self.kind, self.entry_bytes, self.has_levels = items[0].call()


def _run_cases(driver, tmp, cases, timeout=300):
    """name -> (per-item words, per-item outputs: the whole capacity of each)"""
    blob, lines = bytearray(), []
    for name, c in cases.items():
        lines.append("case %s %d %d %d %d %d %s %d" % (c.kind, c.entry_bytes, c.has_levels, c.align, c.nulls, c.ones, tmp / (name + ".out"),
                                                       len(c.items)))
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
        if c.nulls & 2 and p.kind != G.INDEX:
            want = want[:-1] + [FILL * len(want[-1])]
        assert w["guards"] == 1, ("bytes outside an output were written", p.name, w)
        assert w["status"] == status, (p.name, w)
        assert got == want, (p.name, "an output: a refused item's is untouched, an accepted one's is untouched behind what it writes")
        assert w["count"] == (-1 if c.nulls & 1 or p.kind == G.FIXED else count), (p.name, w)
        if c.ones:
            assert (w["one_status"], w["one_count"], w["eq_one"]) == (w["status"], w["count"], 1), (p.name, w)


def _by_call(items):
    groups = {}
    for p in items:
        groups.setdefault(p.call(), []).append(p)
    return groups


def _name(call):
    return "%s_e%d_l%d" % (call[0], call[1], call[2])


@pytest.fixture(scope="module")
def plans():
    return G.all_plans()


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


# ---- 1. the fixtures --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(driver, pages, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_dict_fixtures")
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
            if g.entry_bytes:
                assert outs == [g.want_values, g.want_validity], p.name
            else:
                assert outs[0] == struct.pack("<%di" % (g.rows + 1), *g.want_offsets) and outs[1] == g.want_bytes, p.name
                assert outs[2] == g.want_validity and w["count"] == len(g.want_bytes), p.name
            seen.add((g.version, g.column))
    assert len(want) >= 300 and len(seen) == 16
    assert {c.entry_bytes for c in cases.values()} == {0, 4, 5, 8, 12, 16}


# ---- 2. the planned items -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned(driver, plans, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_dict_planned")
    cases = {_name(call): Case(mine, ones=1) for call, mine in _by_call(plans).items()}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


CALLS = [(G.INDEX, 0), (G.STRINGS, 0)] + [(G.FIXED, e) for e in G.ENTRY_BYTES]


@pytest.mark.parametrize("kind,entry_bytes", CALLS)
def test_planned_items(planned, kind, entry_bytes):
    """in one batch and alone"""
    cases, results = planned
    names = [n for n, c in cases.items() if (c.kind, c.entry_bytes) == (kind, entry_bytes)]
    assert len(names) == (1 if kind == G.INDEX else 2), "dense and with levels"
    for name in names:
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


def test_planned_refusals(planned):
    cases, results = planned
    by_name = {p.name: (w, outs) for name, c in cases.items() for p, w, outs in zip(c.items, *results[name])}
    refused = ["index_0_entries_capacity_one_short", "index_65_entries_capacity_one_short", "index_more_entries_than_the_body_holds",
               "index_one_more_entry_behind_3_bytes", "index_cut_1_inside_the_last_length_word", "index_cut_3_inside_the_last_length_word",
               "index_cut_inside_the_last_entry", "index_cut_inside_an_entry_of_300", "index_nothing_of_1_entry", "index_length_2_31",
               "index_length_2_32_less_1", "index_length_one_above_the_body", "index_no_capacity",
               "strings_bytes_one_short", "strings_offsets_one_short", "strings_no_byte_capacity", "strings_index_of_the_entries_in_the_last_row",
               "strings_one_index_more", "strings_one_index_fewer", "strings_level_above_the_maximum", "strings_dictionary_of_0_entries",
               "strings_dense_bytes_one_short", "strings_dense_offsets_one_short", "strings_offset_decreases_used",
               "strings_offset_negative_used", "strings_offset_lowest_used", "strings_offset_highest_used",
               "strings_last_offset_one_byte_past_the_body_used", "strings_body_one_byte_short_last_entry_used", "strings_no_body",
               "fixed_maximum_level_3_a_level_of_4_e4"]
    accepted = ["index_0_entries", "index_all_empty", "index_lengths_1_63_64_65_300", "index_bytes_behind_the_last_entry",
                "index_bytes_behind_that_are_no_entry", "index_fewer_entries_than_the_body_holds", "index_one_more_empty_entry",
                "index_length_to_the_end_of_the_body", "strings_all_empty", "strings_all_null", "strings_null_at_63_64_127",
                "strings_a_step_of_empty_rows_between_two_of_bytes", "strings_300_bytes_in_rows_63_and_64", "strings_300_bytes_in_every_row",
                "strings_lengths_1_63_64_65_300_in_turn", "strings_capacities_exact", "strings_bytes_to_spare",
                "strings_index_of_the_last_entry_in_the_last_row", "strings_dictionary_of_0_entries_all_null", "strings_offset_decreases_unused",
                "strings_offset_negative_unused", "strings_offset_lowest_unused", "strings_offset_highest_unused",
                "strings_last_offset_at_the_end_of_the_body_used", "strings_body_one_byte_short_last_entry_unused",
                "fixed_maximum_level_3_e4", "fixed_maximum_level_300_e4", "fixed_all_null_and_no_dictionary_e4",
                "fixed_no_rows_and_no_dictionary_e4"]
    for e in G.ENTRY_BYTES:
        refused += [k % e for k in ("fixed_capacity_one_short_e%d", "fixed_index_of_the_entries_in_the_last_row_e%d",
                                    "fixed_index_of_the_entries_in_the_first_row_e%d", "fixed_index_2_32_less_1_e%d", "fixed_one_index_more_e%d",
                                    "fixed_one_index_fewer_e%d", "fixed_no_index_e%d", "fixed_dictionary_one_byte_short_e%d",
                                    "fixed_level_above_the_maximum_in_the_last_row_e%d", "fixed_level_above_the_maximum_e%d",
                                    "fixed_no_entries_e%d", "fixed_dense_index_of_the_entries_in_the_last_row_e%d",
                                    "fixed_dense_capacity_one_short_e%d")]
        accepted += [k % e for k in ("fixed_index_of_the_last_entry_e%d", "fixed_dictionary_with_bytes_behind_e%d", "fixed_all_valid_e%d",
                                     "fixed_all_null_e%d", "fixed_null_at_63_64_127_e%d", "fixed_valid_at_63_64_127_e%d", "fixed_1_entry_e%d",
                                     "fixed_dense_capacity_to_spare_e%d", "fixed_0_rows_dense_e%d", "fixed_129_rows_every_third_null_e%d")]
    for k in refused:
        w, outs = by_name[k]
        assert (w["status"], w["count"]) == (G.CANNOT_DECOMPRESS, -1 if k.startswith("fixed_") else 0), k
        assert all(set(o) <= {G.FILL} for o in outs), ("a refused item's output was written", k)
    for k in accepted:
        assert by_name[k][0]["status"] == G.SUCCESS, k


# ---- 3. isolation -------------------------------------------------------------------------------------------------
def _mixed(n, call, pool):
    """n items of one call: hostile ones first, in the middle, last and every fourth"""
    mine = _by_call(pool)[call]
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


ISOLATED = [(G.INDEX, 0, False), (G.FIXED, 4, True), (G.FIXED, 8, False), (G.FIXED, 5, True), (G.FIXED, 12, True), (G.STRINGS, 0, True),
            (G.STRINGS, 0, False)]
ISOLATION = [(n,) + call for n in (1, 3, 65, 300) for call in ISOLATED]


@pytest.fixture(scope="module")
def isolation(driver, plans, pages, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_dict_isolation")
    pool = plans + [g.item() for g in pages]
    cases = {"n%d_%s" % (key[0], _name(key[1:])): Case(_mixed(key[0], key[1:], pool), ones=1) for key in ISOLATION}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("n,kind,entry_bytes,has_levels", ISOLATION)
def test_isolation(isolation, n, kind, entry_bytes, has_levels):
    """the planned items hold capacities that are exact and one short"""
    cases, results = isolation
    name = "n%d_%s" % (n, _name((kind, entry_bytes, has_levels)))
    _check_case(cases[name], results[name])
    if n >= 65:
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}
        assert any("one_short" in p.name for p in cases[name].items)


# ---- 4. odd addresses, 5. null arrays -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(driver, plans, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_dict_shapes")
    cases = {}
    for align in (1, 3, 7):
        for call, mine in _by_call(plans).items():
            cases["align_%d_%s" % (align, _name(call))] = Case(mine, align=align)
    for nulls in (1, 2, 3):
        for call in ((G.INDEX, 0, False), (G.FIXED, 4, True), (G.FIXED, 3, False), (G.STRINGS, 0, True)):
            if call[0] != G.INDEX or nulls == 1:
                cases["nulls_%d_%s" % (nulls, _name(call))] = Case(_mixed(65, call, plans), nulls=nulls, ones=1)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("align", [1, 3, 7])
def test_odd_addresses(shapes, align):
    cases, results = shapes
    names = [k for k in cases if k.startswith("align_%d_" % align)]
    assert len(names) == 2 * len(G.ENTRY_BYTES) + 3
    for name in names:
        _check_case(cases[name], results[name])
        assert any(w["status"] == G.SUCCESS for w in results[name][0])


@pytest.mark.parametrize("nulls", [1, 2, 3])
def test_null_arrays(shapes, nulls):
    """1: no count array (device_entry_counts, device_out_byte_counts); 2: no device_validity_ptrs; 3: neither.  The
    levels' three arrays are null together in every dense case of the other tests."""
    cases, results = shapes
    names = [k for k in cases if k.startswith("nulls_%d_" % nulls)]
    assert len(names) == (4 if nulls == 1 else 3)
    for name in names:
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


# ---- 6. the chained use ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", ["v1", "v2"])
@pytest.mark.parametrize("column", ["int32", "int64", "int96", "decimal5", "strings"])
def test_levels_indices_dictionary_and_gather_without_a_host_round_trip(driver, pages, version, column, tmp_path):
    """The levels with the count of the maximum level; that device array as the indices' num_values and as the gather's
    device_num_indices; for strings the index call's entry counts as the gather's device_dict_entries.  Every third
    page of the strings names a dictionary cut by one byte: the index call refuses it, its entry count is 0, and the
    gather refuses exactly the pages that have an index into it -- a page that is wholly null has none."""
    mine = [g for g in pages if g.version == version and g.column == column]
    assert len(mine) >= 4
    entry_bytes = mine[0].entry_bytes
    damaged = [entry_bytes == 0 and k % 3 == 1 for k in range(len(mine))]
    blob, lines = bytearray(mine[0].dictionary), []
    for g, cut in zip(mine, damaged):
        lines.append("%d %d %d %d %d 0 %d %d" % (len(blob), len(g.levels.data), len(blob) + len(g.levels.data), len(g.index.data), g.rows,
                                                  len(g.dictionary) - cut, g.dict_entries))
        blob += g.levels.data + g.index.data
    (tmp_path / "pool.bin").write_bytes(bytes(blob))
    (tmp_path / "chain.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "chain", str(tmp_path / "pool.bin"), str(tmp_path / "chain.list"), str(tmp_path / "chain.out"),
                        str(mine[0].levels.form), str(entry_bytes)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, got, pos = _words(r.stdout), (tmp_path / "chain.out").read_bytes(), 0
    assert len(words) == len(mine)
    refused = 0
    for g, w, cut in zip(mine, words, damaged):
        def take(size):
            nonlocal pos
            pos += size
            return got[pos - size:pos]
        assert (w["levels_status"], w["indices_status"], w["non_null"], w["guards"]) == (G.SUCCESS, G.SUCCESS, g.non_null, 1), g.name
        assert take(g.rows) == g.want_levels, g.name
        ok = not (cut and g.non_null)
        assert w["status"] == (G.SUCCESS if ok else G.CANNOT_DECOMPRESS), g.name
        refused += not ok
        if entry_bytes:
            values, validity = take(g.rows * entry_bytes), take((g.rows + 7) // 8)
            assert (values, validity) == (g.want_values, g.want_validity), g.name
            continue
        assert (w["dictionary_status"], w["entries"]) == ((G.CANNOT_DECOMPRESS, 0) if cut else (G.SUCCESS, g.dict_entries)), g.name
        offsets, data, validity = take(4 * (g.rows + 1)), take(400 * g.rows), take((g.rows + 7) // 8)
        if ok:
            assert offsets == struct.pack("<%di" % (g.rows + 1), *g.want_offsets) and w["count"] == len(g.want_bytes), g.name
            assert data == g.want_bytes + FILL * (len(data) - len(g.want_bytes)) and validity == g.want_validity, g.name
        else:
            assert w["count"] == 0 and set(offsets + data + validity) == {G.FILL}, ("a refused page's output was written", g.name)
    assert pos == len(got)
    assert refused >= 3 if entry_bytes == 0 else refused == 0
    if entry_bytes == 0:
        assert any(cut and not g.non_null for g, cut in zip(mine, damaged)), "a wholly null page on the damaged dictionary"


# ---- 7. what throws before a launch -----------------------------------------------------------------------------------
def test_misuse(driver):
    r = subprocess.run([driver, "misuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    w = _words(r.stdout)[0]
    assert w["threw"] == 7 + 14 + 13, ("index: more than 2^20 items and six null arrays; gather: more than 2^20 items, entry_bytes of 0 and "
                                       "65, eight null arrays, the levels' arrays apart three ways; strings: more than 2^20 items, eleven "
                                       "null arrays, the levels alone")
    assert w["nothing_launched"] == 1
    assert w["quiet"] == 3 and w["worked"] == 3, "no items: nothing to do; and the calls as they are meant"
