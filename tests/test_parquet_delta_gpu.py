"""Batches of Parquet DELTA_BINARY_PACKED streams in one call (hipcomp/cascaded.hpp: decode_parquet_delta of the Cascaded
manager; INTEGRATION.md, "Parquet DELTA_BINARY_PACKED values and string offsets in the Cascaded manager", has the
contract), through tests/parquet_delta_driver.cpp, a C++ program written against include/ and linked to libhipcomp.so.
The driver works through a list of cases per process, each process under a timeout; it puts guard bytes on both sides of
every output.

Fixtures: every value stream of tests/golden/parquet_delta/ (pyarrow's V1 and V2 pages of five nullable columns) gives the
fixture's values, or its offsets with the strings' bytes behind the consumed bytes -- pinned to the table pyarrow was
given.  Planned streams: every one of parquet_deltagen's, alone and in one batch, gives what the restatement says; a
refused item leaves its output and guards untouched.  Isolation: in batches of 1, 3, 65 and 300 items with hostile items
first, in the middle and last, capacities exact and one short, every item's result is its one-item result.  Odd
addresses: streams 1, 3 and 7 bytes behind an aligned address.  Each nullable array null in turn.  The chained use on V1
and V2 pages: the levels' match counts are the delta call's device_num_values, with no host round trip between the calls."""
import os
import struct
import subprocess

import pytest

import parquet_deltagen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
CALLS = [(output, element) for output in (G.VALUES, G.OFFSETS) for element in (G.INT, G.LONGLONG)]
FILL = 0xA5


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("parquet_delta") / "parquet_delta_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "parquet_delta_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


class Case:
    """items of one output and one element type, all with a wanted count or all without (a call has one of each)"""

    def __init__(self, items, align=0, nulls=0, ones=0):
        assert len({(p.output, p.element, p.wanted is None) for p in items}) == 1
        self.items, self.output, self.element, self.counted = items, items[0].output, items[0].element, items[0].wanted is not None
        self.align, self.nulls, self.ones = align, nulls, ones


def _run_cases(driver, tmp, cases, timeout=300):
    """name -> (per-item words, per-item output bytes: the whole capacity)"""
    blob, lines = bytearray(), []
    for name, c in cases.items():
        lines.append("case %d %d %d %d %d %d %s %d" % (c.output, c.element, c.align, c.nulls, c.counted, c.ones, tmp / (name + ".out"),
                                                       len(c.items)))
        for p in c.items:
            lines.append("%s %d %d %d %d" % (tmp / "pool.bin", len(blob), len(p.data), p.wanted or 0, p.capacity()))
            blob += p.data
    (tmp / "pool.bin").write_bytes(bytes(blob))
    (tmp / "cases.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "batch", str(tmp / "cases.list")], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, results, at = _words(r.stdout), {}, 0
    for name, c in cases.items():
        items, case = words[at:at + len(c.items)], words[at + len(c.items)]
        at += len(c.items) + 1
        assert [w["item"] for w in items] == list(range(len(c.items))) and case == {"case": len(c.items)}
        got, outs, pos = (tmp / (name + ".out")).read_bytes(), [], 0
        for p in c.items:
            outs.append(got[pos:pos + p.capacity() * c.element])
            pos += p.capacity() * c.element
        assert pos == len(got)
        results[name] = (items, outs)
    assert at == len(words)
    return results


_MODEL = {}


def _model(p):
    key = (p.data, p.wanted, p.capacity(), p.output, p.element)
    if key not in _MODEL:
        _MODEL[key] = p.model()
    return _MODEL[key]


def _check_case(c, result):
    items, outs = result
    for p, w, out in zip(c.items, items, outs):
        status, want, consumed, count = _model(p)
        assert w["guards"] == 1, ("bytes outside the output were written", p.name, w)
        assert w["status"] == status, (p.name, w)
        assert out[:len(want)] == want, (p.name, "the elements")
        assert out[len(want):] == bytes([FILL]) * (len(out) - len(want)), ("elements behind the item's were written", p.name)
        if not c.nulls & 1:
            assert w["count"] == count, (p.name, w)
        if not c.nulls & 2:
            assert w["consumed"] == consumed, (p.name, w)
        if status != G.SUCCESS:
            assert w["untouched"] == 1, ("a refused item's output was written", p.name, w)
        if c.ones:
            assert w["one_status"] == w["status"] and w["eq_one"] == 1, (p.name, w)
            assert (w["one_consumed"], w["one_count"]) == (w["consumed"], w["count"]), (p.name, w)


def _by_call(plans):
    """{(output, element, counted): the plans of it}"""
    groups = {}
    for p in plans:
        groups.setdefault((p.output, p.element, p.wanted is not None), []).append(p)
    return groups


@pytest.fixture(scope="module")
def plans():
    return G.all_plans()


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


# ---- 1. the fixtures --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(driver, pages, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_delta_fixtures")
    cases = {"o%d_e%d_c%d" % key: Case(items) for key, items in _by_call([g.plan for g in pages]).items()}
    return cases, _run_cases(driver, tmp, cases)


def test_fixtures(fixtures, pages):
    cases, results = fixtures
    want = {g.name: g for g in pages}
    seen = 0
    for name, c in cases.items():
        _check_case(c, results[name])
        for p, w, out in zip(c.items, *results[name]):
            g = want[p.name]
            assert w["status"] == G.SUCCESS and w["count"] == p.wanted, p.name
            assert list(struct.unpack_from("<%d%s" % (len(g.want), G.LETTER[p.element]), out)) == g.want, p.name
            if g.want_bytes is None:
                assert w["consumed"] == len(p.data), p.name
            else:
                strings = p.data[w["consumed"]:]
                assert [strings[a:b] for a, b in zip(g.want, g.want[1:])] == [g.want_bytes[a:b] for a, b in zip(g.want, g.want[1:])]
                assert strings == g.want_bytes, p.name
            seen += 1
    assert seen == len(pages) >= 50
    assert {(c.output, c.element) for c in cases.values()} == {(G.VALUES, G.INT), (G.VALUES, G.LONGLONG), (G.OFFSETS, G.INT)}


# ---- 2. the planned streams -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned(driver, plans, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_delta_planned")
    cases = {"o%d_e%d_c%d" % key: Case(items, ones=1) for key, items in _by_call(plans).items()}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("output,element", CALLS)
def test_planned_streams(planned, output, element):
    """in one batch and alone"""
    cases, results = planned
    for counted in (0, 1):
        name = "o%d_e%d_c%d" % (output, element, counted)
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


def test_planned_refusals(planned):
    cases, results = planned
    by_name = {p.name: w for name, c in cases.items() for p, w in zip(c.items, results[name][0])}
    for k in ("width_33_128_4_e4", "width_65_128_4_e8", "width_255_384_4_e8", "width_33_in_one_miniblock_e4", "lengths_width_33_e4",
              "block_size_of_11_bytes_e4", "first_tenth_byte_2_e8", "block_size_2_32_e8", "miniblocks_2_32_e4", "total_2_32_e8",
              "block_size_0_e4", "block_size_64_e8", "block_size_192_e4", "miniblocks_0_e8", "miniblocks_3_e4", "miniblocks_8_of_16_e8",
              "miniblocks_8_of_48_e4", "min_delta_of_11_bytes", "min_delta_tenth_byte_2", "header_alone_0_first_cut_o0_e4",
              "header_alone_1_first_too_long_o1_e8", "header_alone_1_negative_o1_e4", "cut_at_0_o0_e4", "cut_at_1_o1_e8",
              "wanted_295_of_296_o0_e4", "wanted_297_of_296_o1_e8", "wanted_0_of_296_o0_e8", "capacity_one_short_o0_e4",
              "capacity_of_the_total_o1_e4", "unneeded_width_byte_cut", "negative_length_at_0_offsets_e4", "negative_length_at_64_offsets_e8",
              "negative_length_at_200_offsets_e4", "lowest_length_offsets_e8", "sum_2_31_offsets_e4", "sum_2_31_behind_a_block_offsets_e8",
              "sum_one_above_the_bytes_behind_offsets_e4", "sum_one_above_the_bytes_behind_offsets_e8"):
        w = by_name[k]
        assert (w["status"], w["consumed"], w["count"], w["untouched"]) == (G.CANNOT_DECOMPRESS, 0, 0, 1), k
    for k in ("width_32_128_4_e4", "width_64_384_4_e8", "width_33_256_4_e8", "width_255_unneeded_e4", "width_255_unneeded_e8",
              "lengths_width_33_e8", "lengths_width_64_e8", "padded_to_10_bytes_e4", "first_tenth_byte_1_e8", "min_delta_padded",
              "header_alone_0_o1_e4", "header_alone_1_o0_e8", "header_alone_1_negative_o0_e4", "cut_nowhere_o1_e4", "trailing_bytes_o0_e8",
              "trailing_bytes_o1_e4", "wanted_296_of_296_o1_e8", "wanted_0_holds_0_no_capacity_o0_e4", "unneeded_width_bytes_there",
              "alternating_ends_128_e8", "alternating_ends_256_e4", "min_delta_lowest_e8", "min_delta_highest_e4",
              "first_value_of_64_bits_e4", "sum_is_the_bytes_behind_offsets_e4", "sum_below_the_bytes_behind_offsets_e8",
              "empty_strings_offsets_e4", "size_1024_8_2049_e8", "size_384_4_770_offsets_e4"):
        assert by_name[k]["status"] == G.SUCCESS, k
    assert by_name["wanted_0_holds_0_no_capacity_o1_e4"]["status"] == G.CANNOT_DECOMPRESS, "Offsets writes total + 1 elements"
    assert by_name["header_alone_0_o0_e4"]["consumed"] == by_name["header_alone_1_o1_e8"]["consumed"] == 5


# ---- 3. isolation -------------------------------------------------------------------------------------------------
def _mixed(n, output, element, counted=True):
    """n items of one call: hostile ones first, in the middle, last and every fourth; capacities exact and one short"""
    pool = _by_call(G.all_plans() + [g.plan for g in G.fixture_pages()])[(output, element, counted)]
    good = [p for p in pool if _model(p)[0] == G.SUCCESS and (p.wanted or not counted and p.capacity() > 1)]
    hostile = [p for p in pool if _model(p)[0] != G.SUCCESS]
    items = []
    for i in range(n):
        src = hostile[(5 * i + 1) % len(hostile)] if n > 1 and (i in (0, n // 2, n - 1) or i % 4 == 1) else good[(7 * i + 3) % len(good)]
        items.append(G.Plan(src.name, src.data, src.output, src.element, src.wanted, "S" if i % 5 == 2 and src.cap == "E" else src.cap))
    return items


ISOLATION = [(n, output, element) for n in (1, 3, 65, 300) for output, element in CALLS]


@pytest.fixture(scope="module")
def isolation(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_delta_isolation")
    cases = {"n%d_o%d_e%d" % key: Case(_mixed(*key, counted=key[0] != 65), ones=1) for key in ISOLATION}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("n,output,element", ISOLATION)
def test_isolation(isolation, n, output, element):
    cases, results = isolation
    name = "n%d_o%d_e%d" % (n, output, element)
    _check_case(cases[name], results[name])
    if n >= 65:
        items = list(zip(cases[name].items, results[name][0]))
        assert {w["status"] for _, w in items} == {G.SUCCESS, G.CANNOT_DECOMPRESS}
        assert any(p.cap == "S" and p.capacity() and w["status"] == G.CANNOT_DECOMPRESS and w["untouched"] for p, w in items)


# ---- 4. odd addresses, 5. null arrays -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(driver, plans, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_delta_shapes")
    cases = {}
    for align in (1, 3, 7):
        for output, element in CALLS:
            cases["align_%d_o%d_e%d" % (align, output, element)] = Case(_by_call(plans)[(output, element, False)], align=align)
    for nulls in (1, 2, 3):
        for output, element in ((G.VALUES, G.INT), (G.OFFSETS, G.LONGLONG)):
            cases["nulls_%d_o%d_e%d" % (nulls, output, element)] = Case(_mixed(65, output, element, counted=nulls != 3), nulls=nulls, ones=1)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("align", [1, 3, 7])
def test_odd_addresses(shapes, align):
    cases, results = shapes
    names = [k for k in cases if k.startswith("align_%d_" % align)]
    assert len(names) == 4
    for name in names:
        _check_case(cases[name], results[name])
        assert any(w["status"] == G.SUCCESS and w["count"] > 512 for w in results[name][0])


@pytest.mark.parametrize("nulls", [1, 2, 3])
def test_null_arrays(shapes, nulls):
    """1: no device_value_counts; 2: no device_consumed_bytes; 3: neither, and no device_num_values (test_planned_streams and
    test_isolation have that array null and set with the other two set)"""
    cases, results = shapes
    for name in (k for k in cases if k.startswith("nulls_%d_" % nulls)):
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


# ---- 6. the chained use ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", ["v1", "v2"])
@pytest.mark.parametrize("column", ["sums64", "int32", "strings"])
def test_levels_then_values_without_a_host_round_trip(driver, pages, version, column, tmp_path):
    """the levels with the count of the maximum level; that device array as the delta call's device_num_values.  Under
    Offsets the strings are read through the offsets at stream + consumed."""
    mine = [g for g in pages if g.version == version and g.column == column]
    assert len(mine) >= 5
    blob, lines = bytearray(), []
    for g in mine:
        lines.append("%s %d %d %d %d %d %d" % (tmp_path / "pool.bin", len(blob), len(g.levels.data), g.levels.form,
                                               len(blob) + len(g.levels.data), len(g.plan.data), g.levels.wanted))
        blob += g.levels.data + g.plan.data
    (tmp_path / "pool.bin").write_bytes(bytes(blob))
    (tmp_path / "chain.list").write_text("\n".join(lines) + "\n")
    output, element = mine[0].plan.output, mine[0].plan.element
    r = subprocess.run([driver, "chain", str(tmp_path / "chain.list"), str(tmp_path / "chain.out"), str(output), str(element)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, got, pos = _words(r.stdout), (tmp_path / "chain.out").read_bytes(), 0
    assert len(words) == len(mine)
    for g, w in zip(mine, words):
        rows = g.levels.wanted
        assert (w["levels_status"], w["values_status"]) == (G.SUCCESS, G.SUCCESS), g.name
        assert w["non_null"] == w["count"] == g.plan.wanted < rows, g.name
        assert list(got[pos:pos + rows]) == g.want_levels, g.name
        pos += rows
        elements = list(struct.unpack_from("<%d%s" % (len(g.want), G.LETTER[element]), got, pos))
        assert elements == g.want, g.name
        assert got[pos + len(g.want) * element:pos + (rows + 1) * element] == bytes([FILL]) * ((rows + 1 - len(g.want)) * element)
        pos += (rows + 1) * element
        if output == G.OFFSETS:
            strings = g.plan.data[w["consumed"]:]
            assert [strings[a:b] for a, b in zip(elements, elements[1:])] == [g.want_bytes[a:b] for a, b in zip(g.want, g.want[1:])]
            assert strings[:elements[-1]] == g.want_bytes
        else:
            assert w["consumed"] == len(g.plan.data), g.name
    assert pos == len(got)


# ---- 7. what throws before a launch -----------------------------------------------------------------------------------
def test_misuse(driver):
    r = subprocess.run([driver, "misuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    w = _words(r.stdout)[0]
    assert w["threw"] == 14, ("more than 2^20 items, each of the five mandatory arrays null, seven element types outside the two, "
                              "an unknown output")
    assert w["nothing_launched"] == 1
    assert w["quiet"] == 2 and w["decoded"] == 1, "no items: nothing to do; and the call as it is meant"
