"""Batches of Parquet RLE / bit-packed hybrid streams in one call (hipcomp/cascaded.hpp: decode_parquet_hybrid of the
Cascaded manager; INTEGRATION.md, "Parquet levels and dictionary indices in the Cascaded manager", has the contract),
through tests/parquet_hybrid_driver.cpp, a C++ program written against include/ and linked to libhipcomp.so.  The driver
works through a list of cases per process, each process under a timeout; it puts guard bytes on both sides of every
output.

Fixtures: every level stream and every index stream of tests/golden/parquet_hybrid/ (pyarrow's V1 and V2 pages of a
nullable dictionary-encoded column) gives the fixture's values -- pinned to the table pyarrow was given --, match count
and consumed bytes.  Planned streams: every one of parquet_hybridgen's, alone and in one batch, gives what the
restatement says; a refused item leaves its output and guards untouched.  Isolation: in batches of 1, 3, 65 and 300 items
with hostile items first, in the middle and last, capacities exact and one short, every item's result is its one-item
result.  Odd addresses: streams 1, 3 and 7 bytes behind an aligned address.  Null device_consumed_bytes, null match
arrays.  The chained use on V1 and V2 pages: the levels' match counts are the index call's num_values, with no host round
trip between the calls."""
import os
import struct
import subprocess

import pytest

import parquet_hybridgen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
LETTER = {1: "B", 2: "H", 4: "I"}
FORMS = (G.BARE, G.LENGTH_PREFIXED, G.WIDTH_PREFIXED)
ELEMENTS = (G.UCHAR, G.USHORT, G.UINT)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("parquet_hybrid") / "parquet_hybrid_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "parquet_hybrid_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


class Case:
    """items of one form and one element type (a call has one of each)"""

    def __init__(self, items, align=0, nulls=0, ones=0):
        assert len({(p.form, p.element) for p in items}) == 1
        self.items, self.form, self.element = items, items[0].form, items[0].element
        self.align, self.nulls, self.ones = align, nulls, ones


def _run_cases(driver, tmp, cases, timeout=300):
    """name -> (per-item words, per-item output bytes)"""
    blob, lines = bytearray(), []
    for name, c in cases.items():
        lines.append("case %d %d %d %d %d %s %d" % (c.form, c.element, c.align, c.nulls, c.ones, tmp / (name + ".out"), len(c.items)))
        for p in c.items:
            lines.append("%s %d %d %d %d %d %d" % (tmp / "pool.bin", len(blob), len(p.data), p.bit_width, p.wanted, p.capacity(), p.match))
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
        for w in items:
            outs.append(got[pos:pos + w["size"] * c.element])
            pos += w["size"] * c.element
        assert pos == len(got)
        results[name] = (items, outs)
    assert at == len(words)
    return results


_MODEL = {}


def _model(p):
    key = (p.data, p.form, p.bit_width, p.wanted, p.capacity(), p.element, p.match)
    if key not in _MODEL:
        _MODEL[key] = p.model()
    return _MODEL[key]


def _check_case(c, result):
    items, outs = result
    for p, w, out in zip(c.items, items, outs):
        status, want, consumed, matches = _model(p)
        assert w["guards"] == 1, ("bytes outside the wanted elements were written", p.name, w)
        assert (w["status"], w["size"]) == (status, p.wanted if status == G.SUCCESS else 0), (p.name, w)
        assert out == want, (p.name, "the values")
        if not c.nulls & 1:
            assert w["consumed"] == consumed, (p.name, w)
        if not c.nulls & 2:
            assert w["matches"] == matches, (p.name, w)
        if status != G.SUCCESS:
            assert w["untouched"] == 1, ("a refused item's output was written", p.name, w)
        if c.ones:
            assert w["one_status"] == w["status"] and w["eq_one"] == 1, (p.name, w)
            assert (w["one_consumed"], w["one_matches"]) == (w["consumed"], w["matches"]), (p.name, w)


def _by_call(plans):
    """{(form, element): the plans of it}"""
    groups = {}
    for p in plans:
        groups.setdefault((p.form, p.element), []).append(p)
    return groups


# ---- 1. the fixtures --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


@pytest.fixture(scope="module")
def fixtures(driver, pages, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_hybrid_fixtures")
    plans = [p for _, levels, _, indices, _ in pages for p in (levels, indices)]
    cases = {"f%d_e%d" % key: Case(items) for key, items in _by_call(plans).items()}
    return cases, _run_cases(driver, tmp, cases)


def test_fixtures(fixtures, pages):
    cases, results = fixtures
    want = {}
    for _, levels, want_levels, indices, want_indices in pages:
        want[levels.name] = (want_levels, len(want_indices), len(levels.data))
        want[indices.name] = (want_indices, want_indices.count(indices.match), len(indices.data))
    seen = 0
    for name, c in cases.items():
        _check_case(c, results[name])
        for p, w, out in zip(c.items, *results[name]):
            values, matches, consumed = want[p.name]
            assert w["status"] == G.SUCCESS and (w["matches"], w["consumed"]) == (matches, consumed), p.name
            assert list(struct.unpack("<%d%s" % (len(values), LETTER[p.element]), out)) == values, p.name
            seen += 1
    assert seen == 2 * len(pages) >= 48
    assert {c.form for c in cases.values()} == set(FORMS), "V1 levels, V2 levels, indices"


# ---- 2. the planned streams -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_hybrid_planned")
    cases = {"f%d_e%d" % key: Case(items, ones=1) for key, items in _by_call(G.all_plans()).items()}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("element", ELEMENTS)
def test_planned_streams(planned, form, element):
    """in one batch and alone"""
    cases, results = planned
    name = "f%d_e%d" % (form, element)
    _check_case(cases[name], results[name])
    statuses = {w["status"] for w in results[name][0]}
    assert statuses == {G.SUCCESS, G.CANNOT_DECOMPRESS}


def test_planned_refusals(planned):
    cases, results = planned
    by_name = {p.name: w for name, c in cases.items() for p, w in zip(c.items, results[name][0])}
    for k in ("width_33", "width_9_in_uchar", "width_17_in_ushort", "width_byte_33", "no_width_byte_values_wanted", "prefix_longer",
              "prefix_of_3_bytes", "first_header_6_bytes", "last_header_6_bytes", "first_header_33_bits", "last_header_33_bits",
              "first_rle_of_0", "last_rle_of_0", "first_packed_of_0_groups", "last_packed_of_0_groups", "first_rle_value_cut",
              "last_rle_value_cut", "first_packed_bytes_cut", "last_packed_bytes_cut", "first_ends_early", "last_ends_early",
              "capacity_one_short", "cut_w25_wants_17_one_short", "none_wanted_bare_width_33"):
        w = by_name[k]
        assert (w["status"], w["consumed"], w["matches"], w["size"], w["untouched"]) == (G.CANNOT_DECOMPRESS, 0, 0, 0, 1), k
    for k in ("rle_2_31_clipped_e1", "trailing_bytes", "cut_w25_wants_17_enough", "rle_value_above_width", "none_wanted_bare",
              "none_wanted_no_width_byte", "behind_last_rle_of_0", "header_32_bits", "header_across_window", "value_across_window",
              "packed_8192_groups_w12", "w32_e4_bare", "w0_e1_bare", "prefix_shorter"):
        assert by_name[k]["status"] == G.SUCCESS, k
    assert by_name["prefix_shorter"]["consumed"] == by_name["prefix_equal"]["consumed"] == 14
    assert by_name["rle_value_above_width"]["matches"] == 7


# ---- 3. isolation -------------------------------------------------------------------------------------------------
def _mixed(n, form, element):
    """n items of one call: hostile ones first, in the middle, last and every fourth; capacities exact and one short"""
    pool = _by_call(G.all_plans() + [p for _, levels, _, indices, _ in G.fixture_pages() for p in (levels, indices)])[(form, element)]
    good = [p for p in pool if _model(p)[0] == G.SUCCESS and p.wanted]
    hostile = [p for p in pool if _model(p)[0] != G.SUCCESS]
    items = []
    for i in range(n):
        src = hostile[(5 * i + 1) % len(hostile)] if n > 1 and (i in (0, n // 2, n - 1) or i % 4 == 1) else good[(7 * i + 3) % len(good)]
        items.append(G.Plan(src.name, src.data, src.wanted, src.bit_width, src.form, src.element, src.match,
                            "S" if src.cap == "S" or i % 5 == 2 else "E"))
    return items


ISOLATION = [(n, form, element) for n in (1, 3, 65, 300)
             for form, element in ((G.BARE, G.UCHAR), (G.LENGTH_PREFIXED, G.UINT), (G.WIDTH_PREFIXED, G.USHORT))]


@pytest.fixture(scope="module")
def isolation(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_hybrid_isolation")
    cases = {"n%d_f%d_e%d" % key: Case(_mixed(*key), ones=1) for key in ISOLATION}
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("n,form,element", ISOLATION)
def test_isolation(isolation, n, form, element):
    cases, results = isolation
    name = "n%d_f%d_e%d" % (n, form, element)
    _check_case(cases[name], results[name])
    if n >= 65:
        items = list(zip(cases[name].items, results[name][0]))
        assert {w["status"] for _, w in items} == {G.SUCCESS, G.CANNOT_DECOMPRESS}
        assert any(p.cap == "S" and p.wanted and w["status"] == G.CANNOT_DECOMPRESS and w["untouched"] for p, w in items)


# ---- 4. odd addresses, 5. null arrays -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_hybrid_shapes")
    cases = {}
    for align in (1, 3, 7):
        for form, element in ((G.BARE, G.UCHAR), (G.BARE, G.UINT), (G.LENGTH_PREFIXED, G.UINT), (G.WIDTH_PREFIXED, G.USHORT)):
            cases["align_%d_f%d_e%d" % (align, form, element)] = Case(_by_call(G.all_plans())[(form, element)], align=align)
    for nulls in (1, 2, 3):
        for form, element in ((G.BARE, G.UCHAR), (G.WIDTH_PREFIXED, G.UINT)):
            cases["nulls_%d_f%d_e%d" % (nulls, form, element)] = Case(_mixed(65, form, element), nulls=nulls, ones=1)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("align", [1, 3, 7])
def test_odd_addresses(shapes, align):
    cases, results = shapes
    names = [k for k in cases if k.startswith("align_%d_" % align)]
    assert len(names) == 4
    for name in names:
        _check_case(cases[name], results[name])
        assert any(w["status"] == G.SUCCESS and w["size"] > 512 for w in results[name][0])


@pytest.mark.parametrize("nulls", [1, 2, 3])
def test_null_arrays(shapes, nulls):
    """1: no device_consumed_bytes; 2: no match arrays; 3: neither, and no device_bit_widths under WidthPrefixed"""
    cases, results = shapes
    for name in (k for k in cases if k.startswith("nulls_%d_" % nulls)):
        _check_case(cases[name], results[name])
        assert {w["status"] for w in results[name][0]} == {G.SUCCESS, G.CANNOT_DECOMPRESS}


# ---- 6. the chained use ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_levels_then_indices_without_a_host_round_trip(driver, pages, version, tmp_path):
    """the levels with the count of the maximum level; that device array as the index call's num_values"""
    mine = [(n, lv, wl, ix, wi) for n, lv, wl, ix, wi in pages if n.startswith(version + "_c5000") or n.startswith(version + "_c300")]
    mine = [m for m in mine if m[3].element == G.USHORT]
    assert len(mine) >= 8
    blob, lines = bytearray(), []
    for _, levels, _, indices, _ in mine:
        lines.append("%s %d %d %d %d %d %d %d" % (tmp_path / "pool.bin", len(blob), len(levels.data), levels.form,
                                                  len(blob) + len(levels.data), len(indices.data), indices.element, levels.wanted))
        blob += levels.data + indices.data
    (tmp_path / "pool.bin").write_bytes(bytes(blob))
    (tmp_path / "chain.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "chain", str(tmp_path / "chain.list"), str(tmp_path / "chain.out")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, got, pos = _words(r.stdout), (tmp_path / "chain.out").read_bytes(), 0
    assert len(words) == len(mine)
    for (name, levels, want_levels, indices, want_indices), w in zip(mine, words):
        assert (w["levels_status"], w["index_status"]) == (G.SUCCESS, G.SUCCESS), name
        assert w["non_null"] == len(want_indices) < levels.wanted and w["index_consumed"] == len(indices.data), name
        assert list(got[pos:pos + levels.wanted]) == want_levels, name
        pos += levels.wanted
        assert list(struct.unpack_from("<%dH" % len(want_indices), got, pos)) == want_indices, name
        pos += 2 * len(want_indices)
    assert pos == len(got)


# ---- 7. what throws before a launch -----------------------------------------------------------------------------------
def test_misuse(driver):
    r = subprocess.run([driver, "misuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    w = _words(r.stdout)[0]
    assert w["threw"] == 17, ("more than 2^20 items, each mandatory array null (the bit widths under Bare and LengthPrefixed), one "
                              "match array without the other, five element types outside the three, an unknown form")
    assert w["nothing_launched"] == 1
    assert w["quiet"] == 2 and w["decoded"] == 1, "no items: nothing to do; and the call as it is meant"
