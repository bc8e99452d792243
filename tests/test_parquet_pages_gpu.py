"""The pages of Parquet column chunks in one call (hipcomp/snappy.hpp: decompress_parquet_pages and get_parquet_pages_sizes
of the Snappy manager; INTEGRATION.md, "Parquet column chunks in the Snappy manager", has the contract), through
tests/parquet_pages_driver.cpp, a C++ program written against include/ and linked to libhipcomp.so.  The driver works
through a list of cases per process, each process under a timeout; it puts guard bytes on both sides of every output and
every page table and behind a caller-owned scratch buffer.

Fixtures: every chunk of tests/golden/parquet_pages/ (pyarrow's V1 and V2 pages under snappy and none, dictionary pages,
a nested column, one page of 160 000 bytes) decodes to the manifest's hashes page by page, with the manifest's rows as
its table, under each ChecksumPolicy.  Planned chunks: every one of parquet_pagegen's, alone and in a batch, gives what
the restatement says.  Isolation: in batches of 1, 3, 65 and 300 items with hostile items first, in the middle and last,
capacities exact, one short and oversize and page tables exact and one row short, every item's result is its one-item
result.  Passes: two pages per pass give what one pass gives.  Odd addresses: chunks and outputs 1, 3 and 7 bytes behind
an aligned address."""
import functools
import hashlib
import os
import subprocess

import pytest

import parquet_pagegen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
POLICIES = range(5)
ROW = 72
GOOD = (G.SUCCESS, G.CANNOT_VERIFY)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("parquet_pages") / "parquet_pages_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "parquet_pages_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


class Item:
    def __init__(self, name, data, codec, cap="E", rows="E"):
        self.name, self.data, self.codec, self.cap, self.rows = name, data, codec, cap, rows


class Case:
    def __init__(self, policy, items, scratch="own", pass_pages=0, tables=1, align=0, ones=0):
        assert len({it.codec for it in items}) == 1, "a column has one codec"
        self.policy, self.items, self.codec = policy, items, items[0].codec
        self.scratch, self.pass_pages, self.tables, self.align, self.ones = scratch, pass_pages, tables, align, ones


def _run_cases(driver, tmp, cases, timeout=300):
    """name -> (per-item words, the case's words, per item (output, table rows))"""
    blob, lines = bytearray(), []
    for name, c in cases.items():
        lines.append("case %d %d %s %d %d %d %d %s %d" % (c.policy, c.codec, c.scratch, c.pass_pages, c.tables, c.align, c.ones,
                                                       tmp / (name + ".out"), len(c.items)))
        for it in c.items:
            lines.append("%s %d %d %s %s" % (tmp / "pool.bin", len(blob), len(it.data), it.cap, it.rows))
            blob += it.data
    (tmp / "pool.bin").write_bytes(bytes(blob))
    (tmp / "cases.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "batch", str(tmp / "cases.list")], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, results, at = _words(r.stdout), {}, 0
    for name, c in cases.items():
        items, case = words[at:at + len(c.items)], words[at + len(c.items)]
        at += len(c.items) + 1
        assert [w["item"] for w in items] == list(range(len(c.items))) and "case" in case
        got, outs, pos = (tmp / (name + ".out")).read_bytes(), [], 0
        for w in items:
            out = got[pos:pos + w["size"]]
            pos += w["size"]
            rows = got[pos:pos + ROW * w["pages"] * c.tables]
            pos += len(rows)
            outs.append((out, rows))
        assert pos == len(got)
        results[name] = (items, case, outs)
    assert at == len(words)
    return results


# ---- what the restatement says of an item -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _query(data, codec):
    """the size query: (status, size, pages)"""
    try:
        pages = G.walk(data, codec)
    except G.Refused:
        return G.CANNOT_DECOMPRESS, 0, 0
    return G.SUCCESS, sum(p["uncompressed_page_size"] for p in pages), len(pages)


def _sized(word, exact, more):
    return max(exact - 1, 0) if word == "S" else exact + more if word == "O" else exact


@functools.lru_cache(maxsize=None)
def _model(data, codec, policy, capacity, table_capacity):
    status, out, pages = G.model(data, codec, policy, capacity, table_capacity)
    return status, out, b"".join(G.page_row(p) for p in pages), len(pages)


def _check_item(it, c, w, got):
    _, q_size, q_pages = _query(it.data, it.codec)
    capacity = _sized(it.cap, q_size, 77)
    rows = _sized(it.rows, q_pages, 3) if c.tables else None
    policy = {1: 0, 3: 2}.get(c.policy, c.policy)   # (the computing policies read as their twins)
    status, out, table, pages = _model(it.data, it.codec, policy, capacity, rows)
    assert w["guards"] == 1, ("bytes outside an output or a table were written", it.name, w)
    assert (w["q_status"], w["q_size"], w["q_pages"]) == _query(it.data, it.codec), (it.name, w)
    assert (w["status"], w["size"], w["pages"]) == (status, len(out), pages), (it.name, c.policy, it.cap, it.rows, w)
    assert got[0] == out, (it.name, "the bytes")
    if c.tables:
        assert got[1] == table, (it.name, "the page table")
    # what is refused before the passes -- by the walk, for its output or for its table -- has no byte written
    walk_refused = _query(it.data, it.codec)[0] != G.SUCCESS
    too_small = capacity < q_size or (rows is not None and rows < q_pages)
    if walk_refused or too_small:
        assert w["untouched"] == 1, ("a refused item's output was written", it.name, w)
    if c.ones:
        assert (w["one_status"], w["one_size"], w["one_pages"]) == (status, len(out), pages) and w["eq_one"] == 1, (it.name, w)


def _check_case(c, result):
    items, case, outs = result
    assert case["scratch_intact"] == 1
    for it, w, got in zip(c.items, items, outs):
        _check_item(it, c, w, got)
    return case


# ---- the pools --------------------------------------------------------------------------------------------------
def _fixture_items(codec):
    items = []
    for name in G.fixture_names():
        blob, manifest = G.load_fixture(name)
        for k, c in enumerate(manifest["chunks"]):
            if c["codec"] == codec:
                items.append((Item("%s_%d" % (name, k), blob[c["offset"]:c["offset"] + c["length"]], codec), c))
    return items


def _plan_items(codec):
    return [Item(p.name, p.data, p.codec) for p in G.all_plans() if p.codec == codec]


# ---- 1. the fixtures --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_pages_fixtures")
    cases = {}
    for policy in POLICIES:
        for codec in (G.SNAPPY, G.UNCOMPRESSED):
            cases["p%d_c%d" % (policy, codec)] = Case(policy, [it for it, _ in _fixture_items(codec)],
                                                     scratch="caller" if policy == 0 else "own")
    return cases, _run_cases(driver, tmp, cases)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("codec", [G.SNAPPY, G.UNCOMPRESSED])
def test_fixtures(fixtures, policy, codec):
    cases, results = fixtures
    name = "p%d_c%d" % (policy, codec)
    _check_case(cases[name], results[name])
    items, _, outs = results[name]
    # the manifest (what pyarrow's own codec decoded when the fixtures were made), page by page and row by row
    for (it, chunk), w, (out, rows) in zip(_fixture_items(codec), items, outs):
        assert w["status"] == G.SUCCESS and w["pages"] == len(chunk["pages"]) == w["q_pages"], it.name
        assert w["size"] == w["q_size"] == sum(p["uncompressed_page_size"] for p in chunk["pages"]), it.name
        for k, p in enumerate(chunk["pages"]):
            body = out[p["out_offset"]:p["out_offset"] + p["uncompressed_page_size"]]
            assert hashlib.sha256(body).hexdigest() == p["sha256"], (it.name, k)
            assert rows[ROW * k:ROW * (k + 1)] == G.page_row(p), (it.name, k)


# ---- 2. the planned chunks --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_pages_planned")
    cases = {}
    for policy in POLICIES:
        for codec in (G.SNAPPY, G.UNCOMPRESSED):
            cases["p%d_c%d" % (policy, codec)] = Case(policy, _plan_items(codec), ones=1)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("codec", [G.SNAPPY, G.UNCOMPRESSED])
def test_planned_chunks(planned, policy, codec):
    cases, results = planned
    name = "p%d_c%d" % (policy, codec)
    _check_case(cases[name], results[name])
    by_name = {it.name: w for it, w in zip(cases[name].items, results[name][0])}
    verifying = policy in G.VERIFYING
    if codec == G.SNAPPY:
        assert by_name["wrong_crc"]["status"] == by_name["wrong_crc"]["one_status"] == (G.BAD_CHECKSUM if verifying else G.SUCCESS)
        assert by_name["wrong_crc_and_damaged"]["status"] == (G.BAD_CHECKSUM if verifying else G.CANNOT_DECOMPRESS)
        assert by_name["no_crc"]["status"] == (G.CANNOT_VERIFY if policy == 4 else G.SUCCESS) and by_name["no_crc"]["size"] == 501
        assert by_name["three_pages"]["status"] == G.SUCCESS and by_name["three_pages"]["pages"] == 3
        assert by_name["empty_chunk"]["status"] == G.SUCCESS and by_name["empty_chunk"]["size"] == 0
        for k in ("trailing_byte", "damaged_block", "preamble_one_above", "preamble_one_below", "nesting_beyond_the_limit",
                  "varint_six_bytes", "cut_01", "v2_levels_above_compressed"):
            assert (by_name[k]["status"], by_name[k]["size"], by_name[k]["pages"]) == (G.CANNOT_DECOMPRESS, 0, 0), k
    else:
        assert by_name["stored_wrong_crc"]["status"] == (G.BAD_CHECKSUM if verifying else G.SUCCESS)


# ---- 3. isolation -------------------------------------------------------------------------------------------------
def _mixed(n, exact=False):
    good = [it for it, _ in _fixture_items(G.SNAPPY)] + [it for it in _plan_items(G.SNAPPY) if _query(it.data, G.SNAPPY)[0] == G.SUCCESS]
    hostile = [it for it in _plan_items(G.SNAPPY) if G.model(it.data, G.SNAPPY, 4)[0] not in GOOD]
    items = []
    for i in range(n):
        src = hostile[(5 * i + 1) % len(hostile)] if i in (0, n // 2, n - 1) or i % 4 == 1 else good[(7 * i + 3) % len(good)]
        items.append(Item(src.name, src.data, G.SNAPPY, cap="E" if exact else "ESO"[(i // 2) % 3],
                          rows="E" if exact else "EES"[(i // 3) % 3]))
    return items


@pytest.fixture(scope="module")
def isolation(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_pages_isolation")
    cases = {"n%d_p%d" % (n, policy): Case(policy, _mixed(n), ones=1) for n in (1, 3, 65, 300) for policy in (0, 4)}
    cases["n65_no_tables"] = Case(2, _mixed(65), tables=0, ones=1)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("name", ["n%d_p%d" % (n, policy) for n in (1, 3, 65, 300) for policy in (0, 4)] + ["n65_no_tables"])
def test_isolation(isolation, name):
    cases, results = isolation
    _check_case(cases[name], results[name])
    statuses = {w["status"] for w in results[name][0]}
    if len(cases[name].items) >= 65:
        assert {G.SUCCESS, G.CANNOT_DECOMPRESS} <= statuses and (G.INVALID_VALUE in statuses) == bool(cases[name].tables)


# ---- 4. passes, 5. odd addresses ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("parquet_pages_shapes")
    mixed = _mixed(40, exact=True)
    cases = {"one_pass": Case(4, mixed), "two_pages_own": Case(4, mixed, pass_pages=2),
             "two_pages_caller": Case(4, mixed, scratch="caller", pass_pages=2),
             "stored_two_pages": Case(2, [it for it, _ in _fixture_items(G.UNCOMPRESSED)] + _plan_items(G.UNCOMPRESSED),
                                      scratch="caller", pass_pages=2)}
    for align in (1, 3, 7):
        cases["align_%d" % align] = Case(4, _mixed(12) + [it for it, _ in _fixture_items(G.SNAPPY)][-3:], align=align, ones=1)
        cases["align_%d_stored" % align] = Case(2, [it for it, _ in _fixture_items(G.UNCOMPRESSED)][:3] + _plan_items(G.UNCOMPRESSED),
                                                align=align)
    return cases, _run_cases(driver, tmp, cases, timeout=600)


def test_passes(shapes):
    cases, results = shapes
    one = _check_case(cases["one_pass"], results["one_pass"])
    # every page of every item the walk does not refuse goes to the passes: the capacities are exact
    listed = sum(_query(it.data, it.codec)[2] for it in cases["one_pass"].items)
    assert one["passes"] == 1 and one["stats_pages"] == listed and listed > len(cases["one_pass"].items)
    for name in ("two_pages_own", "two_pages_caller"):
        two = _check_case(cases[name], results[name])
        assert two["pass_pages"] == 2 and two["stats_pages"] == one["stats_pages"] and two["passes"] == (one["stats_pages"] + 1) // 2
        assert results[name][2] == results["one_pass"][2], "the bytes and the tables of one pass"
        assert [(w["status"], w["size"], w["pages"]) for w in results[name][0]] == \
               [(w["status"], w["size"], w["pages"]) for w in results["one_pass"][0]]
    stored = _check_case(cases["stored_two_pages"], results["stored_two_pages"])
    assert stored["passes"] > 10


@pytest.mark.parametrize("align", [1, 3, 7])
def test_odd_addresses(shapes, align):
    cases, results = shapes
    for name in ("align_%d" % align, "align_%d_stored" % align):
        _check_case(cases[name], results[name])
        assert any(w["status"] == G.SUCCESS and w["size"] > 4096 for w in results[name][0])


# ---- 6. what throws before a launch -----------------------------------------------------------------------------------
def test_misuse(driver):
    r = subprocess.run([driver, "misuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    w = _words(r.stdout)[0]
    assert w["threw"] == 7, "a caller's scratch that does not hold the states, a null array, more than 2^20 chunks"
    assert w["quiet"] == 1 and w["items"] == 0, "a call that threw counts nothing; no chunks: nothing to do"
