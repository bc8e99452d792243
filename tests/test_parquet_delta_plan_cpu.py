"""The arithmetic and the rules of a decode of Parquet DELTA_BINARY_PACKED streams
(hipcomp-core_amd/csrc/parquet_delta_plan.hpp: decode_parquet_delta of the Cascaded manager -- the one copy the kernel
and the host share).  tests/parquet_delta_plan_driver.cpp, a program of its own, decodes every fixture stream and every
planned stream in a buffer of exactly its length into a buffer of exactly its capacity; it is compiled with g++ under
the address and undefined-behaviour sanitizers, without HIP, and held to the restatement of tests/parquet_deltagen.py
value for value and verdict for verdict.  The restatement itself is held to what the fixtures say their streams hold:
the table pyarrow was given."""
import os
import struct
import subprocess

import pytest

import parquet_deltagen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("parquet_delta_plan") / "parquet_delta_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "parquet_delta_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


@pytest.fixture(scope="module")
def plans():
    return G.all_plans()


def _pool(pages, plans):
    """every fixture stream -- as the page has it and without the caller's count --, every planned stream, and every
    planned stream one element short of its capacity"""
    pool = [g.plan for g in pages] + [G.Plan(g.name + "_uncounted", g.plan.data, g.plan.output, g.plan.element) for g in pages]
    return pool + plans + [p.short() for p in plans if p.cap == "E" and p.capacity()]


@pytest.fixture(scope="module")
def decoded(driver, pages, plans, tmp_path_factory):
    """[(plan, the driver's words, its output bytes)]"""
    tmp = tmp_path_factory.mktemp("parquet_delta_pool")
    pool = _pool(pages, plans)
    (tmp / "pool.bin").write_bytes(b"".join(p.data for p in pool))
    lines, at = [], 0
    for p in pool:
        lines.append("%s %d %d %d %d %d %d %d" % (tmp / "pool.bin", at, len(p.data), p.output, p.element, p.wanted is not None,
                                                  p.wanted or 0, p.capacity()))
        at += len(p.data)
    (tmp / "pool.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, str(tmp / "pool.list"), str(tmp / "pool.out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    words = [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in r.stdout.splitlines())]
    assert [w["item"] for w in words] == list(range(len(pool)))
    out, got, pos = (tmp / "pool.out").read_bytes(), [], 0
    for p, w in zip(pool, words):
        got.append((p, w, out[pos:pos + w["size"] * p.element]))
        pos += w["size"] * p.element
    assert pos == len(out)
    return got


def test_the_header_is_the_restatements(decoded):
    for p, w, out in decoded:
        status, want, consumed, count = p.model()
        assert w["ok"] == (status == G.SUCCESS), p.name
        assert (w["consumed"], w["count"], w["size"]) == (consumed, count, len(want) // p.element), p.name
        assert out == want, p.name
        assert w["untouched"] == 1, ("an element outside the item's, or one of a refused item, was written", p.name)


def _widths(p):
    """the widths of the needed miniblocks of an accepted stream"""
    trace = []
    G.decode(p.data, p.wanted, p.capacity(), p.output, p.element, trace)
    at = [lo for what, lo, hi in trace if what == "widths"]
    block, miniblocks, total = G.read_stream_header(p.data)[:3]
    widths, left = set(), total - 1
    for lo in at:
        widths |= set(p.data[lo:lo + -(-min(left, block) // (block // miniblocks))])
        left -= block
    return widths


def test_the_pool_has_both_verdicts_of_every_output_and_element(decoded):
    seen = {(p.output, p.element, w["ok"]) for p, w, _ in decoded}
    assert seen >= {(output, element, ok) for output in (G.VALUES, G.OFFSETS) for element in (G.INT, G.LONGLONG) for ok in (0, 1)}
    for element in (G.INT, G.LONGLONG):
        widths = set()
        for p, w, _ in decoded:
            if w["ok"] and p.output == G.VALUES and p.element == element and w["count"] > 1:
                widths |= _widths(p)
        assert widths >= set(G.WIDTHS[element]), element
        assert max(widths) == 8 * element
    names = {p.name: w["ok"] for p, w, _ in decoded}
    assert (names["width_33_128_4_e4"], names["width_33_128_4_e8"], names["width_65_128_4_e8"]) == (0, 1, 0)
    assert (names["width_33_in_one_miniblock_e4"], names["width_255_unneeded_e4"], names["width_255_unneeded_e8"]) == (0, 1, 1)
    shapes = {G.read_stream_header(p.data)[:2] for p, w, _ in decoded if w["ok"] and w["count"] > 1}
    assert {b for b, m in shapes} >= {128, 256, 384, 1024} and {m for b, m in shapes} >= {1, 2, 4, 8}
    assert {b // m for b, m in shapes} >= {32, 64, 96, 128}


def test_the_restatement_reads_what_pyarrow_was_given(pages):
    """values, or offsets and the string bytes behind the consumed bytes: pinned to the table when the fixtures were made"""
    assert len(pages) >= 50
    columns, shapes = set(), set()
    for g in pages:
        status, out, consumed, matches = g.levels.model()
        assert status == G.SUCCESS and list(out) == g.want_levels and consumed == len(g.levels.data), g.name
        assert matches == g.plan.wanted, "the count of ones is the value stream's num_values"
        status, out, consumed, count = g.plan.model()
        assert status == G.SUCCESS and count == g.plan.wanted, g.name
        assert list(struct.unpack("<%d%s" % (len(out) // g.plan.element, G.LETTER[g.plan.element]), out)) == g.want, g.name
        if g.want_bytes is None:
            assert consumed == len(g.plan.data), g.name
        else:
            assert g.plan.data[consumed:] == g.want_bytes and g.want[-1] == len(g.want_bytes), g.name
            assert 0 in {b - a for a, b in zip(g.want, g.want[1:])}, "empty strings"
        assert G.read_stream_header(g.plan.data)[:2] == (g.block_size, g.miniblocks), g.name
        columns.add((g.version, g.column))
        shapes.add((g.block_size, g.miniblocks))
    assert columns == {(v, c) for v in ("v1", "v2") for c in ("sums64", "int32", "const", "wrap64", "strings")}
    assert len(shapes) >= 2, "pyarrow cuts INT32 and INT64 streams differently"
    wrap = [g for g in pages if g.column == "wrap64"]
    assert all(set(g.want) == {1 << 63, (1 << 63) - 1} for g in wrap)
    assert all(_widths(g.plan) == {0} for g in pages if g.column == "const")


def test_a_refused_item_of_the_restatement_has_nothing(plans):
    refused = [p for p in plans if p.model()[0] != G.SUCCESS]
    assert len(refused) >= 100
    assert all(p.model() == (G.CANNOT_DECOMPRESS, b"", 0, 0) for p in refused)
