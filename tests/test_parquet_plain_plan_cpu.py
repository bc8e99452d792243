"""The arithmetic and the rules of the placing of a Parquet page's dense values in rows
(hipcomp-core_amd/csrc/parquet_plain_plan.hpp: place_parquet_values, place_parquet_booleans and place_parquet_strings of
the Cascaded manager -- the one copy the kernels and the host share).  tests/parquet_plain_plan_driver.cpp, a program of
its own, works every fixture page and every planned item with every input array in a buffer of exactly its length and
every output in a buffer of exactly its capacity; it is compiled with g++ under the address and undefined-behaviour
sanitizers, without HIP, and held to the restatement of tests/parquet_plaingen.py byte for byte and verdict for verdict.
The restatement itself is held to what the fixtures say their pages hold: the table pyarrow was given."""
import os
import struct
import subprocess

import pytest

import parquet_plaingen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
# (column, encoding) -> value bytes
COLUMNS = {("int32", "plain"): 4, ("int64", "plain"): 8, ("float", "plain"): 4, ("float", "split"): 4, ("double", "plain"): 8,
           ("double", "split"): 8, ("int96", "plain"): 12, ("decimal5", "plain"): 5, ("decimal16", "plain"): 16, ("boolean", "boolean"): 0,
           ("strings", "prefixed"): 0, ("strings", "packed"): 0, ("delta", "delta"): 8}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("parquet_plain_plan") / "parquet_plain_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "parquet_plain_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


@pytest.fixture(scope="module")
def plans():
    return G.all_plans()


@pytest.fixture(scope="module")
def worked(driver, pages, plans, tmp_path_factory):
    """[(item, the driver's words, its outputs)]"""
    tmp = tmp_path_factory.mktemp("parquet_plain_pool")
    pool = [g.item() for g in pages] + plans
    blob = bytearray()
    (tmp / "pool.list").write_text("\n".join(p.line(blob) for p in pool) + "\n")
    (tmp / "pool.bin").write_bytes(bytes(blob))
    r = subprocess.run([driver, str(tmp / "pool.bin"), str(tmp / "pool.list"), str(tmp / "pool.out")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    words = [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in r.stdout.splitlines())]
    assert [w["item"] for w in words] == list(range(len(pool)))
    out, got, pos = (tmp / "pool.out").read_bytes(), [], 0
    for p, w in zip(pool, words):
        outs = []
        for size in p.sizes():
            outs.append(out[pos:pos + size])
            pos += size
        got.append((p, w, outs))
    assert pos == len(out)
    return got


def test_the_header_is_the_restatements(worked):
    """a refused item's outputs are the fill, whole; an accepted item's are the fill behind what it writes"""
    refused = 0
    for p, w, outs in worked:
        status, count, want = p.model()
        assert (w["status"], w["count"]) == (status, count), p.name
        assert outs == want, p.name
        if w["status"] != G.SUCCESS:
            refused += 1
            assert w["count"] == 0 and all(set(o) <= {G.FILL} for o in outs), ("a refused item wrote or counted", p.name)
    assert refused >= 100


def calls():
    """every (kind, value bytes, layout, levels) a call can have"""
    want = {(G.BOOLEANS, 0, 0, levels) for levels in (False, True)}
    want |= {(G.STRINGS, 0, layout, levels) for layout in (G.LENGTH_PREFIXED, G.PACKED) for levels in (False, True)}
    want |= {(G.VALUES, w, layout, levels) for w in G.VALUE_BYTES for layout in (G.PLAIN, G.SPLIT) for levels in (False, True)}
    return want


def test_the_pool_has_both_verdicts_of_every_call(worked):
    seen = {p.call() + (w["status"],) for p, w, _ in worked}
    assert seen >= {c + (s,) for c in calls() for s in (G.SUCCESS, G.CANNOT_DECOMPRESS)}
    rows = {(p.call(), p.rows) for p, w, _ in worked if w["status"] == G.SUCCESS}
    assert rows >= {(c, n) for c in calls() for n in G.ROWS}
    assert sum(w["status"] != G.SUCCESS for _, w, _ in worked) >= 100


def test_a_planned_refusal_for_every_rule(plans):
    """each in the last step of its item, and refused for the rule its name says: the item it was made from is accepted"""
    by_name = {p.name: p for p in plans}
    rules = ["capacity_one_short", "source_one_byte_short", "start_one_above_the_bytes", "level_above_the_maximum_in_the_last_row",
             "one_valid_row_more", "one_valid_row_fewer", "no_values_and_a_valid_row"]
    names = ["values_%s_%s_w%d" % (r, layout, w) for r in rules for layout in ("plain", "split") for w in G.VALUE_BYTES]
    names += ["booleans_" + r for r in rules]
    for layout in ("prefixed", "packed"):
        names += ["strings_%s_%s" % (r, layout) for r in rules + ["bytes_one_short", "the_last_offset_falls", "an_offset_falls", "a_negative_offset",
                                                                   "the_last_end_one_past_the_body", "a_byte_total_of_2_31"]]
    for name in names:
        assert by_name[name].model()[0] == G.CANNOT_DECOMPRESS, name
    assert by_name["values_every_fourth_null_plain_w4"].model()[0] == G.SUCCESS
    assert by_name["booleans_every_fourth_null"].model()[0] == G.SUCCESS
    for layout in ("prefixed", "packed"):
        assert by_name["strings_every_fourth_null_" + layout].model()[0] == G.SUCCESS
        assert by_name["strings_the_last_end_at_the_end_of_the_body_" + layout].model()[0] == G.SUCCESS
        p = by_name["strings_a_byte_total_of_2_31_" + layout]
        assert sum(b - a for a, b in zip(p.offsets, p.offsets[1:p.num_values + 1])) == 1 << 31 and len(p.src) < 20000


def test_the_restatement_reads_what_pyarrow_was_given(pages):
    """values, bits, or offsets and bytes, and the bitmap: pinned to the table when the fixtures were made"""
    assert len(pages) >= 300
    seen = set()
    for g in pages:
        it = g.item()
        assert it.levels == g.want_levels and it.levels.count(1) == g.non_null == it.num_values, g.name
        status, count, outs = it.model()
        assert status == G.SUCCESS, g.name
        if g.encoding == "boolean":
            assert outs == [g.want_bits, g.want_validity], g.name
        elif it.kind == G.VALUES:
            assert outs == [g.want_values, g.want_validity], g.name
            assert len(g.want_values) == g.rows * g.value_bytes and it.value_bytes == g.value_bytes
        else:
            assert outs == [struct.pack("<%di" % (g.rows + 1), *g.want_offsets), g.want_bytes, g.want_validity], g.name
            assert count == len(g.want_bytes) == g.want_offsets[-1]
        seen.add((g.version, g.column, g.encoding, g.value_bytes))
    assert seen == {(v, c, e, w) for v in ("v1", "v2") for (c, e), w in COLUMNS.items()}
    for version in ("v1", "v2"):
        for column, encoding in COLUMNS:
            mine = [g for g in pages if (g.version, g.column, g.encoding) == (version, column, encoding)]
            assert len(mine) >= 4, "several pages"
            assert sum(g.rows for g in mine) == 1500
            assert any(g.non_null == 0 and g.rows for g in mine), "a page that is wholly null"
            assert mine[0].want_levels[0] == 0 and mine[0].want_levels[7] == 0 and mine[0].want_levels[1] == 1, "every seventh row is null"
    # a V1 page's source is the whole page, its start the bytes of its levels
    assert all(g.item().start == len(g.levels.data) > 0 for g in pages if g.version == "v1" and g.encoding in ("plain", "split", "boolean"))
    strings = [g for g in pages if g.column == "strings"]
    lengths = {b - a for g in strings for a, b in zip(g.want_offsets, g.want_offsets[1:])}
    assert lengths >= {0, 1, 63, 64, 65, 301}
