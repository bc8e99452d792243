"""The arithmetic and the rules of the gather of a Parquet dictionary's entries to rows
(hipcomp-core_amd/csrc/parquet_dict_plan.hpp: index_parquet_dictionary, gather_parquet_dictionary and
gather_parquet_dictionary_strings of the Cascaded manager -- the one copy the kernels and the host share).
tests/parquet_dict_plan_driver.cpp, a program of its own, works every fixture page and every planned item with every
input array in a buffer of exactly its length and every output in a buffer of exactly its capacity; it is compiled with
g++ under the address and undefined-behaviour sanitizers, without HIP, and held to the restatement of
tests/parquet_dictgen.py byte for byte and verdict for verdict.  The restatement itself is held to what the fixtures say
their pages hold: the table pyarrow was given."""
import os
import struct
import subprocess

import pytest

import parquet_dictgen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
COLUMNS = {"int32": 4, "int64": 8, "float": 4, "double": 8, "int96": 12, "decimal5": 5, "decimal16": 16, "strings": 0}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("parquet_dict_plan") / "parquet_dict_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "parquet_dict_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


@pytest.fixture(scope="module")
def plans():
    return G.all_plans()


def _dictionaries(pages):
    """the dictionary page of every strings fixture, as an item of index_parquet_dictionary"""
    seen = {}
    for g in pages:
        if not g.entry_bytes:
            seen.setdefault(g.name.rsplit("_", 1)[0], G.Item(G.INDEX, g.name.rsplit("_", 1)[0] + "_dictionary", body=g.dictionary,
                                                             entries=g.dict_entries, capacity=g.dict_entries + 1))
    return list(seen.values())


@pytest.fixture(scope="module")
def worked(driver, pages, plans, tmp_path_factory):
    """[(item, the driver's words, its outputs)]"""
    tmp = tmp_path_factory.mktemp("parquet_dict_pool")
    pool = [g.item() for g in pages] + _dictionaries(pages) + plans
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


def test_the_pool_has_both_verdicts_of_every_call(worked):
    seen = {p.call() + (w["status"],) for p, w, _ in worked}
    want = {(G.INDEX, 0, False), (G.STRINGS, 0, False), (G.STRINGS, 0, True)}
    want |= {(G.FIXED, e, levels) for e in G.ENTRY_BYTES for levels in (False, True)}
    assert seen >= {c + (s,) for c in want for s in (G.SUCCESS, G.CANNOT_DECOMPRESS)}
    rows = {(p.call(), p.rows) for p, w, _ in worked if p.kind != G.INDEX and w["status"] == G.SUCCESS}
    assert rows >= {(c, n) for c in want if c[0] != G.INDEX for n in G.ROWS}


def test_the_restatement_reads_what_pyarrow_was_given(pages):
    """values, or offsets and bytes, and the bitmap: pinned to the table when the fixtures were made"""
    assert len(pages) >= 300
    seen = set()
    for g in pages:
        it = g.item()
        assert it.levels == g.want_levels and it.levels.count(1) == g.non_null == len(it.indices), g.name
        status, count, outs = it.model()
        assert status == G.SUCCESS, g.name
        if g.entry_bytes:
            assert outs == [g.want_values, g.want_validity], g.name
            assert len(g.want_values) == g.rows * g.entry_bytes
        else:
            assert outs == [struct.pack("<%di" % (g.rows + 1), *g.want_offsets), g.want_bytes, g.want_validity], g.name
            assert count == len(g.want_bytes) == g.want_offsets[-1]
        seen.add((g.version, g.column, g.entry_bytes))
    assert seen == {(v, c, e) for v in ("v1", "v2") for c, e in COLUMNS.items()}
    for version in ("v1", "v2"):
        for column in COLUMNS:
            mine = [g for g in pages if (g.version, g.column) == (version, column)]
            assert len(mine) >= 4, "several pages on one dictionary"
            assert len({g.dictionary for g in mine}) == 1
            assert any(g.non_null == 0 and g.rows for g in mine), "a page that is wholly null"
            assert all(g.want_levels[r] == 0 for g in mine[:1] for r in range(0, g.rows, 7)), "every seventh row is null"
    strings = [g for g in pages if g.column == "strings"]
    lengths = {b - a for g in strings for a, b in zip(g.want_offsets, g.want_offsets[1:])}
    assert lengths >= {0, 1, 63, 64, 65, 301}
    offsets = G.index_dictionary(strings[0].dictionary, strings[0].dict_entries, strings[0].dict_entries + 1)
    assert {b - a for a, b in zip(offsets, offsets[1:])} >= {0, 1, 63, 64, 65, 301}

