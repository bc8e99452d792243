"""The arithmetic and the page rules of a read of Parquet column chunks (hipcomp-core_amd/csrc/parquet_pages_plan.hpp:
decompress_parquet_pages of the Snappy manager -- the one copy the kernels and the host share): the Thrift reader and the
page rules over every fixture chunk and every planned chunk, the scratch layout and the partition of the pages into
passes.  tests/parquet_pages_plan_driver.cpp, a program of its own, prints them; it is compiled with g++ under the
address and undefined-behaviour sanitizers, without HIP, and held to the restatement of tests/parquet_pagegen.py, page
for page and verdict for verdict.  Every chunk is walked in a buffer of exactly its length."""
import os
import subprocess

import pytest

import parquet_pagegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
ITEM, LISTS8, LISTS4 = 128, 10, 5
ENTRY = LISTS8 * 8 + LISTS4 * 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("parquet_pages_plan") / "parquet_pages_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "parquet_pages_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, *args):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def _words(line):
    return dict(zip(line[0::2], (int(x) for x in line[1::2])))


# ---- the walk ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    """[(name, bytes, codec)]: every chunk of every fixture, every planned chunk under its codec and under the other"""
    tmp = tmp_path_factory.mktemp("parquet_pages_pool")
    pool = []
    for name in G.fixture_names():
        blob, manifest = G.load_fixture(name)
        for k, c in enumerate(manifest["chunks"]):
            pool.append(("%s_%d" % (name, k), blob[c["offset"]:c["offset"] + c["length"]], c["codec"]))
    for p in G.all_plans():
        pool.append((p.name, p.data, p.codec))
        pool.append((p.name + "_other_codec", p.data, 1 - p.codec))
    blob = b"".join(data for _, data, _ in pool)
    (tmp / "pool.bin").write_bytes(blob)
    lines, at = [], 0
    for _, data, codec in pool:
        lines.append("%s %d %d %d" % (tmp / "pool.bin", at, len(data), codec))
        at += len(data)
    (tmp / "pool.list").write_text("\n".join(lines) + "\n")
    return pool, str(tmp / "pool.list")


def _compare(lines, pool):
    at = 0
    for k, (name, data, codec) in enumerate(pool):
        w = _words(lines[at])
        at += 1
        assert w["item"] == k
        try:
            pages = G.walk(data, codec)
        except G.Refused:
            assert (w["ok"], w["pages"], w["out"]) == (0, 0, 0), name
            assert w["fate_small"] == 1, name
            continue
        total = sum(p["uncompressed_page_size"] for p in pages)
        assert (w["ok"], w["pages"], w["out"]) == (1, len(pages), total), name
        assert w["bare"] == sum(not p["flags"] & G.HAS_CRC for p in pages), name
        stored = [p["compressed_page_size"] if p["flags"] & G.VALUES_STORED else p["rep_levels_bytes"] + p["def_levels_bytes"]
                  for p in pages]
        assert w["largest"] == max(stored, default=0), name
        # a table one row short: InvalidValue; else an output one byte short: CannotDecompress
        assert w["fate_small"] == (2 if pages else 1 if total else 0), name
        for p in pages:
            assert lines[at][0] == "page" and [int(x) for x in lines[at][1:]] == [p[f] for f in G.PAGE_FIELDS], (name, p)
            at += 1
    assert at == len(lines)


def test_walk_is_the_restatements(driver, pool):
    _compare(_run(driver, "walk", pool[1]), pool[0])


@pytest.mark.parametrize("most", [1, 2])
def test_walk_taken_up_again(driver, pool, most):
    """listing walks of at most `most` pages each, every one taken up where the last stopped: the same pages"""
    _compare(_run(driver, "relist", pool[1], most), pool[0])


def test_pool_has_both_verdicts(pool):
    verdicts = set()
    for _, data, codec in pool[0]:
        try:
            verdicts.add(bool(G.walk(data, codec)) or "empty")
        except G.Refused:
            verdicts.add(False)
    assert verdicts == {True, False, "empty"}


# ---- the layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items,P", [(1, 2), (1, 1), (3, 7), (300, 2), (65, 262144), (1 << 20, 2)])
def test_layout(driver, items, P):
    lists = items * ITEM + 64
    want = lists + ENTRY * P
    w = _words(_run(driver, "layout", items, P, want + 5, 1 << 18)[0])
    assert w["entry_bytes"] == ENTRY
    assert w["items_bytes"] == w["totals_at"] == items * ITEM and w["lists_at"] == lists
    assert [w["list8_%d" % j] for j in range(LISTS8)] == [lists + 8 * P * j for j in range(LISTS8)]
    assert [w["list4_%d" % j] for j in range(LISTS4)] == [lists + 8 * P * LISTS8 + 4 * P * j for j in range(LISTS4)]
    assert w["list4_%d" % (LISTS4 - 1)] + 4 * P == w["scratch_bytes"] == want, "the last list ends where the scratch ends"
    assert w["min_scratch_bytes"] == lists + 2 * ENTRY
    assert w["pass_entries"] == (min(P, 1 << 18) if P >= 2 else 0), "P entries fit, and no more, in P entries' room + 5"
    assert w["totals_at"] % 16 == 0 and w["lists_at"] % 16 == 0 and all(w["list8_%d" % j] % 8 == 0 for j in range(LISTS8))
    assert _words(_run(driver, "layout", items, P, lists + 2 * ENTRY - 1, 100)[0])["pass_entries"] == 0
    assert _words(_run(driver, "layout", items, P, lists + 2 * ENTRY, 100)[0])["pass_entries"] == 2
    assert _words(_run(driver, "layout", items, P, lists + 1000 * ENTRY, 100)[0])["pass_entries"] == 100


# ---- the passes --------------------------------------------------------------------------------------------------
def _partition(counts, P):
    """the restatement: number the pages through the batch, cut the numbering every P"""
    owner = [i for i, c in enumerate(counts) for _ in range(c)]
    passes = []
    for lo in range(0, len(owner), P):
        part, slices = owner[lo:lo + P], []
        for at, i in enumerate(part):
            if slices and slices[-1][0] == i:
                slices[-1][2] += 1
            else:
                slices.append([i, at, 1])
        passes.append((len(part), slices))
    return passes


@pytest.mark.parametrize("name,counts,P", [
    ("no_pages", [0], 2), ("one_page", [1], 2), ("empty_items_around", [0, 3, 0], 2), ("one_item_three_passes", [5], 2),
    ("300_items_of_one_page", [1] * 300, 2), ("300_items_one_pass", [1] * 300, 512),
    ("the_passes_test", [5, 0, 1, 1, 1, 3], 2), ("exact_multiple", [2, 2], 2), ("mixed", [3, 0, 0, 4, 1, 0, 6], 4)])
def test_passes(driver, name, counts, P):
    lines = _run(driver, "passes", P, *counts)
    want = _partition(counts, P)
    assert _words(lines[0]) == {"total": sum(counts), "passes": len(want)}
    got, k = [], -1
    for ln in lines[1:]:
        w = _words(ln)
        if "item" in w:
            assert w["pass"] == k
            got[-1][1].append([w["item"], w["at"], w["count"]])
        else:
            k += 1
            assert w["pass"] == k
            got.append((w["count"], []))
    assert got == want
    for count, slices in got:
        assert sum(c for _, _, c in slices) == count <= P
        assert all(at + c <= count for _, at, c in slices)
