"""The arithmetic and the rules of a decode of Parquet RLE / bit-packed hybrid streams
(hipcomp-core_amd/csrc/parquet_hybrid_plan.hpp: decode_parquet_hybrid of the Cascaded manager -- the one copy the kernel
and the host share).  tests/parquet_hybrid_plan_driver.cpp, a program of its own, decodes every fixture stream and every
planned stream in a buffer of exactly its length into a buffer of exactly its capacity; it is compiled with g++ under
the address and undefined-behaviour sanitizers, without HIP, and held to the restatement of tests/parquet_hybridgen.py
value for value and verdict for verdict.  The restatement itself is held to what the fixtures say their streams hold:
the table pyarrow was given."""
import os
import struct
import subprocess

import pytest

import parquet_hybridgen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
LETTER = {1: "B", 2: "H", 4: "I"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("parquet_hybrid_plan") / "parquet_hybrid_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "parquet_hybrid_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def pages():
    return G.fixture_pages()


def _pool(pages):
    """every fixture stream, every planned stream, and every planned stream one value short of its capacity"""
    pool = [p for _, levels, _, indices, _ in pages for p in (levels, indices)] + G.all_plans()
    pool += [G.Plan(p.name + "_capacity_short", p.data, p.wanted, p.bit_width, p.form, p.element, p.match, "S")
             for p in G.all_plans() if p.wanted and p.cap == "E"]
    return pool


@pytest.fixture(scope="module")
def decoded(driver, pages, tmp_path_factory):
    """[(plan, the driver's words, its output bytes)]"""
    tmp = tmp_path_factory.mktemp("parquet_hybrid_pool")
    pool = _pool(pages)
    (tmp / "pool.bin").write_bytes(b"".join(p.data for p in pool))
    lines, at = [], 0
    for p in pool:
        lines.append("%s %d %d %d %d %d %d %d %d" % (tmp / "pool.bin", at, len(p.data), p.form, p.bit_width, p.wanted, p.capacity(),
                                                     p.element, p.match))
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
        status, want, consumed, matches = p.model()
        assert w["ok"] == (status == G.SUCCESS), p.name
        assert (w["consumed"], w["matches"], w["size"]) == (consumed, matches, p.wanted if status == G.SUCCESS else 0), p.name
        assert out == want, p.name
        assert w["untouched"] == 1, ("an element outside the wanted ones, or one of a refused item, was written", p.name)


def test_the_pool_has_both_verdicts_of_every_form_and_element(decoded):
    seen = {(p.form, p.element, w["ok"]) for p, w, _ in decoded}
    assert seen >= {(form, element, ok) for form in (G.BARE, G.LENGTH_PREFIXED, G.WIDTH_PREFIXED)
                    for element in (G.UCHAR, G.USHORT, G.UINT) for ok in (0, 1)}
    widths = {p.bit_width for p, w, _ in decoded if w["ok"] and p.form != G.WIDTH_PREFIXED}
    assert widths >= {0, 1, 7, 8, 9, 16, 17, 24, 25, 31, 32}


def test_the_restatement_reads_what_pyarrow_was_given(pages):
    """levels, then indices with the levels' count of ones: the fixtures' values, pinned to the table when they were made"""
    assert len(pages) >= 24
    widths, kinds = set(), set()
    for name, levels, want_levels, indices, want_indices in pages:
        status, out, consumed, matches = levels.model()
        assert status == G.SUCCESS and list(out) == want_levels and consumed == len(levels.data), name
        assert matches == len(want_indices) == indices.wanted, "the count of ones is the index stream's num_values"
        status, out, consumed, matches = indices.model()
        assert status == G.SUCCESS and consumed == len(indices.data), name
        assert list(struct.unpack("<%d%s" % (indices.wanted, LETTER[indices.element]), out)) == want_indices, name
        assert matches == want_indices.count(indices.match)
        widths.add(indices.data[0])
        for p in (levels, indices):
            pos = {G.BARE: 0, G.LENGTH_PREFIXED: 4, G.WIDTH_PREFIXED: 1}[p.form]
            width = p.data[0] if p.form == G.WIDTH_PREFIXED else 1
            while pos < len(p.data):
                h, pos = G.read_header(p.data, pos, len(p.data))
                kinds.add((p.form, h & 1))
                pos += (h >> 1) * width if h & 1 else (width + 7) // 8
    assert widths >= {1, 2, 6, 9, 11, 12}
    assert kinds == {(form, kind) for form in (G.BARE, G.LENGTH_PREFIXED, G.WIDTH_PREFIXED) for kind in (0, 1)}, "both run kinds"


def test_a_refused_item_of_the_restatement_has_nothing(pages):
    refused = [p for p in G.all_plans() if p.model()[0] != G.SUCCESS]
    assert len(refused) >= 40
    assert all(p.model() == (G.CANNOT_DECOMPRESS, b"", 0, 0) for p in refused)
