"""The restatement of the Parquet page rules (tests/parquet_pagegen.py: what the C++ of
hipcomp-core_amd/csrc/parquet_pages_plan.hpp and the GPU path are compared with) against what pyarrow wrote and said
when the fixtures of tests/golden/parquet_pages/ were made, and every planned chunk against the verdict it is built to
get.  Only the committed files are read: no pyarrow here."""
import os
import zlib

import pytest

import parquet_pagegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipcomp", "snappy.hpp")


def test_the_feature_is_in_the_header():
    text = open(HEADER).read()
    for word in ("enum class ParquetCodec", "struct ParquetPageInfo", "get_parquet_pages_sizes", "decompress_parquet_pages"):
        assert word in text
    assert os.path.exists(os.path.join(ROOT, "hipcomp-core_amd", "csrc", "parquet_pages_plan.hpp"))


def test_fixture_set():
    assert G.fixture_names() == ["big_page", "v1_none", "v1_snappy", "v2_snappy"]
    for name in G.fixture_names():
        assert os.path.getsize(os.path.join(G.GOLDEN, name + ".chunks")) < 65536


@pytest.mark.parametrize("name", ["big_page", "v1_none", "v1_snappy", "v2_snappy"])
def test_manifest_from_the_bytes_alone(name):
    blob, manifest = G.load_fixture(name)
    bare = [dict(offset=c["offset"], length=c["length"], codec=c["codec"], num_values=c["num_values"]) for c in manifest["chunks"]]
    assert G.manifest_of(blob, bare) == manifest["chunks"]
    # the chunks tile the file; what the issue found with pyarrow holds for every chunk
    at = 0
    for c in manifest["chunks"]:
        assert c["offset"] == at
        at += c["length"]
        chunk = blob[c["offset"]:at]
        pages = c["pages"]
        assert pages and pages[-1]["body_offset"] + pages[-1]["compressed_page_size"] == c["length"], "the walk ends at the end"
        assert sum(p["num_values"] for p in pages if p["kind"] != G.DICTIONARY_PAGE) == c["num_values"]
        out = 0
        for p in pages:
            assert p["out_offset"] == out and p["flags"] & G.HAS_CRC
            out += p["uncompressed_page_size"]
            assert zlib.crc32(chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]) == p["crc"]
            assert bool(p["flags"] & G.VALUES_STORED) == (c["codec"] == G.UNCOMPRESSED)
    assert at == len(blob)


def test_fixtures_cover_the_forms():
    kinds, levels, pages_most = {}, 0, 0
    for name in G.fixture_names():
        _, manifest = G.load_fixture(name)
        kinds[name] = {p["kind"] for c in manifest["chunks"] for p in c["pages"]}
        levels += sum(p["rep_levels_bytes"] > 0 and p["def_levels_bytes"] > 0 for c in manifest["chunks"] for p in c["pages"])
        pages_most = max(pages_most, max(len(c["pages"]) for c in manifest["chunks"]))
    assert kinds["v1_snappy"] == kinds["v1_none"] == {G.DATA_PAGE, G.DICTIONARY_PAGE}
    assert kinds["v2_snappy"] == {G.DATA_PAGE_V2, G.DICTIONARY_PAGE}
    assert levels > 0, "a V2 page with repetition and definition levels"
    assert pages_most >= 3, "a chunk of several pages"
    _, big = G.load_fixture("big_page")
    assert max(p["uncompressed_page_size"] for c in big["chunks"] for p in c["pages"]) > 2 * 65536


# ---- the planned chunks ----------------------------------------------------------------------------------------------
# name -> (status without verification, status under a verifying policy, status under ComputeAndVerify, listed pages)
S, C, B, V = G.SUCCESS, G.CANNOT_DECOMPRESS, G.BAD_CHECKSUM, G.CANNOT_VERIFY
VERDICTS = {
    "empty_chunk": (S, S, S, 0), "three_pages": (S, S, S, 3), "dictionary_alone": (S, S, S, 1), "body_cut": (C, C, C, 0),
    "varint_six_bytes": (C, C, C, 0), "varint_five_bytes": (S, S, S, 1), "negative_uncompressed": (C, C, C, 0),
    "negative_compressed": (C, C, C, 0), "negative_num_values": (C, C, C, 0), "body_one_past_the_end": (C, C, C, 0),
    "missing_field_2": (C, C, C, 0), "missing_field_1": (C, C, C, 0), "missing_kind_struct": (C, C, C, 0),
    "other_kinds_struct": (C, C, C, 0), "v2": (S, S, S, 1), "v2_says_compressed": (S, S, S, 1), "v2_not_compressed": (S, S, S, 1),
    "v2_not_compressed_other_length": (C, C, C, 0), "v2_empty_values": (S, S, S, 1), "v2_empty_values_empty_block": (S, S, S, 1),
    "v2_levels_above_compressed": (C, C, C, 0), "v2_levels_above_uncompressed": (C, C, C, 0), "v2_negative_levels": (C, C, C, 0),
    "v2_values_without_block": (C, C, C, 0), "every_wire_type": (S, S, S, 1), "every_wire_type_inside": (S, S, S, 1),
    "long_form_ids": (S, S, V, 1), "wire_type_0": (C, C, C, 0), "wire_type_13": (C, C, C, 0), "element_type_13": (C, C, C, 0),
    "i64_of_eleven_bytes": (C, C, C, 0), "i64_of_ten_bytes": (S, S, S, 1), "binary_past_the_end": (C, C, C, 0),
    "negative_list_size": (C, C, C, 0), "nesting_at_the_limit": (S, S, S, 1), "nesting_beyond_the_limit": (C, C, C, 0),
    "nesting_inside_at_the_limit": (S, S, S, 1), "nesting_inside_beyond_the_limit": (C, C, C, 0),
    "list_at_the_limit": (S, S, S, 1), "list_beyond_the_limit": (C, C, C, 0), "map_at_the_limit": (S, S, S, 1),
    "map_beyond_the_limit": (C, C, C, 0), "stepped_over_between": (S, S, S, 3), "stepped_over_alone": (S, S, S, 0),
    "stepped_over_cut": (C, C, C, 0), "no_crc": (S, S, V, 2), "wrong_crc": (S, B, B, 2), "wrong_crc_and_damaged": (C, B, B, 0),
    "preamble_one_above": (C, C, C, 0), "preamble_one_below": (C, C, C, 0), "header_one_above": (C, C, C, 0),
    "header_one_below": (C, C, C, 0), "damaged_block": (C, C, C, 0), "damaged_block_behind_good": (C, C, C, 0),
    "block_cut": (C, C, C, 0), "empty_block": (C, C, C, 0), "trailing_byte": (C, C, C, 0), "trailing_stop": (C, C, C, 0),
    "trailing_header": (C, C, C, 0), "stored_pages": (S, S, S, 2), "stored_v2": (S, S, S, 1), "stored_other_length": (C, C, C, 0),
    "stored_empty_page": (S, S, S, 1), "stored_wrong_crc": (S, B, B, 1),
}


def test_every_plan_has_a_verdict():
    names = [p.name for p in G.all_plans()]
    cuts = [n for n in names if n.startswith("cut_")]
    assert sorted(n for n in names if not n.startswith("cut_")) == sorted(VERDICTS)
    one = G.make_page(G.DATA_PAGE, G.snappy_literals(bytes(range(40))), 40)
    assert len(cuts) == len(one) - len(G.snappy_literals(bytes(range(40)))), "the header cut at every byte"
    assert all(len(p.data) < 1024 for p in G.all_plans())


@pytest.mark.parametrize("plan", G.all_plans(), ids=lambda p: p.name)
def test_planned_chunk(plan):
    want = (C, C, C, 0) if plan.name.startswith("cut_") else VERDICTS[plan.name]
    for policy in range(5):
        status, out, pages = plan.result(policy)
        expect = want[0] if policy < 2 else want[2] if policy == 4 else want[1]
        assert status == expect, (plan.name, policy)
        if status in (S, V):
            assert len(pages) == want[3] and len(out) == sum(p["uncompressed_page_size"] for p in pages)
        else:
            assert out == b"" and pages == []
    # the capacities: one byte or one row short
    status, out, pages = plan.result(0)
    if status == S and out:
        assert plan.result(0, capacity=len(out))[0] == S and plan.result(0, capacity=len(out) - 1)[0] == C
    if status == S and pages:
        assert plan.result(0, table_capacity=len(pages))[0] == S
        assert plan.result(0, capacity=0, table_capacity=len(pages) - 1)[0] == G.INVALID_VALUE


def test_what_the_good_plans_decode_to():
    plans = {p.name: p for p in G.all_plans()}
    text, ramp = b"The walk of Thrift page headers on the device. " * 3, bytes(range(40))
    levels = bytes([3, 0, 0, 0, 5, 9, 2, 1, 1])
    assert plans["three_pages"].result(4)[1] == text + ramp * 9 + ramp
    assert plans["stepped_over_between"].result(4)[1] == text + ramp * 9 + ramp
    assert plans["v2"].result(4)[1] == levels + ramp * 9
    assert plans["v2_not_compressed"].result(4)[1] == levels + text
    assert plans["v2_empty_values"].result(4)[1] == plans["v2_empty_values_empty_block"].result(4)[1] == levels
    assert plans["stored_pages"].result(4)[1] == text + ramp
    assert plans["no_crc"].result(4)[0] == V and plans["no_crc"].result(4)[1] == text + ramp * 9
    rows = plans["v2"].result(0)[2]
    assert (rows[0]["num_nulls"], rows[0]["num_rows"], rows[0]["def_levels_bytes"], rows[0]["rep_levels_bytes"]) == (1, 4, 3, 6)
    assert len(G.page_row(rows[0])) == 72, "a ParquetPageInfo"


def test_snappy_writer_and_reader():
    for data in (b"", b"a", bytes(range(200)), b"xyz" * 100):
        assert G.snappy_decode(G.snappy_literals(data)) == data
    assert G.snappy_decode(G.snappy_repeat(b"abcdefg", 30)) == b"abcdefg" * 30
    with pytest.raises(ValueError):
        G.snappy_decode(G.snappy_repeat(b"abcdefg", 30)[:-1])
