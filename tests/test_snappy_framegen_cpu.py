"""tests/snappy_framegen.py held to what it restates: its CRC-32C and mask to the known vectors (RFC 3720 B.4 and the
format's own), its planned streams to pyarrow's Snappy codec -- every legal one decodes to the planned bytes with
every payload decoded by pyarrow, independently of this project -- and to its own parser: every hostile one gets the
planned reason; and a census that every refusal the reader owes a status for is planned."""
import zlib

import pyarrow as pa
import pytest

import snappy_framegen as G


def _pyarrow_block(payload: bytes) -> bytes:
    pre = G.read_varint(payload, 0, len(payload))
    if pre is None:
        raise G.Refused("bad_block")
    try:
        return pa.Codec("snappy").decompress(payload, pre[0]).to_pybytes()
    except Exception:   # (pyarrow.lib.ArrowIOError: "Corrupt snappy compressed data.")
        raise G.Refused("bad_block")


def test_crc32c_vectors():
    assert G.crc32c(b"123456789") == 0xE3069283
    assert G.mask(0xE3069283) == 0xC78AB0E5
    assert G.mask(G.crc32c(b"")) == 0xA282EAD8
    assert G.crc32c(bytes(32)) == 0x8A9136AA
    assert G.crc32c(b"\xff" * 32) == 0x62A8AB43
    assert G.crc32c(bytes(range(32))) == 0x46DD794E
    assert G.crc32c(bytes(range(31, -1, -1))) == 0x113FDB5C
    assert G.SMALLEST == G.IDENTIFIER + G.stored_chunk(b"123456789") and len(G.SMALLEST) == 27


def test_mask_and_unmask():
    for c in (0, 1, 0xE3069283, 0xFFFFFFFF, 0x80000000, 0x00007FFF, 0x00008000):
        assert G.unmask(G.mask(c)) == c
    assert G.mask(0) == 0xA282EAD8


def test_long_and_batched_crc_forms_agree_with_the_bytewise_one():
    data = G.noise(70000, 1)
    for n in (4095, 4096, 4097, 65535, 65536, 70000):
        assert G.crc32c(data[:n]) == G._bytewise(G.M, data[:n]) ^ G.M, n
    pieces = [data[i * 100:i * 100 + 100] for i in range(40)] + [data[:7], b"", data[:100]]
    assert G.crc32c_many(pieces) == [G.crc32c(p) for p in pieces]


def test_the_block_writer_writes_snappy():
    codec = pa.Codec("snappy")
    for n in (0, 1, 59, 60, 61, 300, 5000, 65536):
        for data in (G.text(n, n), G.noise(n, n), bytes(n)):
            block = G.block_of(data)
            assert G.decode_block(block) == data
            assert codec.decompress(block, n).to_pybytes() == data
            # and the decoder reads the library's blocks
            assert G.decode_block(codec.compress(data).to_pybytes()) == data


@pytest.mark.parametrize("plan", G.legal_plans() + G.truncation_plans()[:2], ids=lambda p: p.name)
def test_legal_plans_decode_to_their_content_with_pyarrow(plan):
    chunks = G.parse(plan.data)
    assert len(chunks) == plan.chunks and sum(c[2] for c in chunks) == plan.declared == len(plan.content)
    for verify in (False, True):
        assert G.decode(plan.data, verify, _pyarrow_block) == ("ok", plan.content)
        assert G.decode(plan.data, verify) == ("ok", plan.content)
    assert plan.status(0) == plan.status(4) == G.SUCCESS


def test_legal_plans_cover_the_forms():
    plans = {p.name: p for p in G.legal_plans()}
    kinds = {}
    for p in plans.values():
        for kind, payload, content, _ in G.parse(p.data):
            kinds.setdefault(kind, set()).add(content)
            if kind == "compressed" and len(payload) > content > 0:
                kinds.setdefault("longer", set()).add(content)
    assert {0, 1, 65536} <= kinds["stored"] and {0, 1, 65536} <= kinds["compressed"] and kinds["longer"]
    assert set(G.MANY_LENGTHS) <= {c[2] for c in G.parse(plans["many_chunks"].data)}
    assert plans["many_chunks"].chunks >= 300
    assert plans["smallest"].data == G.SMALLEST
    types = set()
    for p in plans.values():
        at = 0
        while at < len(p.data):
            types.add(p.data[at])
            at += G.parse_chunk(p.data, at, at == 0)[1]
    assert {0x00, 0x01, 0x80, 0xfd, 0xfe, 0xff} <= types


@pytest.mark.parametrize("plan", G.hostile_plans() + G.truncation_plans()[2:], ids=lambda p: p.name)
def test_hostile_plans_get_their_planned_reason(plan):
    for verify in (False, True):
        want = plan.expected_reason(verify)
        for decoder in (G.decode_block, _pyarrow_block):
            reason, content = G.decode(plan.data, verify, decoder)
            if decoder is _pyarrow_block and want == "size_mismatch":
                assert reason in ("size_mismatch", "bad_block")   # (pyarrow does not say which)
            else:
                assert reason == want, (plan.name, verify)
            if want == "ok":
                assert content == plan.content
    assert plan.status(0) == plan.status(1) == (G.SUCCESS if plan.reason == "ok" else G.CANNOT_DECOMPRESS)
    assert plan.status(2) == plan.status(3) == plan.status(4) == (G.BAD_CHECKSUM if plan.bad_crc else G.CANNOT_DECOMPRESS)
    if plan.configures:
        chunks = G.parse(plan.data)
        assert len(chunks) == plan.chunks and sum(c[2] for c in chunks) == plan.declared
    else:
        with pytest.raises(G.Refused):
            G.parse(plan.data)


def test_the_census_of_reasons_is_complete():
    seen = set()
    for p in G.hostile_plans() + G.truncation_plans():
        seen.add(p.reason)
        if p.bad_crc:
            seen.add("bad_checksum")
    assert seen == set(G.REASONS)
    assert {p.truncated_at for p in G.truncation_plans() if p.truncated_at} == set(G.TRUNCATION_POINTS)
    names = [p.name for p in G.all_plans()]
    assert len(names) == len(set(names))
    # the wrong CRCs are the planned kinds of wrong
    plans = {p.name: p for p in G.hostile_plans()}
    t, z = G.text(500, 9), G.noise(200, 4)
    assert G.parse(plans["unmasked_crc"].data)[0][3] == G.crc32c(t)
    assert G.parse(plans["ieee_crc_masked"].data)[1][3] == G.mask(zlib.crc32(z))
    both = plans["wrong_crc_and_bad_block"]
    assert both.status(0) == G.CANNOT_DECOMPRESS and both.status(3) == G.BAD_CHECKSUM
