"""The gzip / zlib / BGZF entry points (include/hipcomp/gzip.h, lib/libhipcomp_gzip.so) on the GPU.  The arbiter is
zlib: a member is right exactly when zlib.decompressobj(31) (gzip, BGZF) or zlib.decompressobj(15) (zlib) returns
the chunk with `eof` set and nothing left over; a decode succeeds exactly where zlib does.  Every buffer of the
byte-level tests lies in decode_guard.GuardedSlots."""
import gzip
import random
import struct
import zlib

import pytest

import deflate_streamgen as G
import gzip_membergen as M
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu

WRAPPERS = {"gzip": M.GZIP, "zlib": M.ZLIB, "bgzf": M.BGZF}
EXTRA = {"gzip": 18, "zlib": 6, "bgzf": 26}
LIMIT = {"gzip": 65536, "zlib": 65536, "bgzf": 65280}
SIZES = (0, 1, 4, 63, 64, 65, 258, 4095, 32768, 65535, 65536)
EDGES = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 5551, 5552, 5553, 65535, 65536)
OK, CANNOT, BAD = M.OK, M.CANNOT, M.BAD_CHECKSUM


def raw_bound(n: int) -> int:
    return n + 5 * max(1, -(-n // 65535))


def bench_text(n: int) -> bytes:
    import bench
    return bench.gen_text(n).tobytes()


_inputs = {}


def inputs():
    """the raw encoder test's kinds (tests/test_deflate_compress_gpu.py), built once"""
    if not _inputs:
        size = 65536
        rnd = random.Random(5)

        def period(p):
            unit = bytes(rnd.randrange(256) for _ in range(p))
            return (unit * (2 * size // p + 2))[:size]
        _inputs.update({
            "empty": b"", "one_byte": b"x", "text": G._text(size, 17), "tpch_text": bench_text(size),
            "random": rnd.randbytes(size), "zeros": bytes(size),
            "period_1": period(1), "period_2": period(2), "period_3": period(3), "period_255": period(255),
            "period_32768": period(32768)})
    return _inputs


def cases(limit: int):
    """[(name, bytes)], distinct"""
    seen, out = set(), []
    for name, data in inputs().items():
        for size in SIZES:
            cut = data[:min(size, limit)]
            if (name, len(cut)) not in seen:
                seen.add((name, len(cut)))
                out.append((f"{name}_{len(cut)}", cut))
    return out


def compress_guarded(hc, torch, dev, wrapper, chunks, max_chunk, offsets=(0,), turn=0):
    """-> (members, sizes): every chunk compressed inside guarded slots; containment is asserted here"""
    n = len(chunks)
    cap = raw_bound(max_chunk) + EXTRA[wrapper]
    codec = hc.batch.GzipCodec(wrapper)
    assert codec.max_output_chunk_size(max_chunk) == cap
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=offsets, turn=turn, seed=31, chunks=chunks)
    dst = GuardedSlots(torch, [cap] * n, dev, offsets=offsets, turn=turn + 3, seed=32)
    temp = torch.empty(max(codec.compress_temp_size(n, max_chunk), 8), dtype=torch.uint8, device=dev)
    out_batch = dst.batch(hc)
    out_batch.sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    assert codec.compress_async(src.batch(hc), max_chunk, temp, out_batch) == 0
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()                      # the input is only read
    got = dst.after()
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)   # nothing at or beyond out_i + bound
    sizes = out_batch.sizes.cpu().tolist()
    return [dst.slot_bytes(got, i, max(sizes[i], 0)) for i in range(n)], sizes


def decode_guarded(hc, torch, dev, wrapper, members, caps, offsets=(0,), turn=0, with_actual=True, with_statuses=True):
    """-> (dst slots, arena bytes after, actual, statuses, sizes of the size query); the input is asserted unread"""
    n = len(members)
    codec = hc.batch.GzipCodec(wrapper)
    src = GuardedSlots(torch, [len(m) for m in members], dev, offsets=offsets, turn=turn, seed=33, chunks=members)
    dst = GuardedSlots(torch, caps, dev, offsets=offsets, turn=turn + 3, seed=34)
    actual = torch.full((n,), -1, dtype=torch.int64, device=dev) if with_actual else None
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev) if with_statuses else None
    temp = torch.empty(max(codec.decompress_temp_size(n, max(caps + [0])), 8), dtype=torch.uint8, device=dev)
    assert codec.decompress_async(src.batch(hc), dst.caps_t, actual, temp, dst.batch(hc), statuses) == 0
    sizes = codec.get_decompress_size(src.batch(hc))
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()
    return (dst, dst.after(), None if actual is None else actual.cpu().tolist(),
            None if statuses is None else statuses.cpu().tolist(), sizes.cpu().tolist())


def check_decode(hc, torch, dev, wrapper, named, **kw):
    """named: [(name, member, expected)]: all succeed with the expected bytes, nothing else is touched"""
    caps = [len(e) for _, _, e in named]
    dst, got, actual, statuses, sizes = decode_guarded(hc, torch, dev, wrapper, [m for _, m, _ in named], caps, **kw)
    for i, (name, _, want) in enumerate(named):
        assert statuses[i] == OK, (name, statuses[i])
        assert actual[i] == len(want) and sizes[i] == len(want), (name, actual[i], sizes[i], len(want))
        assert dst.slot_bytes(got, i, len(want)) == want, name
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_compress_is_what_zlib_reads_at_every_byte_offset(hc, cuda, wrapper):
    import torch
    w, limit = WRAPPERS[wrapper], LIMIT[wrapper]
    named = cases(limit)
    assert len(named) >= 80
    offsets = tuple(range(16))
    for turn in range(16):   # chunk i at input offset (i + turn) % 16 and output offset (i + turn + 3) % 16
        members, sizes = compress_guarded(hc, torch, cuda, wrapper, [d for _, d in named], limit, offsets=offsets, turn=turn)
        for (name, data), m, s in zip(named, members, sizes):
            assert 0 < s <= raw_bound(len(data)) + EXTRA[wrapper], (name, s)
            assert M.arbiter(m, w) == data, name
            if wrapper == "bgzf":
                assert m[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), name
                assert struct.unpack_from("<H", m, 16)[0] == len(m) - 1, name
        if wrapper == "bgzf" and turn == 0:
            assert gzip.decompress(b"".join(members) + hc.api.BGZF_EOF_BLOCK) == b"".join(d for _, d in named)
            whole = b"".join(members) + hc.api.BGZF_EOF_BLOCK
            offs, stopped = hc.api.gzip_library().bgzf_split(whole)
            assert stopped == len(whole) and len(offs) == len(members) + 1


def test_payload_is_the_raw_encoders_stream(hc, cuda):
    import torch
    for wrapper, (lead, trail) in (("gzip", (10, 8)), ("zlib", (2, 4)), ("bgzf", (18, 8))):
        named = cases(LIMIT[wrapper])[::2]
        chunks = [d for _, d in named]
        members, _ = compress_guarded(hc, torch, cuda, wrapper, chunks, LIMIT[wrapper], offsets=(0, 5, 11))
        raw = hc.batch.DeflateEncoder().compress(hc.batch.from_host_chunks(chunks, cuda), LIMIT[wrapper])
        torch.cuda.synchronize()
        for (name, _), m, s in zip(named, members, raw.to_host_chunks()):
            assert m[lead:len(m) - trail] == s, (wrapper, name)
        fixed = bytes.fromhex({"gzip": "1f8b08000000000000ff", "zlib": "7801", "bgzf": "1f8b08040000000000ff060042430200"}[wrapper])
        assert all(m[:len(fixed)] == fixed for m in members), wrapper


def test_a_chunk_above_the_calls_chunk_size_gets_no_bytes(hc, cuda):
    import torch
    for wrapper in WRAPPERS:
        chunks = [b"a" * 100, b"b" * 101, b"", b"c" * 300]
        members, sizes = compress_guarded(hc, torch, cuda, wrapper, chunks, 100)
        assert sizes[1] == 0 and sizes[3] == 0 and sizes[0] > 0 and sizes[2] > 0
        assert M.arbiter(members[0], WRAPPERS[wrapper]) == chunks[0] and M.arbiter(members[2], WRAPPERS[wrapper]) == b""
        # and nothing at all was written for the two (their whole slots still hold the guard pattern)
        n = len(chunks)
        cap = raw_bound(100) + EXTRA[wrapper]
        codec = hc.batch.GzipCodec(wrapper)
        src = hc.batch.from_host_chunks(chunks, cuda)
        dst = GuardedSlots(torch, [cap] * n, cuda, seed=35, region=[cap, 0, cap, 0])
        out = dst.batch(hc)
        out.sizes = torch.full((n,), -1, dtype=torch.int64, device=cuda)
        temp = torch.empty(max(codec.compress_temp_size(n, 100), 8), dtype=torch.uint8, device=cuda)
        assert codec.compress_async(src, 100, temp, out) == 0
        torch.cuda.synchronize()
        assert dst.first_guard_change() is None, dst.first_guard_change()


def zlib_made(wrapper: int):
    """[(name, member, chunk)]: members at zlib's levels, every legal header form, planned streams wrapped by hand"""
    out = []
    kinds = inputs()
    for kind in ("empty", "one_byte", "text", "random", "zeros", "period_255"):
        data = kinds[kind]
        for level in (0, 1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, M.WBITS[wrapper])
            out.append((f"{kind}_level_{level}", c.compress(data) + c.flush(), data))
    text = kinds["text"][:3000]
    if wrapper == M.ZLIB:
        out += [(f"flevel_{f}_cinfo_{c}", M.zlib_member(text, flevel=f, cinfo=c, level=0), text)
                for f in range(4) for c in (7, 0)]
    else:
        out += [(name, M.gzip_member(text, **kw), text) for name, kw in M.legal_gzip_headers()]
        out.append(("bgzf_block", M.bgzf_block(text), text))
        out.append(("bgzf_eof", M.BGZF_EOF, b""))
    out += [(name, M.wrap(wrapper, want, s), want) for name, s, want in G.legal_plans() if not has_slack(s)]
    return out


def has_slack(stream: bytes) -> bool:
    """bytes behind the final block: wrapped, zlib looks for the trailer there (the documented difference)"""
    d = zlib.decompressobj(-15)
    d.decompress(stream)
    return d.unused_data != b""


def test_slack_behind_the_final_block_is_the_documented_difference(hc, cuda):
    """the trailer is taken from the chunk's last bytes and the raw decoder ignores what lies behind its final
    block: such a member decodes here, with its checksum verified, where zlib refuses it"""
    import torch
    slack = [(name, s, want) for name, s, want in G.legal_plans() if has_slack(s)]
    assert slack
    for wrapper in ("gzip", "zlib"):
        named = [(name, M.wrap(WRAPPERS[wrapper], want, s), want) for name, s, want in slack]
        assert all(M.arbiter(m, WRAPPERS[wrapper]) is None for _, m, _ in named)
        check_decode(hc, torch, cuda, wrapper, named)
        wrong = [flip(m, len(m) - 1) for _, m, _ in named]
        _, _, actual, statuses, _ = decode_guarded(hc, torch, cuda, wrapper, wrong, [len(w) for _, _, w in named])
        assert statuses == [BAD] * len(named) and actual == [0] * len(named)


@pytest.mark.parametrize("wrapper", ["gzip", "zlib"])
def test_decode_of_members_zlib_made_at_every_byte_offset(hc, cuda, wrapper):
    import torch
    named = zlib_made(WRAPPERS[wrapper])
    for name, m, want in named:
        assert M.arbiter(m, WRAPPERS[wrapper]) == want, name
    offsets = tuple(range(16))
    small = [c for c in named if len(c[2]) <= 4096]
    large = [c for c in named if len(c[2]) > 4096]
    assert len(small) >= 40 and len(large) >= 16
    for turn in range(16):   # member i at input offset (i + turn) % 16 and output offset (i + turn + 3) % 16
        check_decode(hc, torch, cuda, wrapper, small, offsets=offsets, turn=turn)
    for turn in (0, 9):      # (the large ones, 16 of them or more, meet every offset in one turn)
        check_decode(hc, torch, cuda, wrapper, large, offsets=offsets, turn=turn)
    if wrapper == "gzip":   # on decode BGZF is accepted and means gzip
        check_decode(hc, torch, cuda, "bgzf", named, offsets=offsets, turn=5)


def edge_members(wrapper: int):
    rnd = random.Random(1952)
    big = (1 << 20) + 3
    ff, noise = b"\xff" * big, rnd.randbytes(big)
    out = []
    for kind, data in (("ff", ff), ("random", noise)):
        for n in EDGES + (big,):
            chunk = data[:n]
            c = zlib.compressobj(0, zlib.DEFLATED, M.WBITS[wrapper])   # stored blocks: the decoder copies
            out.append((f"{kind}_{n}", c.compress(chunk) + c.flush(), chunk))
    return out


@pytest.mark.parametrize("wrapper", ["gzip", "zlib"])
def test_checksum_edges(hc, cuda, wrapper):
    """status 0 means the kernel's CRC-32 / Adler-32 is zlib's: all-0xFF data (the largest sums) and random data at
    the sizes where a lane's segment, the 5552-byte reduction and the 16-byte blocks begin and end"""
    import torch
    named = edge_members(WRAPPERS[wrapper])
    assert len(named) == 2 * 17
    for turn in (0, 1):   # two alignments of every chunk: 16-byte aligned and 7 bytes behind it
        check_decode(hc, torch, cuda, wrapper, named, offsets=(0, 7), turn=turn)


def flip(member: bytes, at: int, bit: int = 0) -> bytes:
    b = bytearray(member)
    b[at] ^= 1 << bit
    return bytes(b)


def damaged(wrapper: int):
    """[(name, member)]: one bit flipped in the trailer's words, in a literal of a stored block, in the Huffman
    payload and in every header field, and every prefix of a 40-byte member"""
    text = G._text(600, 3)
    out = []
    if wrapper == M.ZLIB:
        stored, coded = M.zlib_member(b"stored literal bytes" * 3, level=0), M.zlib_member(text)
        header_len, fields = 2, {"cmf": 0, "flg": 1}
        small = M.zlib_member(bytes(range(29)), level=0)
        words = {"adler": range(-4, 0)}
    else:
        stored = M.gzip_member(b"stored literal bytes" * 3, level=0)
        coded = M.gzip_member(text, flg=M.FEXTRA | M.FNAME | M.FCOMMENT | M.FHCRC, xlen=4)
        header_len = 10
        fields = {"id1": 0, "id2": 1, "cm": 2, "flg": 3, "mtime": 5, "xfl": 8, "os": 9}
        small = M.gzip_member(bytes(range(17)), level=0)
        words = {"crc": range(-8, -4), "isize": range(-4, 0)}
    assert len(small) == 40
    for base_name, base in (("stored", stored), ("coded", coded)):
        for word, where in words.items():
            for k, at in enumerate(where):
                out.append((f"{base_name}_{word}_byte{k}", flip(base, len(base) + at, (3 * k + 1) % 8)))
        for field, at in fields.items():
            for bit in range(8):
                out.append((f"{base_name}_{field}_bit{bit}", flip(base, at, bit)))
    for at in (header_len + 5, header_len + 20, len(stored) - len(words) * 4 - 1):
        out.append((f"stored_literal_at_{at}", flip(stored, at, 2)))
    if wrapper != M.ZLIB:   # the optional fields of the coded member: XLEN, the extra bytes, name, comment, FHCRC
        end = M.header_model(coded, wrapper)[1]
        for at in range(10, end):
            out.append((f"coded_header_byte_{at}", flip(coded, at, at % 8)))
    start = M.header_model(coded, wrapper)[1]
    for at in range(start, len(coded) - M.TRAILER[wrapper], 7):
        out.append((f"coded_payload_byte_{at}", flip(coded, at, at % 8)))
    out += [(f"prefix_{k}", small[:k]) for k in range(40)]
    return out, (stored, coded, small)


@pytest.mark.parametrize("wrapper", ["gzip", "zlib"])
def test_damage(hc, cuda, wrapper):
    import torch
    w = WRAPPERS[wrapper]
    bad, goods = damaged(w)
    assert len(bad) >= 100
    good = goods[1]
    want_good = M.arbiter(good, w)
    cap = 1000
    members, expect = [good], [(OK, want_good)]
    for name, m in bad:   # each damaged member between two good neighbours
        members += [m, good]
        expect += [M.status_model(m, w, cap), (OK, want_good)]
    dst, got, actual, statuses, sizes = decode_guarded(hc, torch, cuda, wrapper, members, [cap] * len(members), offsets=(0, 3, 9, 14))
    seen = set()
    for i, (st, data) in enumerate(expect):
        name = "good" if i % 2 == 0 else bad[i // 2][0]
        # success exactly where zlib succeeds (no case of the suite has slack behind its final block)
        assert (st == OK) == (M.arbiter(members[i], w) is not None), name
        assert statuses[i] == st, (name, statuses[i], st)
        assert actual[i] == (len(data) if st == OK else 0), (name, actual[i])
        if st == OK:
            assert dst.slot_bytes(got, i, len(data)) == data, name
        seen.add(st)
    assert seen == {OK, CANNOT, BAD}
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    by_name = {name: statuses[2 * k + 1] for k, (name, _) in enumerate(bad)}
    assert all(by_name[n] == BAD for n in by_name if "_crc_" in n or "_isize_" in n or "_adler_" in n or "stored_literal" in n)
    assert all(by_name[f"prefix_{k}"] == CANNOT for k in range(40))


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
@pytest.mark.parametrize("n", [1, 7, 1000, 20000])
def test_round_trip_on_the_device(hc, cuda, n, wrapper):
    """n chunks drawn from 60 distinct inputs, laid out on the device by a gather, compressed, decoded and compared
    on the device (as tests/test_deflate_compress_gpu.py does for the raw calls)"""
    import torch
    pool = [d for d in inputs().values() if len(d) >= 65536]
    kinds = [d[97 * j: 97 * j + size] for d in pool for j, size in enumerate((6, 63, 258, 1000, 2000, 3000, 17))][:57]
    kinds += [b"", b"q", b"abc"]
    k = len(kinds)
    assert k == 60 and len(set(kinds)) == k
    cap = max(len(d) for d in kinds)
    table = hc.batch.from_host_chunks(kinds, cuda, stride=cap)
    pick = (torch.arange(n, device=cuda) * 7 + torch.arange(n, device=cuda) // k) % k
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, n, table.stride), table.sizes[pick], table.stride)
    before = data.clone()
    codec = hc.batch.GzipCodec(wrapper)
    comp = codec.compress(src, cap)
    dec, actual, statuses = codec.decompress(comp, cap)
    sizes = codec.get_decompress_size(comp)
    torch.cuda.synchronize()
    assert torch.equal(data, before)
    assert bool((statuses == 0).all())
    assert torch.equal(actual, src.sizes) and torch.equal(sizes, src.sizes)
    assert bool((comp.sizes > 0).all()) and bool((comp.sizes <= src.sizes + 5 + EXTRA[wrapper]).all())
    got = dec.data[: n * dec.stride].view(n, dec.stride)[:, :cap]
    exp = data.view(n, table.stride)[:, :cap]
    inside = torch.arange(cap, device=cuda)[None, :] < src.sizes[:, None]
    assert bool(((got == exp) | ~inside).all())


@pytest.mark.parametrize("wrapper", ["gzip", "zlib"])
def test_graph_capture(hc, cuda, wrapper):
    """one compress and one decompress call captured, replayed twice onto cleared output: the direct calls' results"""
    import torch
    named = cases(65536)[::7]
    chunks = [d for _, d in named]
    n = len(chunks)
    src = hc.batch.from_host_chunks(chunks, cuda)
    codec = hc.batch.GzipCodec(wrapper)
    want = codec.compress(src, 65536)
    torch.cuda.synchronize()
    want_members = want.to_host_chunks()
    for (name, d), m in zip(named, want_members):
        assert M.arbiter(m, WRAPPERS[wrapper]) == d, name
    comp = hc.batch.alloc_batch(n, codec.max_output_chunk_size(65536), cuda, fill=0xEE)
    dst = hc.batch.alloc_batch(n, 65536, cuda, fill=0xEE)
    caps = torch.full((n,), 65536, dtype=torch.int64, device=cuda)
    actual = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    ctemp = torch.empty(max(codec.compress_temp_size(n, 65536), 8), dtype=torch.uint8, device=cuda)
    dtemp = torch.empty(max(codec.decompress_temp_size(n, 65536), 8), dtype=torch.uint8, device=cuda)

    def both():
        assert codec.compress_async(src, 65536, ctemp, comp) == 0
        assert codec.decompress_async(comp, caps, actual, dtemp, dst, statuses) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()   # warm: the code objects are loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both()
    for _ in range(2):
        for t in (comp.data, dst.data):
            t.fill_(0xEE)
        for t in (comp.sizes, actual, statuses):
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert comp.to_host_chunks() == want_members
        assert statuses.cpu().tolist() == [OK] * n
        assert actual.cpu().tolist() == [len(c) for c in chunks]
        for i, c in enumerate(chunks):
            assert dst.chunk_bytes(i, len(c)) == c, named[i][0]


def test_null_actual_and_null_statuses(hc, cuda):
    import torch
    data = G._text(5000, 2)
    for wrapper, member in (("gzip", M.gzip_member(data, flg=M.FNAME)), ("zlib", M.zlib_member(data))):
        members = [member, flip(member, len(member) - 1), member]
        for with_actual, with_statuses in ((False, True), (True, False), (False, False)):
            dst, got, actual, statuses, _ = decode_guarded(
                hc, torch, cuda, wrapper, members, [len(data)] * 3, with_actual=with_actual, with_statuses=with_statuses)
            assert dst.slot_bytes(got, 0, len(data)) == data and dst.slot_bytes(got, 2, len(data)) == data
            assert dst.first_guard_change(got) is None
            if with_actual:
                assert actual == [len(data), 0, len(data)]
            if with_statuses:
                assert statuses == [OK, BAD, OK]
