"""The batched Deflate encoder (include/hipcomp/deflate_compress.h, lib/libhipcomp_deflate_compress.so) on the GPU.
The arbiter is zlib: a chunk's stream is right exactly when zlib.decompressobj(-15) returns the chunk with `eof` set
and nothing left over -- and when this library's own decoder returns it too.  Every buffer of the byte-level tests
lies in decode_guard.GuardedSlots, so a read-modify-write of the input or a byte written at or beyond the output
bound is seen."""
import random
import struct
import zlib

import pytest

import deflate_streamgen as G
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu

MAX_CHUNK = 65536
SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 260, 4095, 32767, 32768, 32769, 65535, 65536)


def bound(n: int) -> int:
    return n + 5 * max(1, -(-n // 65535))


def bench_text(n: int) -> bytes:
    import bench
    return bench.gen_text(n).tobytes()


def inputs(size=65536):
    """the twelve kinds of tests/test_deflate_gpu.py's inputs(), built here"""
    rnd = random.Random(5)
    ints = sorted(rnd.randrange(-2 ** 31, 2 ** 31) for _ in range(size // 4))

    def period(p):
        unit = bytes(rnd.randrange(256) for _ in range(p))
        return (unit * (2 * size // p + 2))[:max(size, 2 * p + 100)]
    return {
        "empty": b"", "one_byte": b"x", "text": G._text(size, 17), "tpch_text": bench_text(size),
        "random": rnd.randbytes(size), "zeros": bytes(size),
        "sorted_int32": struct.pack(f"<{len(ints)}i", *ints),
        "period_1": period(1), "period_2": period(2), "period_3": period(3), "period_255": period(255),
        "period_32768": period(32768),
    }


def match_edges():
    rnd = random.Random(1951)
    unit = rnd.randbytes(300)
    out = {}
    for d in (1, 2):
        out[f"repeat_at_distance_{d}"] = rnd.randbytes(40) + (rnd.randbytes(d) * 400)[:700] + rnd.randbytes(40)
    # (32769 must not be used: inflate refuses a distance beyond the window.  The filler is one long run: its
    # matches leave the table slots of the unit's positions alone)
    for d in (32767, 32768, 32769):
        out[f"repeat_at_distance_{d}"] = unit + bytes(d - 300) + unit + rnd.randbytes(20)
    out["match_runs_to_the_chunks_end"] = unit + rnd.randbytes(500) + unit[:100]
    out["match_would_pass_the_chunks_end"] = rnd.randbytes(100) + bytes(7) * 30 + b"\x07" * 301
    out["repeat_of_258"] = unit[:259] + rnd.randbytes(100) + unit[:258] + rnd.randbytes(50)
    out["repeat_of_259"] = unit[:259] + rnd.randbytes(100) + unit[:259] + rnd.randbytes(50)
    assert all(len(v) <= MAX_CHUNK for v in out.values())
    return out


def cases():
    """[(name, bytes)], distinct"""
    seen, out = set(), []
    for name, data in inputs().items():
        for size in SIZES:
            cut = data[:size]
            if (name, len(cut)) not in seen:
                seen.add((name, len(cut)))
                out.append((f"{name}_{len(cut)}", cut))
    return out + list(match_edges().items())


def inflate(stream: bytes):
    d = zlib.decompressobj(-15)
    got = d.decompress(stream)
    return got, d.eof, d.unused_data


def compress_guarded(hc, torch, dev, chunks, max_chunk=MAX_CHUNK, offsets=(0,), turn=0):
    """-> (streams, sizes): every chunk compressed inside guarded slots, the temp space -- exactly the size the
    library asks for -- in one too; containment is asserted here"""
    n = len(chunks)
    cap = bound(max_chunk)
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=offsets, turn=turn, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, [cap] * n, dev, offsets=offsets, turn=turn + 3, seed=22)
    enc = hc.batch.DeflateEncoder()
    temp_size = enc.compress_temp_size(n, max_chunk)
    temp = GuardedSlots(torch, [temp_size], dev, seed=23)
    at = int(temp.at[0])
    out_batch = dst.batch(hc)
    out_batch.sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    assert enc.compress_async(src.batch(hc), max_chunk, temp.data[at:at + temp_size], out_batch) == 0
    torch.cuda.synchronize()
    assert temp.first_guard_change() is None, temp.first_guard_change()      # every wave stays in its token buffer
    assert src.unchanged() is None, src.unchanged()                      # the input is only read
    got = dst.after()
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)   # nothing at or beyond out_i + bound
    sizes = out_batch.sizes.cpu().tolist()
    for c, s in zip(chunks, sizes):
        assert 0 < s <= bound(len(c)), (len(c), s)
    return [dst.slot_bytes(got, i, sizes[i]) for i in range(n)], sizes


def check_round_trip(named, streams):
    for (name, data), s in zip(named, streams):
        got, eof, unused = inflate(s)
        assert eof and unused == b"" and got == data, name   # (nothing unused: the size is the stream's, not more)


def test_round_trip_by_zlib_at_every_byte_offset(hc, cuda):
    import torch
    named = cases()
    assert len(named) >= 150
    offsets = tuple(range(16))
    for turn in range(16):   # chunk i at input offset (i + turn) % 16 and output offset (i + turn + 3) % 16
        streams, _ = compress_guarded(hc, torch, cuda, [d for _, d in named], offsets=offsets, turn=turn)
        check_round_trip(named, streams)


def test_far_repeat_is_found_only_inside_the_window(hc, cuda):
    """distance 32768 is used (the chunk shrinks by most of the repeated unit), 32769 is not"""
    import torch
    e = match_edges()
    names = ["repeat_at_distance_32767", "repeat_at_distance_32768", "repeat_at_distance_32769"]
    streams, sizes = compress_guarded(hc, torch, cuda, [e[n] for n in names])
    check_round_trip([(n, e[n]) for n in names], streams)
    # (the unit is 300 random bytes: as literals a second time they cost some 300 bytes more than as two matches)
    print("repeat at 32767 / 32768 / 32769:", sizes)
    assert sizes[0] < sizes[2] - 200 and sizes[1] < sizes[2] - 200


@pytest.mark.parametrize("n", [1, 7, 1000, 100000])
def test_round_trip_on_the_device(hc, cuda, n):
    """n chunks drawn from about 60 distinct inputs, laid out on the device by a gather, compressed, decoded by
    DeflateDecoder and compared on the device"""
    import torch
    pool = [d for d in inputs().values() if len(d) >= 65536]
    kinds = [d[97 * j: 97 * j + size] for d in pool for j, size in enumerate((6, 63, 258, 1000, 2000, 3000))][:57]
    kinds += [b"", b"q", b"abc"]
    k = len(kinds)
    assert k == 60 and len(set(kinds)) == k
    cap = max(len(d) for d in kinds)
    table = hc.batch.from_host_chunks(kinds, cuda, stride=cap)
    pick = (torch.arange(n, device=cuda) * 7 + torch.arange(n, device=cuda) // k) % k
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, n, table.stride), table.sizes[pick], table.stride)
    before = data.clone()
    comp = hc.batch.DeflateEncoder().compress(src, cap)
    dec, actual, statuses = hc.batch.DeflateDecoder().decompress(comp, cap)
    torch.cuda.synchronize()
    assert torch.equal(data, before)
    assert bool((statuses == 0).all())
    assert torch.equal(actual, src.sizes)
    assert bool((comp.sizes > 0).all()) and bool((comp.sizes <= src.sizes + 5).all())
    got = dec.data[: n * dec.stride].view(n, dec.stride)[:, :cap]
    exp = data.view(n, table.stride)[:, :cap]
    inside = torch.arange(cap, device=cuda)[None, :] < src.sizes[:, None]
    assert bool(((got == exp) | ~inside).all())


def test_block_choice(hc, cuda):
    import torch
    chunks = [random.Random(3).randbytes(65536), bench_text(65536), b"abc", b""]
    streams, sizes = compress_guarded(hc, torch, cuda, chunks)
    check_round_trip(list(zip("random text abc empty".split(), chunks)), streams)
    btype = [(s[0] >> 1) & 3 for s in streams]
    assert btype == [0, 2, 1, 1], btype
    assert sizes[0] == 65546
    assert sizes[2] == 5    # 3 + 3 * 8 + 7 = 34 bits; stored is 8 bytes, a dynamic header alone is longer
    assert sizes[3] == 2    # one fixed block holding only symbol 256: 10 bits
    assert streams[3] == b"\x03\x00"


def test_matches_reach_full_length(hc, cuda):
    """65536 bytes of one value: 255 matches of up to 258 bytes at 13 bits each under fixed codes, about 415 bytes"""
    import torch
    for value in (0, 0xA5):
        (stream,), (size,) = compress_guarded(hc, torch, cuda, [bytes([value]) * 65536])
        assert inflate(stream)[0] == bytes([value]) * 65536
        print("one value: %d bytes" % size)
        assert size <= 512, size


def test_the_parse_contributes(hc, cuda):
    """a floor: smaller than Huffman coding alone (zlib's Z_HUFFMAN_ONLY) and smaller than this library's Snappy"""
    import torch
    text = bench_text(64 * 65536)
    chunks = [text[i * 65536:(i + 1) * 65536] for i in range(64)]
    src = hc.batch.from_host_chunks(chunks, cuda)
    comp = hc.batch.DeflateEncoder().compress(src, 65536)
    snappy = hc.batch.Codec("Snappy").compress(src, 65536)
    torch.cuda.synchronize()
    total = int(comp.sizes.sum().item())
    snappy_total = int(snappy.sizes.sum().item())

    def huffman_only(c):
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        return len(z.compress(c) + z.flush())
    huff_total = sum(huffman_only(c) for c in chunks)
    raw = 64 * 65536
    print("ratio: deflate %.3f, huffman only %.3f, snappy %.3f" % (raw / total, raw / huff_total, raw / snappy_total))
    assert total < huff_total
    assert total < snappy_total
    for c, s in zip(chunks[:4], comp.to_host_chunks()[:4]):
        assert inflate(s)[0] == c


def test_determinism(hc, cuda):
    """the same chunk at batch positions 0, 1 and n - 1, among different neighbours and at different addresses,
    in a batch of another size, and in a second call: identical bytes"""
    import torch
    named = dict(cases())
    x = named["tpch_text_65536"]
    others = [named["random_4095"], named["zeros_65536"], named["text_32769"], named["period_255_65535"], b""]
    a = [x, x] + others + [x]
    b = [others[2], x, others[0]]
    sa, _ = compress_guarded(hc, torch, cuda, a, offsets=(0, 3, 9), turn=0)
    sa2, _ = compress_guarded(hc, torch, cuda, a, offsets=(0, 3, 9), turn=0)
    sb, _ = compress_guarded(hc, torch, cuda, b, offsets=(5, 1), turn=1)
    assert sa == sa2
    assert sa[0] == sa[1] == sa[-1] == sb[1]
    assert sa[4] == sb[0] and sa[2] == sb[2]
    assert inflate(sa[0])[0] == x


def test_graph_capture(hc, cuda):
    """capture once, replay twice onto cleared output: the bytes of the direct call"""
    import torch
    named = cases()[::9]
    chunks = [d for _, d in named]
    n = len(chunks)
    src = hc.batch.from_host_chunks(chunks, cuda)
    enc = hc.batch.DeflateEncoder()
    cap = enc.max_output_chunk_size(MAX_CHUNK)
    direct = enc.compress(src, MAX_CHUNK)
    torch.cuda.synchronize()
    want = direct.to_host_chunks()
    check_round_trip(named, want)
    dst = hc.batch.alloc_batch(n, cap, cuda, fill=0xEE)
    temp = torch.empty(max(enc.compress_temp_size(n, MAX_CHUNK), 8), dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert enc.compress_async(src, MAX_CHUNK, temp, dst) == 0   # warm: the code object is loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert enc.compress_async(src, MAX_CHUNK, temp, dst) == 0
    for _ in range(2):
        dst.data.fill_(0xEE)
        dst.sizes.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert dst.to_host_chunks() == want


def test_a_larger_max_chunk_gives_the_same_bytes(hc, cuda):
    import torch
    named = [(nm, d) for nm, d in cases() if len(d) <= 4095][::3]
    chunks = [d for _, d in named]
    exact, _ = compress_guarded(hc, torch, cuda, chunks, max_chunk=max(len(c) for c in chunks))
    generous, _ = compress_guarded(hc, torch, cuda, chunks, max_chunk=MAX_CHUNK)
    assert exact == generous
    check_round_trip(named, exact)
