"""The batched Zstandard encoder (include/hipcomp/zstd_compress.h, lib/libhipcomp_zstd_compress.so) on the GPU.
The judge of every frame is this library's own decoder on the device (ZstdDecoder: status 0, the exact size, the
bytes), which the committed fixtures hold to libzstd; libzstd itself (G.arbiter) judges too wherever it loads, and
test_libzstd_returns_every_chunk is the one test that is skipped where it does not.  Every buffer of the byte-level
tests lies in decode_guard.GuardedSlots, so a read-modify-write of the input or a byte written at or beyond the
output bound is seen."""
import random
import struct
import zlib

import numpy as np
import pytest

import deflate_streamgen as D
import zstd_framegen as G
import zstd_seqscan as S
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu

MAX_CHUNK = 65536
SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 16383, 16384, 16385, 32768, 65535, 65536)


def bound(n: int) -> int:
    return n + 14


def bench_text(n: int) -> bytes:
    import bench
    return bench.gen_text(n).tobytes()


def inputs(size=65536):
    """the twelve kinds of tests/test_deflate_compress_gpu.py's inputs(), built here, one with a skewed histogram of
    byte values >= 128 (its tree cannot be described directly), one of 256 distinct values and one of four low
    values (a tree that is shortest described directly)"""
    rnd = random.Random(5)
    ints = sorted(rnd.randrange(-2 ** 31, 2 ** 31) for _ in range(size // 4))

    def period(p):
        unit = bytes(rnd.randrange(256) for _ in range(p))
        return (unit * (2 * size // p + 2))[:max(size, 2 * p + 100)]
    rng = np.random.default_rng(8878)
    skewed = (255 - np.minimum(rng.geometric(0.08, size) - 1, 127)).astype(np.uint8).tobytes()
    distinct = bytes(range(256)) + rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), size // 256 - 1)).tobytes()
    return {
        "empty": b"", "one_byte": b"x", "text": D._text(size, 17), "tpch_text": bench_text(size),
        "random": rnd.randbytes(size), "zeros": bytes(size),
        "sorted_int32": struct.pack(f"<{len(ints)}i", *ints),
        "period_1": period(1), "period_2": period(2), "period_3": period(3), "period_255": period(255),
        "period_32768": period(32768),
        "skewed_high_bytes": skewed, "distinct_256": distinct,
        "four_values": rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size, p=[0.6, 0.2, 0.1, 0.1]).tobytes(),
    }


def match_edges():
    """The farthest offsets.  A match of 4 bytes at offset d starts at position d or later and ends inside the chunk,
    so d <= 65532 in a chunk of 65536 bytes: 65534 and 65535 cannot occur in one block of at most 65536 bytes.
    65531 and 65532 are reached, at 65533 only 3 bytes are left and none is found.  (The filler is one long run:
    its matches leave the table slots of the unit's positions alone.)"""
    rnd = random.Random(8878)
    unit = bytes(rnd.randrange(1, 256) for _ in range(300))
    out = {}
    for d in (65531, 65532, 65533):
        out[f"repeat_at_offset_{d}"] = unit[:100] + bytes(d - 100) + unit[:65536 - d]
    out["match_runs_to_the_chunks_end"] = unit + rnd.randbytes(500) + unit[:100]
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


_cases = None


def shared_cases():
    global _cases
    if _cases is None:
        _cases = cases()
    return _cases


def compress_guarded(hc, torch, dev, chunks, max_chunk=MAX_CHUNK, offsets=(0,), turn=0, checksum=False):
    """-> (frames, sizes): every chunk compressed inside guarded slots; containment is asserted here"""
    n = len(chunks)
    cap = bound(max_chunk)
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=offsets, turn=turn, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, [cap] * n, dev, offsets=offsets, turn=turn + 3, seed=22)
    enc = hc.batch.ZstdEncoder(checksum=checksum)
    temp = torch.empty(max(enc.compress_temp_size(n, max_chunk), 8), dtype=torch.uint8, device=dev)
    out_batch = dst.batch(hc)
    out_batch.sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    assert enc.compress_async(src.batch(hc), max_chunk, temp, out_batch) == 0
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()                      # the input is only read
    got = dst.after()
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)   # nothing at or beyond out_i + bound
    sizes = out_batch.sizes.cpu().tolist()
    for c, s in zip(chunks, sizes):
        assert 0 < s <= bound(len(c)), (len(c), s)
    return [dst.slot_bytes(got, i, sizes[i]) for i in range(n)], sizes


def check_round_trip(hc, torch, dev, named, frames, libzstd=None):
    """ZstdDecoder on the device: status 0, the exact size, the bytes; and libzstd where it loads"""
    cap = max([len(d) for _, d in named] + [1])
    comp = hc.batch.from_host_chunks(frames, dev)
    dec, actual, statuses = hc.batch.ZstdDecoder().decompress(comp, cap)
    torch.cuda.synchronize()
    st, sz = statuses.cpu().tolist(), actual.cpu().tolist()
    for (name, data), s, z in zip(named, st, sz):
        assert s == 0 and z == len(data), (name, s, z)
    for (name, data), got in zip(named, dec.to_host_chunks()):
        assert got == data, name
    if libzstd is None:
        libzstd = G.libzstd() is not None
    if libzstd:
        for (name, data), f in zip(named, frames):
            assert G.arbiter(f, len(data)) == data, name


def test_round_trip_at_every_byte_offset(hc, cuda):
    import torch
    named = shared_cases()
    assert len(named) >= 200
    offsets = tuple(range(16))
    for checksum in (False, True):
        for turn in range(4):   # chunk i at input offset (i + 4 * turn) % 16 and output offset (i + 4 * turn + 3) % 16
            frames, _ = compress_guarded(hc, torch, cuda, [d for _, d in named], offsets=offsets, turn=4 * turn, checksum=checksum)
            check_round_trip(hc, torch, cuda, named, frames)
            for (name, data), f in zip(named, frames):
                assert ("checksum" in G.inspect(f)) == checksum, name


def test_far_offsets_are_found(hc, cuda):
    import torch
    e = match_edges()
    names = ["repeat_at_offset_65531", "repeat_at_offset_65532", "repeat_at_offset_65533", "match_runs_to_the_chunks_end"]
    frames, sizes = compress_guarded(hc, torch, cuda, [e[n] for n in names])
    check_round_trip(hc, torch, cuda, [(n, e[n]) for n in names], frames)
    seqs = [S.sequences_of(f) for f in frames]
    assert seqs[0][-1] == (0, 5, 65531 + 3) and seqs[1][-1] == (0, 4, 65532 + 3)
    assert all(ov - 3 < 65000 for _, _, ov in seqs[2])
    assert seqs[3][-1][1:] == (100, 800 + 3)      # the last match ends with the chunk: no literals behind it


def test_libzstd_returns_every_chunk(hc, cuda):
    import torch
    if G.libzstd() is None:
        pytest.skip("libzstd.so.1 does not load here: the frames are judged by this library's decoder alone")
    named = shared_cases()
    for checksum in (False, True):
        frames, _ = compress_guarded(hc, torch, cuda, [d for _, d in named], checksum=checksum)
        for (name, data), f in zip(named, frames):
            assert G.arbiter(f, len(data)) == data, name
            assert G.arbiter(f, len(data) + 100) == data, name


def test_forms(hc, cuda):
    """What the parse reaches.  It does not reach: RLE literals (literals that are all one byte make a chunk that is
    all one byte, which is an RLE_Block), a 4-stream literals section with the 3-byte header (one stream is taken
    wherever both sizes fit 10 bits), the 3-byte sequence count (32512 sequences: a 64 KiB chunk has at most
    16384), Repeat_Mode and treeless literals (one block per frame).  tests/test_zstd_codes_cpu.py covers the forms
    that a planned token list can reach."""
    import torch
    named = shared_cases()
    forms = set()
    for checksum in (False, True):
        frames, _ = compress_guarded(hc, torch, cuda, [d for _, d in named], checksum=checksum)
        for f in frames:
            forms |= G.inspect(f)
    print(sorted(forms))
    assert {"raw_block", "rle_block", "compressed_block", "fcs_1", "fcs_2", "checksum", "weights_direct", "weights_fse",
            "huffman_literals_1_stream_3"} <= forms
    assert forms & {"huffman_literals_4_stream_4", "huffman_literals_4_stream_5"}
    assert any(f.startswith("raw_literals_") for f in forms)
    full = [t for t in ("ll", "of", "ml") if {f"{t}_predefined", f"{t}_rle", f"{t}_fse"} <= forms]
    assert len(full) >= 2, forms
    assert not forms & {"ll_repeat", "of_repeat", "ml_repeat", "seq_count_3", "treeless_literals_1_stream_3",
                        "treeless_literals_4_stream_3", "window_descriptor", "fcs_4", "fcs_8", "fcs_0"}


def test_exact_small_frames(hc, cuda):
    import torch
    rnd = random.Random(3)
    chunks = [b"", b"x", bytes(65536), rnd.randbytes(65536)]
    named = list(zip("empty x zeros random".split(), chunks))
    frames, sizes = compress_guarded(hc, torch, cuda, chunks)
    check_round_trip(hc, torch, cuda, named, frames)
    assert frames[0] == bytes.fromhex("28b52ffd2000010000")
    if G.libzstd() is not None:
        assert frames[0] == G.compress(b"", 3)
    assert sizes[1] == 10 and "raw_block" in G.inspect(frames[1])
    assert sizes[2] == 11 and "rle_block" in G.inspect(frames[2])
    assert sizes[3] == 65546 and "raw_block" in G.inspect(frames[3])
    with_sum, sizes = compress_guarded(hc, torch, cuda, chunks, checksum=True)
    check_round_trip(hc, torch, cuda, named, with_sum)
    assert sizes == [13, 14, 15, 65550]
    assert with_sum[0] == bytes.fromhex("28b52ffd2400010000") + struct.pack("<I", G.xxh64(b"") & 0xFFFFFFFF)
    for f, c in zip(with_sum, chunks):
        assert f[-4:] == struct.pack("<I", G.xxh64(c) & 0xFFFFFFFF)


def repeat_inputs():
    """A strictly rising int32 column with a constant stride has no 4-byte repeat at all -- every window of 4 bytes
    holds both low bytes of a value, which name it among 65536 -- and a period of 255 bytes is one match to the
    chunk's end.  Both are here and their counts are printed; the column that can use a repeat code is the sorted one
    with the same constant stride in which every value stands three times (a sorted key column with duplicates):
    behind the two bytes that change, the match at offset 4 goes on."""
    rnd = random.Random(5)
    unit = bytes(rnd.randrange(256) for _ in range(255))
    return [("sorted_int32_stride_1000", np.arange(0, 16384 * 1000, 1000, dtype=np.int32).tobytes()),
            ("sorted_int32_stride_1000_each_thrice", (np.arange(16384, dtype=np.int32) // 3 * 1000).astype(np.int32).tobytes()),
            ("period_255", (unit * 258)[:65536])]


def test_repeat_offsets_pay(hc, cuda):
    """sequences whose offset code is 0 (Offset_Value 1), counted by decoding the sequences sections"""
    import torch
    named = repeat_inputs()
    frames, sizes = compress_guarded(hc, torch, cuda, [d for _, d in named])
    check_round_trip(hc, torch, cuda, named, frames)
    total = 0
    for (name, data), f, size in zip(named, frames, sizes):
        seqs = S.sequences_of(f)
        count = 0 if seqs is None else sum(1 for ll, ml, ov in seqs if ov == 1)
        print("%s: %d bytes, %s sequences, %d with Offset_Value 1" % (name, size, "no" if seqs is None else len(seqs), count))
        for ll, ml, ov in seqs or ():
            assert ov == 1 or ov > 3          # repeat offsets 2 and 3 are not used
            assert not (ov == 1 and ll == 0)  # and the first one only behind literals
        total += count
    assert total > 0


def test_the_parse_contributes(hc, cuda):
    """a floor: smaller than Huffman coding alone (zlib's Z_HUFFMAN_ONLY) and smaller than this library's Snappy.  The
    ratios of the Deflate encoder and of libzstd level 1 are printed, not compared: the section overheads at 64 KiB may
    go either way."""
    import torch
    text = bench_text(64 * 65536)
    chunks = [text[i * 65536:(i + 1) * 65536] for i in range(64)]
    src = hc.batch.from_host_chunks(chunks, cuda)
    comp = hc.batch.ZstdEncoder().compress(src, 65536)
    deflate = hc.batch.DeflateEncoder().compress(src, 65536)
    snappy = hc.batch.Codec("Snappy").compress(src, 65536)
    torch.cuda.synchronize()
    total = int(comp.sizes.sum().item())
    deflate_total = int(deflate.sizes.sum().item())
    snappy_total = int(snappy.sizes.sum().item())

    def huffman_only(c):
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        return len(z.compress(c) + z.flush())
    huff_total = sum(huffman_only(c) for c in chunks)
    raw = 64 * 65536
    line = "ratio: zstd %.3f, deflate %.3f, huffman only %.3f, snappy %.3f" % (raw / total, raw / deflate_total, raw / huff_total, raw / snappy_total)
    if G.libzstd() is not None:
        line += ", libzstd level 1 %.3f" % (raw / sum(len(G.compress(c, 1)) for c in chunks))
    print(line)
    assert total < huff_total
    assert total < snappy_total
    named = [("text_%d" % i, c) for i, c in enumerate(chunks)]
    check_round_trip(hc, torch, cuda, named, comp.to_host_chunks())


@pytest.mark.parametrize("n", [1, 7, 3073])
def test_round_trip_on_the_device(hc, cuda, n):
    """n chunks drawn from about 60 distinct inputs, laid out on the device by a gather, compressed, decoded by
    ZstdDecoder and compared on the device.  3073 is one more than the grid's waves: the grid-stride loop takes a
    second trip."""
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
    comp = hc.batch.ZstdEncoder(checksum=True).compress(src, cap)
    dec, actual, statuses = hc.batch.ZstdDecoder().decompress(comp, cap)
    torch.cuda.synchronize()
    assert torch.equal(data, before)
    assert bool((statuses == 0).all())
    assert torch.equal(actual, src.sizes)
    assert bool((comp.sizes > 0).all()) and bool((comp.sizes <= src.sizes + 14).all())
    got = dec.data[: n * dec.stride].view(n, dec.stride)[:, :cap]
    exp = data.view(n, table.stride)[:, :cap]
    inside = torch.arange(cap, device=cuda)[None, :] < src.sizes[:, None]
    assert bool(((got == exp) | ~inside).all())


def test_determinism(hc, cuda):
    """the same chunk at batch positions 0, 1 and n - 1, among different neighbours and at different addresses,
    in a batch of another size, and in a second call: identical bytes"""
    import torch
    named = dict(shared_cases())
    x = named["tpch_text_65536"]
    others = [named["random_4095"], named["zeros_65536"], named["text_32768"], named["period_255_65535"], b""]
    a = [x, x] + others + [x]
    b = [others[2], x, others[0]]
    sa, _ = compress_guarded(hc, torch, cuda, a, offsets=(0, 3, 9), turn=0)
    sa2, _ = compress_guarded(hc, torch, cuda, a, offsets=(0, 3, 9), turn=0)
    sb, _ = compress_guarded(hc, torch, cuda, b, offsets=(5, 1), turn=1)
    assert sa == sa2
    assert sa[0] == sa[1] == sa[-1] == sb[1]
    assert sa[4] == sb[0] and sa[2] == sb[2]
    check_round_trip(hc, torch, cuda, [("x", x)], sa[:1])


def test_graph_capture(hc, cuda):
    """warm, capture on a side stream, replay twice onto cleared output: the bytes of the direct call"""
    import torch
    named = shared_cases()[::9]
    chunks = [d for _, d in named]
    n = len(chunks)
    src = hc.batch.from_host_chunks(chunks, cuda)
    enc = hc.batch.ZstdEncoder(checksum=True)
    cap = enc.max_output_chunk_size(MAX_CHUNK)
    direct = enc.compress(src, MAX_CHUNK)
    torch.cuda.synchronize()
    want = direct.to_host_chunks()
    check_round_trip(hc, torch, cuda, named, want)
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
    named = [(nm, d) for nm, d in shared_cases() if len(d) <= 4095][::3]
    chunks = [d for _, d in named]
    exact, _ = compress_guarded(hc, torch, cuda, chunks, max_chunk=max(len(c) for c in chunks))
    generous, _ = compress_guarded(hc, torch, cuda, chunks, max_chunk=MAX_CHUNK)
    assert exact == generous
    check_round_trip(hc, torch, cuda, named, exact)


def test_an_oversized_chunk_is_left_alone(hc, cuda):
    """a chunk above the call's max_uncompressed_chunk_bytes: size 0, not a byte of its slot written, its neighbours
    compressed as ever"""
    import torch
    text = bench_text(8000)
    chunks = [text[:1000], text[:5000], text[1000:1900], text[:1001], b""]
    cap = bound(1000)
    over = [len(c) > 1000 for c in chunks]
    src = GuardedSlots(torch, [len(c) for c in chunks], cuda, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, [cap] * len(chunks), cuda, seed=22, region=[0 if o else cap for o in over])
    enc = hc.batch.ZstdEncoder()
    temp = torch.empty(max(enc.compress_temp_size(len(chunks), 1000), 8), dtype=torch.uint8, device=cuda)
    out_batch = dst.batch(hc)
    out_batch.sizes = torch.full((len(chunks),), -1, dtype=torch.int64, device=cuda)
    assert enc.compress_async(src.batch(hc), 1000, temp, out_batch) == 0
    torch.cuda.synchronize()
    assert src.unchanged() is None
    got = dst.after()
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    sizes = out_batch.sizes.cpu().tolist()
    assert [s == 0 for s in sizes] == over
    kept = [i for i, o in enumerate(over) if not o]
    frames = [dst.slot_bytes(got, i, sizes[i]) for i in kept]
    check_round_trip(hc, torch, cuda, [(str(i), chunks[i]) for i in kept], frames)
    alone, _ = compress_guarded(hc, torch, cuda, [chunks[i] for i in kept], max_chunk=1000)
    assert frames == alone
