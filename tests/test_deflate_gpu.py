"""The batched Deflate decoder (include/hipcomp/deflate.h, lib/libhipcomp_deflate.so) against zlib on the GPU:
byte-exact parity on a corpus of zlib's own streams (every level, strategy and flush mode that changes the block
structure), on every legal planned stream of tests/deflate_streamgen.py at every input / output byte offset, the
capacity rules, large batches and graph capture.  The oracle is zlib.decompress(stream, -15) throughout."""
import random
import struct
import zlib

import pytest

import deflate_streamgen as G
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu

OK, CANNOT = 0, 12
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush is None or len(data) < 2:
        return c.compress(data) + c.flush()
    third = len(data) // 3
    return (c.compress(data[:third]) + c.flush(flush) + c.compress(data[third:2 * third]) + c.flush(flush)
            + c.compress(data[2 * third:]) + c.flush())


def bench_text(n: int) -> bytes:
    import bench
    return bench.gen_text(n).tobytes()


def inputs(size=65536):
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


def corpus(size=65536):
    """[(name, stream, source)]"""
    out = []
    for name, data in inputs(size).items():
        for level in (0, 1, 6, 9):
            for strategy in STRATEGIES:
                for fname, flush in (("", None), ("_sync", zlib.Z_SYNC_FLUSH), ("_full", zlib.Z_FULL_FLUSH)):
                    out.append((f"{name}_l{level}_s{strategy}{fname}", deflate(data, level, strategy, flush), data))
    return out


def run(hc, torch, dev, streams, caps, in_offsets=(0,), out_offsets=(0,), turn=0):
    n = len(streams)
    src = GuardedSlots(torch, [len(s) for s in streams], dev, offsets=in_offsets, turn=turn, seed=11, chunks=streams)
    dst = GuardedSlots(torch, caps, dev, offsets=out_offsets, turn=turn + 3, seed=12)
    actual = torch.full((n,), -1, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    dec = hc.batch.DeflateDecoder()
    assert dec.decompress_async(src.batch(hc), dst.caps_t, actual, None, dst.batch(hc), statuses) == 0
    sizes = dec.get_decompress_size(src.batch(hc))
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()
    return dst, dst.after(), actual.cpu().tolist(), statuses.cpu().tolist(), sizes.cpu().tolist()


def check_parity(hc, torch, dev, cases, caps=None, **kw):
    """cases: [(name, stream, expected)]: all succeed with the expected bytes, nothing else is touched."""
    caps = [len(e) for _, _, e in cases] if caps is None else caps
    dst, got, actual, statuses, sizes = run(hc, torch, dev, [s for _, s, _ in cases], caps, **kw)
    for i, (name, _, want) in enumerate(cases):
        assert statuses[i] == OK, (name, statuses[i])
        assert actual[i] == len(want) and sizes[i] == len(want), (name, actual[i], sizes[i], len(want))
        assert dst.slot_bytes(got, i, len(want)) == want, name
    # the tails of generous capacities and every guard byte: untouched
    for i, (_, _, want) in enumerate(cases):
        dst.region[i] = len(want)
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)


def test_zlib_agrees_with_itself():
    """the corpus holds what its names say: stored, fixed and dynamic blocks, several blocks with flushes"""
    kinds = set()
    for name, s, data in corpus(4096):
        assert zlib.decompress(s, -15) == data
        kinds.add((s[0] >> 1) & 3)
    assert kinds == {0, 1, 2}


def test_parity_on_the_corpus(hc, cuda):
    import torch
    cases = corpus()
    assert len(cases) == 12 * 4 * 4 * 3
    check_parity(hc, torch, cuda, cases)


@pytest.mark.parametrize("kind", ["text", "random"])
def test_parity_on_16_mib_chunks(hc, cuda, kind):
    import torch
    n = 16 << 20
    data = bench_text(n) if kind == "text" else random.Random(9).randbytes(n)
    s = deflate(data, 6)
    comp = hc.batch.from_host_chunks([s], cuda)
    dec = hc.batch.DeflateDecoder()
    dst, actual, statuses = dec.decompress(comp, n)
    sizes = dec.get_decompress_size(comp)
    torch.cuda.synchronize()
    assert statuses.cpu().tolist() == [OK] and actual.cpu().tolist() == [n] and sizes.cpu().tolist() == [n]
    assert bytes(dst.data[:n].cpu().numpy().tobytes()) == data


@pytest.mark.parametrize("n", [1, 7, 1000, 100000])
def test_batches_of_mixed_kinds(hc, cuda, n):
    """n chunks drawn from 61 distinct streams of every kind (equal streams repeat on purpose); the batch and its
    expectation are laid out on the device by a gather, and compared there."""
    import torch
    kinds = [(nm, s, d) for nm, s, d in corpus(3000) if len(d) > 1][::9][:58]
    kinds += [("empty", deflate(b""), b""), ("one", deflate(b"q"), b"q"), ("fixed_empty", G.legal_plans()[24][1], b"")]
    assert G.legal_plans()[24][0] == "empty_fixed"
    k = len(kinds)
    cap = max(len(d) for _, _, d in kinds)
    table = hc.batch.from_host_chunks([s for _, s, _ in kinds], cuda)
    want = hc.batch.from_host_chunks([d for _, _, d in kinds], cuda, stride=cap)
    pick = (torch.arange(n, device=cuda) * 7 + torch.arange(n, device=cuda) // k) % k
    comp_data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    comp = hc.batch.ChunkBatch(comp_data, hc.batch.make_ptrs(comp_data, n, table.stride), table.sizes[pick], table.stride)
    dec = hc.batch.DeflateDecoder()
    dst, actual, statuses = dec.decompress(comp, cap)
    sizes = dec.get_decompress_size(comp)
    torch.cuda.synchronize()
    assert bool((statuses == OK).all())
    true = want.sizes[pick]
    assert torch.equal(actual, true) and torch.equal(sizes, true)
    got = dst.data[: n * dst.stride].view(n, dst.stride)[:, :cap]
    exp = want.data[: k * want.stride].view(k, want.stride)[pick][:, :cap]
    inside = torch.arange(cap, device=cuda)[None, :] < true[:, None]
    assert bool(((got == exp) | ~inside).all())


def test_every_legal_planned_stream_at_every_byte_offset(hc, cuda):
    import torch
    plans = G.legal_plans()
    offsets = tuple(range(16))
    for turn in range(16):   # plan i sits at input offset (i + turn) % 16 and output offset (i + turn + 3) % 16
        check_parity(hc, torch, cuda, plans, in_offsets=offsets, out_offsets=offsets, turn=turn)


def test_capacities(hc, cuda):
    """one byte short: CannotDecompress, actual 0, guards intact; exact: success; generous: the tail untouched"""
    import torch
    base = [(n, s, e) for n, s, e in G.legal_plans() if len(e) > 0 and not n.startswith("stored65535_at_bit")]
    base += [(n, s, d) for n, s, d in corpus(5000) if len(d) > 1][::11]
    streams = [s for _, s, _ in base]
    short = [len(e) - 1 for _, _, e in base]
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, streams, short)
    assert statuses == [CANNOT] * len(base) and actual == [0] * len(base)
    assert sizes == [len(e) for _, _, e in base]   # the size query knows no capacity
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    check_parity(hc, torch, cuda, base)
    check_parity(hc, torch, cuda, base, caps=[len(e) + 1 + 37 * (i % 5) for i, (_, _, e) in enumerate(base)])
    # capacity 0: only the empty streams decode
    empties = [(n, s, e) for n, s, e in G.legal_plans() if len(e) == 0]
    assert len(empties) >= 4
    check_parity(hc, torch, cuda, empties)


def test_null_statuses_and_actual_sizes(hc, cuda):
    import torch
    data = G._text(5000, 2)
    comp = hc.batch.from_host_chunks([deflate(data)] * 3, cuda)
    dst = hc.batch.alloc_batch(3, len(data), cuda)
    caps = torch.full((3,), len(data), dtype=torch.int64, device=cuda)
    assert hc.batch.DeflateDecoder().decompress_async(comp, caps, None, None, dst, None) == 0
    torch.cuda.synchronize()
    assert [dst.chunk_bytes(i, len(data)) for i in range(3)] == [data] * 3


def test_graph_capture(hc, cuda):
    """capture once, replay twice on cleared output: the same bytes (nothing synchronises or allocates)"""
    import torch
    cases = [(n, s, d) for n, s, d in corpus(4000)][::13]
    comp = hc.batch.from_host_chunks([s for _, s, _ in cases], cuda)
    cap = max(len(d) for _, _, d in cases)
    n = len(cases)
    dst = hc.batch.alloc_batch(n, cap, cuda, fill=0xEE)
    caps = torch.full((n,), cap, dtype=torch.int64, device=cuda)
    actual = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    dec = hc.batch.DeflateDecoder()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert dec.decompress_async(comp, caps, actual, None, dst, statuses) == 0   # warm: the code object is loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert dec.decompress_async(comp, caps, actual, None, dst, statuses) == 0
    for _ in range(2):
        dst.data.fill_(0xEE)
        actual.fill_(-1)
        statuses.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert statuses.cpu().tolist() == [OK] * n
        assert actual.cpu().tolist() == [len(d) for _, _, d in cases]
        for i, (name, _, d) in enumerate(cases):
            assert dst.chunk_bytes(i, len(d)) == d, name
