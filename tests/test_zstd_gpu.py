"""The batched Zstandard decoder on the GPU (include/hipcomp/zstd.h) through api.py and batch.py: every legal
planned frame (tests/zstd_framegen.py) and every libzstd-made fixture frame (tests/zstd_fixtures.py) decodes to its
bytes, in batches that mix forms and sizes from 0 bytes to 300 KiB, with inputs and outputs at odd addresses and
guard bytes around the inputs, the outputs and the temp space (tests/decode_guard.py)."""
import pytest

import zstd_fixtures as F
import zstd_framegen as G
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu
OK, CANNOT, INVALID = 0, 12, 10
ODD = (1, 3, 5, 7, 9, 11, 13, 15)


def run(hc, torch, dev, chunks, caps, offsets=ODD, max_chunk=None, stream=None):
    """-> (output slots, arena after, actual, statuses, sizes); the temp space is a guarded slot of its own"""
    n = len(chunks)
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=offsets, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, caps, dev, offsets=offsets, turn=3, seed=22)
    dec = hc.batch.ZstdDecoder()
    tbytes = dec.decompress_temp_size(n, max(caps) if max_chunk is None else max_chunk)
    temp = GuardedSlots(torch, [tbytes], dev, seed=23)
    actual = torch.full((n,), -1, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st = dec.lib.hipcompBatchedZstdDecompressAsync(
        src.ptrs.data_ptr(), src.sizes.data_ptr(), dst.caps_t.data_ptr(), actual.data_ptr(), n, int(temp.ptrs[0].item()), tbytes,
        dst.ptrs.data_ptr(), statuses.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
    assert st == OK
    sizes = dec.get_decompress_size(src.batch(hc))
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()
    assert temp.first_guard_change() is None, "temp space: " + str(temp.first_guard_change())
    return dst, dst.after(), actual.cpu().tolist(), statuses.cpu().tolist(), sizes.cpu().tolist()


def legal_cases():
    """[(name, chunk, content)]: the planned frames, then libzstd's own"""
    return [(n, c, d) for n, c, d, _ in G.legal_plans()] + F.load()[0]


def check_parity(hc, torch, dev, cases, caps):
    dst, got, actual, statuses, sizes = run(hc, torch, dev, [c for _, c, _ in cases], caps)
    for i, (name, _, want) in enumerate(cases):
        assert statuses[i] == OK, (name, statuses[i])
        assert actual[i] == len(want), (name, actual[i], len(want))
        assert dst.slot_bytes(got, i, len(want)) == want, name
        dst.region[i] = len(want)
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    return sizes


def test_every_legal_frame_exact_capacity(hc, cuda):
    import torch
    cases = legal_cases()
    assert 60 <= len(cases) <= 512 and {len(d) for _, _, d in cases} >= {0, 300 * 1024}
    sizes = check_parity(hc, torch, cuda, cases, [len(d) for _, _, d in cases])
    # the size query: declared sizes and, for the frames without one, the decode without an output
    declared = 0
    for (name, chunk, want), size in zip(cases, sizes):
        assert size == len(want), name
        declared += "fcs_0" not in G.inspect(chunk)
    assert 0 < declared < len(cases)


def test_generous_capacity_leaves_the_tail_alone(hc, cuda):
    import torch
    cases = legal_cases()
    check_parity(hc, torch, cuda, cases, [len(d) + 1 + 37 * (i % 5) for i, (_, _, d) in enumerate(cases)])


def test_capacity_one_short_is_refused(hc, cuda):
    import torch
    cases = [c for c in legal_cases() if len(c[2]) > 0]
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [c for _, c, _ in cases], [len(d) - 1 for _, _, d in cases])
    assert statuses == [CANNOT] * len(cases) and actual == [0] * len(cases)
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    assert sizes == [len(d) for _, _, d in cases]     # (the query knows no capacity)


def test_size_query_returns_a_false_declared_size(hc, cuda):
    import torch
    lie = G.frame_header(11, single_segment=True, fcs_bytes=1) + G.block(0, b"0123456789", True)
    honest = G.frame([("raw", b"0123456789")])[0]
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [lie, honest], [64, 64])
    assert sizes == [11, 10] and statuses == [CANNOT, OK] and actual == [0, 10]


def test_temp_space_too_small_is_refused_by_the_host(hc, cuda):
    import torch
    dec = hc.batch.ZstdDecoder()
    src = hc.batch.from_host_chunks([G.frame([("raw", b"abc")])[0]] * 3, cuda)
    dst = hc.batch.alloc_batch(3, 16, cuda)
    caps = torch.full((3,), 16, dtype=torch.int64, device=cuda)
    need = dec.decompress_temp_size(3, 1)
    temp = torch.empty(need, dtype=torch.uint8, device=cuda)
    assert need == 3 * 256
    assert dec.decompress_async(src, caps, None, temp[:need - 1], dst, None) == INVALID
    assert dec.decompress_async(src, caps, None, None, dst, None) == INVALID
    assert dec.decompress_async(src, caps, None, temp, dst, None) == OK
    torch.cuda.synchronize()
    assert dst.chunk_bytes(1, 3) == b"abc"


def test_two_calls_on_one_stream_and_the_batch_helper(hc, cuda):
    import torch
    cases = legal_cases()[::3]
    dec = hc.batch.ZstdDecoder()
    cap = max(len(d) for _, _, d in cases)
    comp = hc.batch.from_host_chunks([c for _, c, _ in cases], cuda)
    a, a_actual, a_status = dec.decompress(comp, cap)
    b, b_actual, b_status = dec.decompress(comp, cap)     # (a temp buffer of its own)
    torch.cuda.synchronize()
    for out, actual, status in ((a, a_actual, a_status), (b, b_actual, b_status)):
        assert status.cpu().tolist() == [OK] * len(cases)
        assert out.to_host_chunks() == [d for _, _, d in cases]


def test_one_call_captured_into_a_graph(hc, cuda):
    import torch
    cases = legal_cases()[1::4]
    dec = hc.batch.ZstdDecoder()
    cap = max(len(d) for _, _, d in cases)
    comp = hc.batch.from_host_chunks([c for _, c, _ in cases], cuda)
    dst = hc.batch.alloc_batch(comp.n, cap, cuda, fill=0xEE)
    caps = torch.full((comp.n,), cap, dtype=torch.int64, device=cuda)
    actual = torch.full((comp.n,), -1, dtype=torch.int64, device=cuda)
    statuses = torch.full((comp.n,), -1, dtype=torch.int32, device=cuda)
    temp = torch.empty(dec.decompress_temp_size(comp.n, cap), dtype=torch.uint8, device=cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        assert dec.decompress_async(comp, caps, actual, temp, dst, statuses, stream=side) == OK
    graph.replay()
    torch.cuda.synchronize()
    assert statuses.cpu().tolist() == [OK] * comp.n
    dst.sizes = actual
    assert dst.to_host_chunks() == [d for _, _, d in cases]


def test_every_wave_stays_inside_its_temp_slice(hc, cuda):
    """Wave w of the launch owns temp[w * share, (w + 1) * share), the share being temp_bytes / min(chunks, 3072) rounded
    down to 256 bytes; chunk i is decoded by wave i of the first min(chunks, 3072).  With a share larger than any
    chunk's content (no block has more literals than content) the tail of every slice keeps its pattern."""
    import numpy as np
    import torch
    cases = [c for c in legal_cases() if len(c[2]) <= 3000]
    assert len(cases) >= 40 and any("huffman" in n for n, _, _ in cases)
    share, n = 4096, len(cases)
    dec = hc.batch.ZstdDecoder()
    assert dec.decompress_temp_size(n, share) == n * share
    comp = hc.batch.from_host_chunks([c for _, c, _ in cases], cuda)
    dst = hc.batch.alloc_batch(n, share, cuda)
    caps = torch.full((n,), share, dtype=torch.int64, device=cuda)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    before = np.random.default_rng(24).integers(0, 256, n * share, dtype=np.uint8)
    temp = torch.from_numpy(before.copy()).to(cuda)
    assert dec.decompress_async(comp, caps, None, temp, dst, statuses) == OK
    torch.cuda.synchronize()
    assert statuses.cpu().tolist() == [OK] * n
    after = temp.cpu().numpy()
    used = 0
    for w, (name, _, content) in enumerate(cases):
        lo, hi = w * share, (w + 1) * share
        assert (after[lo + len(content):hi] == before[lo + len(content):hi]).all(), (name, w)
        used += int((after[lo:hi] != before[lo:hi]).any())
    assert used >= 5      # (Huffman and RLE literals do go through the temp space)
