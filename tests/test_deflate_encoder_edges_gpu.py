"""The Deflate encoder's kernel held to its scalar writer, bit for bit, on the planned inputs of
tests/deflate_inputgen.py (tests/test_deflate_inputgen_cpu.py says what they reach) and on generic ones.

A round trip proves that a stream is legal, not that it is the stream this encoder is specified to write.  Here
every kernel stream is read back into its tokens (tests/deflate_tokenscan.py), the tokens are held to the plan of the
case, and tests/deflate_codes_driver.cpp's `encode` -- deflate_codes.hpp and nothing else: histograms, sort, code
lengths, codes, header, the three costs, the choice with its ties, and a bit writer of four lines -- writes the
stream again from them: the two are identical, whatever the parse chose.  That holds the ds_add histograms, the
sort over the lanes, the ds_or stage with its flushes and the stored writer to the header at once.  The wave's
record buffer in temp space is read as well: it holds the records of the stream's tokens and nothing more.

All cases go through one launch; input, output and temp space -- exactly the size the library asks for -- lie in
decode_guard.GuardedSlots.  A stream of stored blocks holds no tokens: its tokens are the record buffer's."""
import time
import zlib

import numpy as np
import pytest

import deflate_inputgen as D
import deflate_tokenscan as S
import test_deflate_compress_gpu as T
from decode_guard import GuardedSlots
from test_deflate_inputgen_cpu import build_driver, encode_all

pytestmark = pytest.mark.gpu

MAX_WAVES = 3072


def records_per_wave(max_chunk):
    return (max_chunk // 4 + 2 + 63) // 64 * 64


def launch(hc, torch, dev, chunks, max_chunk):
    """one launch with everything guarded, n <= 3072 so that wave i takes chunk i
    -> (streams, per chunk the wave's buffer as dwords, per chunk which of its dwords changed)"""
    n = len(chunks)
    assert n <= MAX_WAVES
    enc = hc.batch.DeflateEncoder()
    per_wave = records_per_wave(max_chunk)
    size = enc.compress_temp_size(n, max_chunk)
    assert size == 4 * n * per_wave
    temp = GuardedSlots(torch, [size], dev, seed=23)
    at = int(temp.at[0])
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=(0, 1, 2, 3), seed=21, chunks=chunks)
    dst = GuardedSlots(torch, [T.bound(max_chunk)] * n, dev, offsets=(0, 3, 1, 2), seed=22)
    out_batch = dst.batch(hc)
    out_batch.sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
    assert enc.compress_async(src.batch(hc), max_chunk, temp.data[at:at + size], out_batch) == 0
    torch.cuda.synchronize()
    got_temp = temp.after()
    assert temp.first_guard_change(got_temp) is None, temp.first_guard_change(got_temp)
    assert src.unchanged() is None, src.unchanged()
    got = dst.after()
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    sizes = out_batch.sizes.cpu().tolist()
    for c, s in zip(chunks, sizes):
        assert 0 < s <= T.bound(len(c)), (len(c), s)
    streams = [dst.slot_bytes(got, i, sizes[i]) for i in range(n)]
    words = got_temp[at:at + size].view("<u4").reshape(n, per_wave)
    changed = words != temp.host[at:at + size].view("<u4").reshape(n, per_wave)
    return streams, words, changed


def records_in(words, n):
    """the records of a wave's buffer up to the final one of a chunk of n bytes, as (literal run, match length, distance - 1)"""
    out, pos = [], 0
    for w in words.tolist():
        ll, ml, d = w >> 24, (w >> 15) & 511, w & 32767
        out.append((ll, ml, d))
        pos += ll + ml
        if ml == 0 and ll < D.RUN_SENT:          # (a run of 192 left on its own: the final record still follows)
            break
    assert pos == n and out[-1][1] == 0, (pos, n)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("deflate_edges"))


@pytest.fixture(scope="module")
def run(hc, cuda, driver, tmp_path_factory):
    """-> (cases, kernel streams, their scans, the tokens of every stream, the buffers, what changed in them,
    the driver's output for (chunk, those tokens))"""
    import torch
    t0 = time.perf_counter()
    cases = D.all_cases()
    t1 = time.perf_counter()
    streams, words, changed = launch(hc, torch, cuda, [c.content for c in cases], D.MAX_CHUNK)
    t2 = time.perf_counter()
    scans = [S.scan(s) for s in streams]
    tokens = []
    for c, s, w in zip(cases, scans, words):
        if all(b.kind == S.STORED for b in s.blocks):
            tokens.append(D.tokens_of(records_in(w, len(c.content)))[0])
        else:
            tokens.append(s.tokens)
    t3 = time.perf_counter()
    scalar = encode_all(driver, tmp_path_factory.mktemp("edges"), [(c.content, t) for c, t in zip(cases, tokens)])
    t4 = time.perf_counter()
    print("fixture: %d cases built in %.1f s, launch and copies %.1f s, %d stream bytes scanned in %.1f s, driver %.1f s" % (
        len(cases), t1 - t0, t2 - t1, sum(len(s) for s in streams), t3 - t2, t4 - t3))
    return cases, streams, scans, tokens, words, changed, scalar


def test_tokens(run):
    cases, streams, scans, tokens, _, _, _ = run
    planned = 0
    for c, stream, s, toks in zip(cases, streams, scans, tokens):
        got, eof, unused = T.inflate(stream)
        assert eof and unused == b"" and got == c.content and s.output == c.content, c.name
        if c.family != "generic":
            assert c.tokens is not None, c.name
        if c.tokens is not None:                 # every planned case, and the generic ones the mirror can predict
            planned += 1
            assert toks == c.tokens, c.name
        assert D.rebuilds(c.content, toks), c.name
        assert D.maximal(c.content, toks), c.name
        assert all(D.MIN_MATCH <= ml <= D.MAX_MATCH and 1 <= d <= D.MAX_DISTANCE for _, ml, d in toks), c.name
    print("%d cases, the tokens of %d equal the mirror's" % (len(cases), planned))
    assert planned >= 180


def test_bytes_equal_the_scalar_writer(run):
    cases, streams, scans, _, _, _, scalar = run
    kinds = {0: 0, 1: 0, 2: 0}
    for c, stream, s, (want, kind, bits, dyn, fixed, stored) in zip(cases, streams, scans, scalar):
        assert stream == want, (c.name, kind, [b.kind for b in s.blocks], len(stream), len(want))
        assert len(stream) == (bits + 7) // 8 and s.total_bits == bits, c.name
        kinds[kind] += 1
    print("kinds (stored, fixed, dynamic):", kinds)
    assert all(kinds.values())


def test_temp_space_holds_the_records_and_nothing_more(run):
    cases, _, _, tokens, words, changed, _ = run
    for c, toks, w, ch in zip(cases, tokens, words, changed):
        recs = D.records(toks, len(c.content))
        assert records_in(w, len(c.content)) == recs, c.name               # field for field, the final record too
        assert w[:len(recs)].tolist() == D.record_words(recs), c.name
        stored = (len(recs) + 63) // 64 * 64
        assert not ch[stored:].any(), (c.name, len(recs), int(np.flatnonzero(ch)[-1]))


def test_batch_position_and_max_chunk(hc, cuda, run):
    """the chunk with the most records alone, its buffer sized for exactly its length: the bytes of the large batch"""
    import torch
    cases, streams = run[0], run[1]
    k = [c.name for c in cases].index("counts/max_records")
    c = cases[k]
    recs = D.records(c.tokens, len(c.content))
    assert len(recs) > records_per_wave(len(c.content)) - 128
    (exact,), words, changed = launch(hc, torch, cuda, [c.content], len(c.content))
    assert exact == streams[k]
    assert words[0][:len(recs)].tolist() == D.record_words(recs)
    assert not changed[0][(len(recs) + 63) // 64 * 64:].any()
    (generous,), _, _ = launch(hc, torch, cuda, [c.content], D.MAX_CHUNK)
    assert generous == exact


def test_second_grid_stride_trip(hc, cuda, run):
    """3073 tiny chunks: wave 0 takes chunk 0 and, with what its LDS and its buffer hold from it, chunk 3072"""
    import torch
    cases, streams = run[0], run[1]
    small = [(c, s) for c, s in zip(cases, streams) if len(c.content) <= 64]
    first = [c.name for c, _ in small].index("trip/position0_of_an_empty_slot")
    n = MAX_WAVES + 1
    pick = [(first + i) % len(small) for i in range(n)]
    pick[n - 1] = first
    src = hc.batch.from_host_chunks([small[p][0].content for p in pick], cuda)
    comp = hc.batch.DeflateEncoder().compress(src, 64)
    torch.cuda.synchronize()
    got = comp.to_host_chunks()
    assert got[n - 1] == got[0] == small[first][1]
    for i in (0, n - 1):
        assert T.inflate(got[i]) == (small[first][0].content, True, b"")
    assert got == [small[p][1] for p in pick]
