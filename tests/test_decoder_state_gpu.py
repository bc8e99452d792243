"""No decoder state outlives its chunk, frame or block (tests/decoder_state_plans.py, held to libzstd and zlib by
tests/test_decoder_state_cpu.py).

The four companion decoders walk a batch grid-stride with their tables in a wave's slice of LDS.  Each of the large tests
here is one launch of three chunks for every wave of the decoder's grid: a primer that leaves as much behind as the
format allows, then a victim -- every planned stream of 4 KiB or less, the illegal ones included, which are illegal only
for a table that the primer has just left in LDS -- then a legal stream right behind the victim.  The distinct streams
are uploaded once and the batch is pointers into that table; every chunk has its exact capacity and the outputs lie
back to back, so that a byte too many lands in a neighbour that is compared.  Statuses, sizes and bytes are compared on
the device.  The small tests ask the same inside one chunk: a primer frame and a victim frame, a primer block and a
victim block, in guarded slots at odd offsets (tests/decode_guard.py)."""
import numpy as np
import pytest

import decoder_state_plans as S
import gzip_membergen as M
import zstd_framegen as G

pytestmark = pytest.mark.gpu
OK, CANNOT, BAD = 0, 12, 13
GUARD = 64
ODD = (1, 3, 5, 7, 9, 11, 13, 15)
WRAPPERS = {"gzip": M.GZIP, "zlib": M.ZLIB, "bgzf": M.BGZF}


class Batch:
    """The batch of S.layout(): `streams` (primers + victims) uploaded once, chunk i being streams[index[i]] by pointer,
    its capacity the stream's room, its output behind chunk i - 1's.  status_want / size_want: per stream, by default
    success or CannotDecompress and the content's length or 0; a size of None is not compared."""

    def __init__(self, hc, torch, dev, waves, primers, victims, status_want=None, size_want=None):
        self.torch, self.waves, self.primers, self.victims = torch, waves, primers, victims
        streams = self.streams = list(primers) + list(victims)
        index = S.layout(waves, primers, victims)
        self.n = len(index)
        assert self.n == 3 * waves
        table = hc.batch.from_host_chunks([s.chunk for s in streams], dev)
        self.idx = idx = torch.tensor(index, dtype=torch.int64, device=dev)
        self.comp = hc.batch.ChunkBatch(table.data, table.ptrs[idx], table.sizes[idx], table.stride)
        self.caps = torch.tensor([s.room for s in streams], dtype=torch.int64, device=dev)[idx]
        self.offs = torch.cumsum(self.caps, 0) - self.caps
        self.total = int(self.caps.sum().item())
        self.max_room = max(s.room for s in streams)
        self.arena = torch.empty(GUARD + self.total + GUARD, dtype=torch.uint8, device=dev)
        self.dst = hc.batch.ChunkBatch(self.arena, self.offs + (self.arena.data_ptr() + GUARD), torch.zeros_like(self.caps), 0)
        self.actual = torch.empty(self.n, dtype=torch.int64, device=dev)
        self.statuses = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.clear()
        # what is expected, per stream, and the contents back to back
        legal = [S.is_legal(s) for s in streams]
        if status_want is None:
            status_want = [OK if ok else CANNOT for ok in legal]
        if size_want is None:
            size_want = [len(s.content) if ok else 0 for s, ok in zip(streams, legal)]
        lens = [len(s.content) if ok else 0 for s, ok in zip(streams, legal)]
        t = lambda values, dtype=torch.int64: torch.tensor(values, dtype=dtype, device=dev)
        self.legal, self.status_want, self.len_want = t(legal, torch.bool), t(status_want, torch.int32), t(lens)
        self.size_known = t([v is not None for v in size_want], torch.bool)
        self.size_want = t([v or 0 for v in size_want])
        flat = np.frombuffer(b"".join(s.content for s in streams if S.is_legal(s)) + b"\0", dtype=np.uint8).copy()
        self.want_flat = torch.from_numpy(flat).to(dev)
        self.want_at = torch.cumsum(self.len_want, 0) - self.len_want

    def clear(self):
        self.arena.fill_(0xEE)
        self.actual.fill_(-1)
        self.statuses.fill_(-1)

    def failures(self, sizes=None):
        """-> [what is wrong with a chunk, by the names of its wave's plans], at most 8 of them"""
        torch, idx = self.torch, self.idx
        bad = (self.statuses != self.status_want[idx]) | (self.actual != torch.where(self.status_want[idx] == OK, self.len_want[idx], 0))
        if sizes is not None:
            bad |= self.size_known[idx] & (sizes != self.size_want[idx])
        # the bytes of the legal chunks: chunk and offset of every byte of the arena, then a gather of the contents
        chunk = torch.repeat_interleave(torch.arange(self.n, device=idx.device), self.caps)
        pos = torch.arange(self.total, device=idx.device) - self.offs[chunk]
        compared = self.legal[idx][chunk]
        want = self.want_flat[torch.where(compared, self.want_at[idx][chunk] + pos, 0)]
        differs = compared & (self.arena[GUARD:GUARD + self.total] != want)
        bad[chunk[differs]] = True
        out = []
        if not bool((self.arena[:GUARD] == 0xEE).all()) or not bool((self.arena[GUARD + self.total:] == 0xEE).all()):
            out.append("a byte outside the packed outputs changed")
        for i in torch.nonzero(bad).flatten()[:8].cpu().tolist():
            s = self.streams[int(idx[i])]
            first = torch.nonzero(differs & (chunk == i)).flatten()[:1].cpu().tolist()
            out.append(f"{S.describe(self.waves, self.primers, self.victims, i)}: status {int(self.statuses[i])} (expected {int(self.status_want[idx[i]])}), "
                       f"actual {int(self.actual[i])} of {len(s.content) if S.is_legal(s) else None}, capacity {s.room}"
                       + (f", size query {int(sizes[i])} (expected {int(self.size_want[idx[i]])})" if sizes is not None else "")
                       + (f", first wrong byte at {int(pos[first[0]])}" if first else ""))
        if out:
            out.insert(0, f"{int(bad.sum())} of {self.n} chunks are wrong")
        return out

    def guarded_temp(self, nbytes):
        buf = torch_full(self.torch, GUARD + nbytes + GUARD, self.arena.device)
        return buf, buf[GUARD:GUARD + nbytes]


def torch_full(torch, n, dev):
    return torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)


def temp_guards_hold(buf):
    return bool((buf[:GUARD] == 0xEE).all()) and bool((buf[-GUARD:] == 0xEE).all())


# ------------------------------------------------------------------------------------------------------ Deflate
@pytest.fixture(scope="module")
def deflate_batch(hc, cuda):
    import torch
    return Batch(hc, torch, cuda, S.DEFLATE_WAVES, S.deflate_primers(), S.deflate_victims()[0])


def test_deflate_waves_carry_nothing_to_their_next_chunk(hc, cuda, deflate_batch):
    import torch
    b = deflate_batch
    assert b.n == 3 * 8192 and len(b.primers) * len(b.victims) <= b.waves
    dec = hc.batch.DeflateDecoder()
    b.clear()
    assert dec.decompress_async(b.comp, b.caps, b.actual, None, b.dst, b.statuses) == OK
    sizes = dec.get_decompress_size(b.comp)
    torch.cuda.synchronize()
    failures = b.failures(sizes)
    assert not failures, "\n".join(failures)


def test_deflate_batch_captured_and_replayed(hc, cuda, deflate_batch):
    """the same launch captured once and replayed once onto cleared outputs (one kernel: the captured call is linear)"""
    import torch
    b = deflate_batch
    dec = hc.batch.DeflateDecoder()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert dec.decompress_async(b.comp, b.caps, b.actual, None, b.dst, b.statuses) == OK     # warm: the code object is loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert dec.decompress_async(b.comp, b.caps, b.actual, None, b.dst, b.statuses, stream=side) == OK
    b.clear()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    failures = b.failures()
    assert not failures, "\n".join(failures)


def small_failures(streams, dst, got, actual, statuses, sizes, size_want):
    """the within-chunk cases, decoded into guarded slots: -> [what is wrong with a case]"""
    out = []
    for i, s in enumerate(streams):
        if S.is_legal(s):
            if statuses[i] != OK or actual[i] != len(s.content):
                out.append(f"{s.name}: status {statuses[i]}, actual {actual[i]} of {len(s.content)}")
            elif dst.slot_bytes(got, i, len(s.content)) != s.content:
                out.append(f"{s.name}: other bytes")
        elif statuses[i] != CANNOT or actual[i] != 0:
            out.append(f"{s.name}: status {statuses[i]}, actual {actual[i]}: a refused chunk")
        if sizes[i] != size_want[i]:
            out.append(f"{s.name}: size query {sizes[i]}, expected {size_want[i]}")
    guard = dst.first_guard_change(got)
    return out + ([guard] if guard else [])


def test_deflate_blocks_carry_nothing_to_the_next_block(hc, cuda):
    import torch
    from test_deflate_gpu import run
    streams = S.deflate_within_stream()
    assert len(streams) >= 14
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [s.chunk for s in streams], [s.room for s in streams], in_offsets=ODD, out_offsets=ODD)
    failures = small_failures(streams, dst, got, actual, statuses, sizes, [len(s.content) if S.is_legal(s) else 0 for s in streams])
    assert not failures, "\n".join(failures)


# --------------------------------------------------------------------------------------------------------- gzip
@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_gzip_members_behind_a_wrong_checksum_are_untouched(hc, cuda, wrapper):
    """the Deflate layout as members: victims with a wrong CRC-32 / Adler-32 or ISIZE directly behind right members report
    the checksum status, right members stay right, refused streams stay refused"""
    import torch
    w = WRAPPERS[wrapper]
    primers, victims = S.gzip_streams(w)
    models = [M.status_model(s.chunk, w, s.room) for s in primers + victims]
    assert {st for st, _ in models} == {OK, CANNOT, BAD} and all((st == OK) == S.is_legal(s) for (st, _), s in zip(models, primers + victims))
    b = Batch(hc, torch, cuda, S.DEFLATE_WAVES, primers, victims, status_want=[st for st, _ in models],
              size_want=[len(s.content) if S.is_legal(s) else None for s in primers + victims])
    codec = hc.batch.GzipCodec(wrapper)
    buf, temp = b.guarded_temp(max(codec.decompress_temp_size(b.n, b.max_room), 8))
    assert codec.decompress_async(b.comp, b.caps, b.actual, temp, b.dst, b.statuses) == OK
    sizes = codec.get_decompress_size(b.comp)
    torch.cuda.synchronize()
    failures = b.failures(sizes)
    assert not failures, "\n".join(failures)
    assert temp_guards_hold(buf)


# ---------------------------------------------------------------------------------------------------- Zstandard
def test_zstandard_waves_carry_nothing_to_their_next_chunk(hc, cuda):
    import torch
    primers, victims = S.zstd_primers(), S.zstd_victims()[0]
    streams = primers + victims
    b = Batch(hc, torch, cuda, S.ZSTD_WAVES, primers, victims, size_want=[S.zstd_size_query_model(s) for s in streams])
    assert b.n == 3 * 3072 and b.max_room == S.PRIMER_CONTENT_MAX
    dec = hc.batch.ZstdDecoder()
    buf, temp = b.guarded_temp(dec.decompress_temp_size(b.n, b.max_room))       # a literal buffer as large as the largest primer
    assert temp.numel() == S.ZSTD_WAVES * S.PRIMER_CONTENT_MAX
    assert dec.decompress_async(b.comp, b.caps, b.actual, temp, b.dst, b.statuses) == OK
    sizes = dec.get_decompress_size(b.comp)
    torch.cuda.synchronize()
    failures = b.failures(sizes)
    assert not failures, "\n".join(failures)
    assert temp_guards_hold(buf)


def test_zstandard_frames_carry_nothing_to_the_next_frame(hc, cuda):
    import torch
    from test_zstd_gpu import run
    streams = S.zstd_within_chunk()
    assert len(streams) == 2 * len(S.zstd_primers()) * len(S.zstd_sensitive_names()) >= 360
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [s.chunk for s in streams], [s.room for s in streams])
    failures = small_failures(streams, dst, got, actual, statuses, sizes, [S.zstd_size_query_model(s) for s in streams])
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ dictionaries
def needs_libzstd():
    if G.libzstd() is None:
        pytest.skip("libzstd.so.1 does not load: what a frame gives with another dictionary is the arbiter's to say")


def test_dictionary_waves_carry_nothing_to_their_next_chunk(hc, cuda):
    """the blob of a chunk is A for a primer that needs none, the frame's own for the two that repeat a dictionary's tables,
    and A, B or none in turn for every victim: what is expected is the arbiter's with that dictionary"""
    import torch
    needs_libzstd()
    ds = S.dictionaries()
    primers, victims = S.dict_primers(), S.dict_victims()
    streams = primers + victims
    ids = {"A": ds["A"].dict_id, "B": ds["B"].dict_id, None: 0}
    b = Batch(hc, torch, cuda, S.ZSTD_WAVES, primers, victims, size_want=[S.zstd_size_query_model(s, ids[s.dictionary]) for s in streams])
    dec = hc.batch.ZstdDictDecoder()
    blobs, prepared_statuses = dec.prepare([ds["A"].bytes, ds["B"].bytes], cuda)
    ptr = {"A": int(blobs.ptrs[0]), "B": int(blobs.ptrs[1]), None: 0}
    prepared = torch.tensor([ptr[s.dictionary] for s in streams], dtype=torch.int64, device=cuda)[b.idx]
    assert int((prepared == 0).sum()) >= 500 and int((prepared == ptr["B"]).sum()) >= 500
    buf, temp = b.guarded_temp(dec.decompress_temp_size(b.n, b.max_room))
    assert dec.decompress_async(b.comp, b.caps, b.actual, temp, b.dst, b.statuses, prepared) == OK
    sizes = dec.get_decompress_size(b.comp, prepared)
    torch.cuda.synchronize()
    assert prepared_statuses.cpu().tolist() == [OK, OK]
    failures = b.failures(sizes)
    assert not failures, "\n".join(failures)
    assert temp_guards_hold(buf)


def test_dictionary_frames_carry_nothing_to_the_next_frame(hc, cuda):
    """in one chunk: a frame with its own tree and tables, then one that repeats the dictionary's; a frame that moves the
    dictionary's repeat offsets, then one that begins with a repeat code; and the plain within-chunk cases without a
    dictionary (a null blob: the plain decoder's verdict)"""
    import torch
    from test_zstd_dict_gpu import Prepared, run
    a = S.dictionary_a()
    with_a, plain = S.dict_within_chunk(), S.zstd_within_chunk()
    streams = with_a + plain
    prepared = Prepared(hc, torch, cuda, [a.bytes], [True])
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [s.chunk for s in streams], [s.room for s in streams],
                                            [prepared.ptr(a.bytes)] * len(with_a) + [0] * len(plain))
    failures = small_failures(streams, dst, got, actual, statuses, sizes,
                              [S.zstd_size_query_model(s, a.dict_id) for s in with_a] + [S.zstd_size_query_model(s, 0) for s in plain])
    assert not failures, "\n".join(failures)
