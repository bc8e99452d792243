"""The batched Zstandard decoder with dictionaries on the GPU (include/hipcomp/zstd_dict.h) through api.py and batch.py.
Every planned dictionary (tests/zstd_dictgen.py) and the three fixture dictionaries (tests/zstd_dict_fixtures.py) are
prepared in one launch; every planned and fixture frame, legal and illegal, is decoded in one mixed batch with per-chunk
blobs and null entries among them.  What is expected is libzstd's verdict and bytes, to which tests/test_zstd_dict_cpu.py
holds the plans and the fixture on the CPU.  Inputs, outputs, blobs and the temp space lie between guard bytes
(tests/decode_guard.py)."""
import numpy as np
import pytest

import zstd_dict_fixtures as F
import zstd_dictgen as D
import zstd_framegen as G
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu
OK, CANNOT, INVALID = 0, 12, 10
ODD = (1, 3, 5, 7, 9, 11, 13, 15)
HEADER = 64
CONTENT_AT = 9280


class Prepared:
    """dictionaries digested by one prepare launch: blob i of dictionaries[i] in a guarded slot of its own"""

    def __init__(self, hc, torch, dev, dictionaries, legal):
        self.dec = hc.batch.ZstdDictDecoder()
        self.dictionaries = list(dictionaries)
        self.sizes = [self.dec.prepared_size(len(d)) for d in self.dictionaries]
        src = GuardedSlots(torch, [len(d) for d in self.dictionaries], dev, offsets=ODD, seed=31, chunks=self.dictionaries)
        # a refused dictionary leaves a header marked invalid and nothing else
        self.blobs = GuardedSlots(torch, self.sizes, dev, seed=32, region=[s if ok else HEADER for s, ok in zip(self.sizes, legal)])
        self.statuses_t = torch.full((len(self.sizes),), -1, dtype=torch.int32, device=dev)
        st = self.dec.lib.hipcompBatchedZstdDictPrepareAsync(
            src.ptrs.data_ptr(), src.sizes.data_ptr(), len(self.sizes), self.blobs.ptrs.data_ptr(), self.blobs.caps_t.data_ptr(),
            self.statuses_t.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
        assert st == OK
        torch.cuda.synchronize()
        assert src.unchanged() is None, src.unchanged()
        self.after = self.blobs.after()
        assert self.blobs.first_guard_change(self.after) is None, self.blobs.first_guard_change(self.after)
        self.statuses = self.statuses_t.cpu().tolist()
        self.ptrs = self.blobs.ptrs.cpu().tolist()
        self.index = {}
        for i, d in enumerate(self.dictionaries):
            self.index.setdefault(d, i)

    def ptr(self, dictionary):
        """the blob of a dictionary given as bytes; None: no dictionary (a null entry)"""
        return 0 if dictionary is None else self.ptrs[self.index[dictionary]]

    def header(self, i):
        at = int(self.blobs.at[i])
        return np.frombuffer(self.after[at:at + HEADER].tobytes(), dtype=np.uint32).tolist()


def run(hc, torch, dev, chunks, caps, blob_ptrs, in_offsets=ODD, out_offsets=ODD, turn=3):
    """one decode launch and one size query -> (output slots, arena after, actual, statuses, sizes)"""
    n = len(chunks)
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=in_offsets, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, caps, dev, offsets=out_offsets, turn=turn, seed=22)
    dec = hc.batch.ZstdDictDecoder()
    tbytes = dec.decompress_temp_size(n, max(caps))
    temp = GuardedSlots(torch, [tbytes], dev, seed=23)
    prepared = torch.tensor(blob_ptrs, dtype=torch.int64, device=dev)
    actual = torch.full((n,), -1, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st = dec.lib.hipcompBatchedZstdDictDecompressAsync(
        src.ptrs.data_ptr(), src.sizes.data_ptr(), dst.caps_t.data_ptr(), actual.data_ptr(), n, int(temp.ptrs[0].item()), tbytes,
        dst.ptrs.data_ptr(), statuses.data_ptr(), prepared.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
    assert st == OK
    sizes = dec.get_decompress_size(src.batch(hc), prepared)
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()
    assert temp.first_guard_change() is None, "temp space: " + str(temp.first_guard_change())
    return dst, dst.after(), actual.cpu().tolist(), statuses.cpu().tolist(), sizes.cpu().tolist()


def check(dst, got, actual, statuses, cases):
    """cases: [(name, chunk, dictionary, content or None)]"""
    for i, (name, _, _, want) in enumerate(cases):
        if want is None:
            assert statuses[i] == CANNOT and actual[i] == 0, (name, statuses[i], actual[i])
        else:
            assert statuses[i] == OK and actual[i] == len(want), (name, statuses[i], actual[i], len(want))
            assert dst.slot_bytes(got, i, len(want)) == want, name
            dst.region[i] = len(want)
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)


def all_cases():
    """[(name, chunk, dictionary bytes or None, content or None)]: the planned frames against their dictionaries, the
    fixture frames against theirs, and planned frames of tests/zstd_framegen.py without one"""
    dicts, frames, _ = F.load()
    plain = [(n, c, None, w) for n, c, w, _ in G.legal_plans() if len(w) <= 4096] + [(n, c, None, None) for n, c in G.illegal_plans()]
    return D.planned_frames() + [(n, c, dicts[dn], w) for n, c, w, dn in frames] + plain


def all_dictionaries():
    """[(name, dictionary, legal?)]"""
    dicts, _, _ = F.load()
    return [(n, d, True) for n, d in dicts.items()] + D.planned_dictionaries()


@pytest.fixture(scope="module")
def prepared(hc, cuda):
    import torch
    cases = all_cases()
    named = all_dictionaries()
    assert {d for _, _, d, _ in cases if d is not None} <= {d for _, d, _ in named}
    return Prepared(hc, torch, cuda, [d for _, d, _ in named], [ok for _, _, ok in named])


@pytest.fixture(scope="module")
def mixed(hc, cuda, prepared):
    import torch
    cases = all_cases()
    caps = [len(w) if w is not None else 4096 for _, _, _, w in cases]
    return cases, run(hc, torch, cuda, [c for _, c, _, _ in cases], caps, [prepared.ptr(d) for _, _, d, _ in cases])


def test_prepare_statuses_are_libzstds_verdicts(prepared):
    named = all_dictionaries()
    assert len(named) >= 50
    for i, (name, d, legal) in enumerate(named):
        assert prepared.statuses[i] == (OK if legal else CANNOT), (name, prepared.statuses[i])
        h = prepared.header(i)
        assert h[2] == int(legal) and h[14] == (prepared.sizes[i] if legal else HEADER), (name, h)
        if legal:
            formatted = len(d) >= 8 and d[:4] == (0xEC30A437).to_bytes(4, "little")
            assert h[3] == (int.from_bytes(d[4:8], "little") if formatted else 0) and h[4] == int(formatted) and h[12] == CONTENT_AT, name
            at = int(prepared.blobs.at[i]) + CONTENT_AT
            assert prepared.after[at:at + h[13]].tobytes() == d[len(d) - h[13]:], name


def test_one_mixed_batch_equals_the_arbiter(mixed):
    cases, (dst, got, actual, statuses, sizes) = mixed
    assert 150 <= len(cases) <= 512 and max(len(w or b"") for _, _, _, w in cases) == 300 * 1024
    assert sum(d is None for _, _, d, _ in cases) >= 30 and sum(w is None for _, _, _, w in cases) >= 40
    check(dst, got, actual, statuses, cases)


def test_size_query_agrees_with_the_decode(mixed):
    cases, (dst, got, actual, statuses, sizes) = mixed
    undeclared = 0
    for (name, chunk, d, want), size, status in zip(cases, sizes, statuses):
        if want is not None:
            assert size == len(want), name
            undeclared += "fcs_0" in G.inspect(chunk)
        elif size != 0:      # the query walked headers that declare a size: the decode found the chunk illegal
            assert status == CANNOT, name
    assert undeclared >= 3
    by_name = {n: s for (n, _, _, _), s in zip(cases, sizes)}
    for name in ("dictionary_id_different", "dictionary_id_against_raw_content", "dictionary_id_without_a_dictionary",
                 "dictionary_id_of_another_dictionary", "dictionary_refused", "undeclared_size_offset_beyond"):
        assert by_name[name] == 0, name


def test_null_blobs_give_what_the_plain_decoder_gives(hc, cuda):
    import torch
    cases = all_cases()
    cases = [c for c in cases if len(c[1]) <= 20000]
    chunks = [c for _, c, _, _ in cases]
    caps = [len(w) if w is not None else 4096 for _, _, _, w in cases]
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, chunks, caps, [0] * len(cases))
    # the same slots through include/hipcomp/zstd.h
    src = GuardedSlots(torch, [len(c) for c in chunks], cuda, offsets=ODD, seed=21, chunks=chunks)
    ref = GuardedSlots(torch, caps, cuda, offsets=ODD, turn=3, seed=22)
    dec = hc.batch.ZstdDecoder()
    tbytes = dec.decompress_temp_size(len(cases), max(caps))
    temp = torch.empty(tbytes, dtype=torch.uint8, device=cuda)
    ref_actual = torch.full((len(cases),), -1, dtype=torch.int64, device=cuda)
    ref_statuses = torch.full((len(cases),), -1, dtype=torch.int32, device=cuda)
    assert dec.lib.hipcompBatchedZstdDecompressAsync(
        src.ptrs.data_ptr(), src.sizes.data_ptr(), ref.caps_t.data_ptr(), ref_actual.data_ptr(), len(cases), temp.data_ptr(), tbytes,
        ref.ptrs.data_ptr(), ref_statuses.data_ptr(), int(torch.cuda.current_stream().cuda_stream)) == OK
    ref_sizes = dec.get_decompress_size(src.batch(hc))
    torch.cuda.synchronize()
    ref_got = ref.after()
    assert statuses == ref_statuses.cpu().tolist() and actual == ref_actual.cpu().tolist() and sizes == ref_sizes.cpu().tolist()
    assert OK in statuses and CANNOT in statuses
    for i, (name, _, _, _) in enumerate(cases):
        if statuses[i] == OK:
            assert dst.slot_bytes(got, i, actual[i]) == ref.slot_bytes(ref_got, i, actual[i]), name
    # a frame that needs its dictionary is refused or decodes to other bytes; one with a Dictionary_ID is refused
    by_name = {n: s for (n, _, _, _), s in zip(cases, statuses)}
    assert by_name["dictionary_id_equal"] == CANNOT and by_name["treeless_first_block"] == CANNOT and by_name["dictionary_id_absent"] == OK


def test_frames_of_one_dictionary_against_another_are_refused(hc, cuda, prepared):
    import torch
    dicts, frames, _ = F.load()
    of_a = [(n, c, w) for n, c, w, dn in frames if dn == "a" and c[4] & 3 and len(w) <= 5000]
    assert len(of_a) >= 12
    cases = [(n, c, dicts["b"], None) for n, c, w in of_a] + [(n, c, dicts["raw"], None) for n, c, w in of_a] + \
            [(n, c, dicts["a"], w) for n, c, w in of_a]
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [c for _, c, _, _ in cases], [5000] * len(cases),
                                            [prepared.ptr(d) for _, _, d, _ in cases])
    check(dst, got, actual, statuses, cases)
    assert sizes[:2 * len(of_a)] == [0] * (2 * len(of_a))


def test_a_blob_copied_to_another_address_decodes_the_same(hc, cuda, prepared):
    import torch
    dicts, frames, _ = F.load()
    cases = [c for c in D.planned_frames() if c[2] is not None and c[3] is not None] + \
            [(n, c, dicts[dn], w) for n, c, w, dn in frames if len(w) <= 5000]
    used = sorted({d for _, _, d, _ in cases})
    # the copies: back to back in a new allocation, 16-byte aligned, in another order
    sizes = {d: prepared.sizes[prepared.index[d]] for d in used}
    arena = torch.empty(sum(sizes.values()) + 48, dtype=torch.uint8, device=cuda)
    at, where = (-arena.data_ptr()) % 16 + 32, {}
    for d in reversed(used):
        i = prepared.index[d]
        lo = int(prepared.blobs.at[i])
        arena[at:at + sizes[d]] = prepared.blobs.data[lo:lo + sizes[d]]
        where[d] = arena.data_ptr() + at
        at += sizes[d]
    assert all(p % 16 == 0 and p not in prepared.ptrs for p in where.values())
    dst, got, actual, statuses, _ = run(hc, torch, cuda, [c for _, c, _, _ in cases], [len(w) for _, _, _, w in cases],
                                        [where[d] for _, _, d, _ in cases])
    check(dst, got, actual, statuses, cases)


def test_every_alignment_of_input_output_and_content(hc, cuda, prepared):
    """inputs and outputs at every pair of offsets mod 16 drawn from {0, 1, 7, 15}, the match beginning at content[16 k + c]
    for c in the same set (the blob itself is 16-byte aligned, so that is the source's address mod 16)"""
    import torch
    plans = {n: (c, d, w) for n, c, d, w in D.planned_frames()}
    cases, ins, outs = [], [], []
    for tag in ("formatted", "raw"):
        for c in (0, 1, 7, 15):
            chunk, d, want = plans[f"match_begins_at_content_{c}_mod_16_{tag}"]
            for i in (0, 1, 7, 15):
                for o in (0, 1, 7, 15):
                    cases.append((f"{tag} content {c} in {i} out {o}", chunk, d, want))
                    ins.append(i)
                    outs.append(o)
    assert len(cases) == 128
    dst, got, actual, statuses, _ = run(hc, torch, cuda, [c for _, c, _, _ in cases], [len(w) for _, _, _, w in cases],
                                        [prepared.ptr(d) for _, _, d, _ in cases], in_offsets=ins, out_offsets=outs, turn=0)
    assert (dst.at % 16).tolist() == outs
    check(dst, got, actual, statuses, cases)


def test_prepare_refuses_a_misplaced_blob(hc, cuda):
    """a blob pointer that is not 16-byte aligned, a capacity one below the size query's answer, and too small for a header"""
    import torch
    dec = hc.batch.ZstdDictDecoder()
    d = D.formatted().bytes
    need = dec.prepared_size(len(d))
    dicts = hc.batch.from_host_chunks([d] * 4, cuda)
    blobs = GuardedSlots(torch, [need] * 4, cuda, seed=41, region=[need, 0, HEADER, 0])
    ptrs = blobs.ptrs.clone()
    ptrs[1] += 8
    caps = torch.tensor([need, need, need - 1, HEADER - 1], dtype=torch.int64, device=cuda)
    statuses = torch.full((4,), -1, dtype=torch.int32, device=cuda)
    assert dec.lib.hipcompBatchedZstdDictPrepareAsync(dicts.ptrs.data_ptr(), dicts.sizes.data_ptr(), 4, ptrs.data_ptr(), caps.data_ptr(),
                                                       statuses.data_ptr(), int(torch.cuda.current_stream().cuda_stream)) == OK
    torch.cuda.synchronize()
    assert statuses.cpu().tolist() == [OK, INVALID, INVALID, INVALID]
    after = blobs.after()
    assert blobs.first_guard_change(after) is None, blobs.first_guard_change(after)
    header = lambda i: np.frombuffer(after[int(blobs.at[i]):int(blobs.at[i]) + HEADER].tobytes(), dtype=np.uint32).tolist()
    assert header(0)[2] == 1 and header(2)[2] == 0 and header(2)[0] == header(0)[0]
    # a chunk that names the blob marked invalid is refused
    chunk, content = D.frame(None, [("raw", b"needs nothing")])
    src = hc.batch.from_host_chunks([chunk] * 2, cuda)
    prepared = torch.tensor([int(blobs.ptrs[0].item()), int(blobs.ptrs[2].item())], dtype=torch.int64, device=cuda)
    out, actual, st = dec.decompress(src, 64, prepared)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [OK, CANNOT] and actual.cpu().tolist() == [len(content), 0]
    assert out.chunk_bytes(0, len(content)) == content
    assert dec.get_decompress_size(src, prepared).cpu().tolist() == [len(content), 0]
