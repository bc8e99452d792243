"""The Zstandard encoder's kernel held to the scalar encoder, byte for byte, on the planned inputs of
tests/zstd_inputgen.py (tests/test_zstd_inputgen_cpu.py says what they reach) and on the generic inputs of
tests/test_zstd_compress_gpu.py.

A round trip proves that a frame is legal, not that it is the frame this encoder is specified to write.  Here a
kernel frame is read back into its tokens (tests/zstd_seqscan.py), the tokens are checked against the plan of the
case, and the scalar encoder of tests/zstd_codes_driver.cpp -- zstd_codes.hpp's encode_frame, which makes every
decision the kernel makes from the chunk and a token list -- writes the frame again from them: the two are
identical, whatever the parse chose.  The driver is built here with plain g++ -O1; its sanitizer builds are the CPU
tests'.  Every buffer lies in decode_guard.GuardedSlots, the temp space included."""
import os
import subprocess

import numpy as np
import pytest

import test_zstd_compress_gpu as T
import zstd_inputgen as Z
import zstd_seqscan as S
from decode_guard import GuardedSlots
from test_zstd_codes_cpu import CSRC, ENC_INCLUDES, ROOT, encode_all

pytestmark = pytest.mark.gpu

CHECKSUM = 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zstd_edges") / "zstd_codes_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + ENC_INCLUDES
                       + [os.path.join(ROOT, "tests", "zstd_codes_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return (exe,)


@pytest.fixture(scope="module")
def planned(hc, cuda, driver, tmp_path_factory):
    """-> (cases, kernel frames without and with the checksum, the scalar encoder's frames of the planned tokens)"""
    import torch
    cases = Z.kernel_cases()
    assert len(cases) <= 400
    chunks = [c.content for c in cases]
    frames = {cs: T.compress_guarded(hc, torch, cuda, chunks, checksum=bool(cs))[0] for cs in (0, CHECKSUM)}
    scalar = encode_all(driver, tmp_path_factory.mktemp("planned"), [(c.content, c.scalar_tokens(), 0) for c in cases])
    return cases, frames, scalar


def test_planned_parses(planned):
    cases, frames, scalar = planned
    compressed = 0
    for c, f, want in zip(cases, frames[0], scalar):
        if c.tokens is None:
            continue
        kind = S.compressed_block(want)[0]
        assert S.compressed_block(f)[0] == kind, c.name
        if kind == 2:
            compressed += 1
            assert S.tokens_of(f) == c.tokens, c.name
    print("%d planned cases, %d of them compressed blocks whose tokens equal the plan" % (sum(c.tokens is not None for c in cases), compressed))
    assert compressed >= 260


def held_to_the_scalar_encoder(hc, cuda, driver, tmp_path, named, plans, frames, with_sum):
    """frames: the kernel's without the checksum, with_sum: with it.  plans: per case the planned tokens that stand
    in where the kernel's frame holds none (a block that was not kept), else None."""
    import torch
    jobs = []
    for (name, data), plan, f, fs in zip(named, plans, frames, with_sum):
        tokens = S.tokens_of(f)
        if tokens is None:
            tokens = plan or []
        else:
            assert Z.rebuilds(data, tokens), name
            assert Z.maximal(data, tokens), name
            assert all(ml >= 4 and 1 <= off <= 65535 for _, ml, off in tokens), name
        # the checksum changes the descriptor's flag and adds four bytes, nothing else
        assert fs[:4] == f[:4] and fs[4] == f[4] | 4 and fs[5:-4] == f[5:], name
        jobs += [(data, tokens, 0), (data, tokens, CHECKSUM)]
    scalar = encode_all(driver, tmp_path, jobs)
    for k, ((name, data), f, fs) in enumerate(zip(named, frames, with_sum)):
        assert f == scalar[2 * k], name
        assert fs == scalar[2 * k + 1], name
    T.check_round_trip(hc, torch, cuda, named, frames)
    T.check_round_trip(hc, torch, cuda, named, with_sum)


def test_frames_equal_the_scalar_encoder(hc, cuda, driver, planned, tmp_path):
    cases, frames, _ = planned
    # a block that the kernel did not keep is held to the scalar encoder's decision on the PLANNED tokens
    held_to_the_scalar_encoder(hc, cuda, driver, tmp_path, [(c.name, c.content) for c in cases], [c.tokens for c in cases],
                               frames[0], frames[CHECKSUM])


def test_generic_frames_equal_the_scalar_encoder(hc, cuda, driver, tmp_path):
    import torch
    named = T.shared_cases()
    chunks = [d for _, d in named]
    frames = {cs: T.compress_guarded(hc, torch, cuda, chunks, checksum=bool(cs))[0] for cs in (0, CHECKSUM)}
    held_to_the_scalar_encoder(hc, cuda, driver, tmp_path, named, [None] * len(named), frames[0], frames[CHECKSUM])


def test_temp_space_is_contained(hc, cuda):
    """the temp space as a guarded slot filled with a pattern: the guards stay, and inside a wave's slice only the
    records of the chunk's sequences, rounded up to 64, and its literals change"""
    import torch
    by = {c.name: c for c in Z.kernel_cases()}
    cases = [by[f"counts/n{Z.MANY_SEQUENCES}"], by["codes/ll65532_offset65532"], by["trip/tail1"]]
    chunks = [c.content for c in cases]
    n, max_chunk = len(chunks), max(len(c) for c in chunks)
    assert max_chunk == 65536
    enc = hc.batch.ZstdEncoder()
    size = enc.compress_temp_size(n, max_chunk)
    records = (max_chunk // 4 + 64) // 64 * 64
    per_wave = 8 * records + (max_chunk + 256) // 256 * 256
    assert size == n * per_wave
    temp = GuardedSlots(torch, [size], cuda, seed=23)
    at = int(temp.at[0])
    src = GuardedSlots(torch, [len(c) for c in chunks], cuda, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, [T.bound(max_chunk)] * n, cuda, seed=22)
    out_batch = dst.batch(hc)
    out_batch.sizes = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    assert enc.compress_async(src.batch(hc), max_chunk, temp.data[at:at + size], out_batch) == 0
    torch.cuda.synchronize()
    got = temp.after()
    assert temp.first_guard_change(got) is None, temp.first_guard_change(got)
    assert src.unchanged() is None and dst.first_guard_change() is None
    changed = got[at:at + size] != temp.host[at:at + size]
    for w, c in enumerate(cases):                # wave w takes chunk w
        mine, words = changed[w * per_wave:(w + 1) * per_wave], got[at + w * per_wave:at + (w + 1) * per_wave]
        nseq, lits = len(c.tokens), Z.literals_of(c.content, c.tokens)
        nlit = len(lits)                         # (those behind the last match are gathered too)
        stored = (nseq + 63) // 64 * 64
        for k, what in enumerate(("literal run | offset << 16", "match length")):
            rec = mine[4 * records * k:4 * records * (k + 1)]
            assert not rec[4 * stored:].any(), (c.name, what, int(np.flatnonzero(rec)[-1]) // 4)
        assert not mine[8 * records + nlit:].any(), (c.name, int(np.flatnonzero(mine)[-1]) - 8 * records)
        rec_a = words[:4 * nseq].view("<u4")
        rec_b = words[4 * records:4 * records + 4 * nseq].view("<u4")
        assert rec_a.tolist() == [ll | off << 16 for ll, _, off in c.tokens], c.name
        assert rec_b.tolist() == [ml for _, ml, _ in c.tokens], c.name
        assert words[8 * records:8 * records + nlit].tobytes() == lits, c.name


@pytest.mark.parametrize("first, second", [("fat/extra15_v0", "trip/tail1"), (f"counts/n{Z.MANY_SEQUENCES}", "near_rle/len4_at1"),
                                           ("codes/ll65532_offset65532", "limit/copies1_L9")])
def test_tail_of_a_grid_stride_trip(hc, cuda, planned, first, second):
    """The planned batch repeated by a device-side gather to one more chunk than the 3072 waves of the grid: wave 0
    takes `first`, a chunk that fills its LDS and its buffers, and in its second trip `second`, a small one.
    Every frame is the one of the planned batch."""
    import torch
    cases, frames, _ = planned
    names = [c.name for c in cases]
    k, n, cap = len(cases), 3073, 65536
    table = hc.batch.from_host_chunks([c.content for c in cases], cuda, stride=cap)
    pick = (torch.arange(n, device=cuda) + names.index(first)) % k
    pick[n - 1] = names.index(second)
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, n, table.stride), table.sizes[pick], table.stride)
    comp = hc.batch.ZstdEncoder().compress(src, cap)
    torch.cuda.synchronize()
    want = hc.batch.from_host_chunks(frames[0], cuda, stride=comp.stride)
    assert torch.equal(comp.sizes, want.sizes[pick])
    got = comp.data[: n * comp.stride].view(n, comp.stride)
    exp = want.data[: k * want.stride].view(k, want.stride)[pick]
    inside = torch.arange(comp.stride, device=cuda)[None, :] < comp.sizes[:, None]
    differs = ((got != exp) & inside).any(dim=1)
    assert not bool(differs.any()), [names[int(pick[i])] for i in torch.nonzero(differs).flatten()[:5].tolist()]
