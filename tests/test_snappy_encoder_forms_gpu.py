"""The batched Snappy encoder on the planned inputs of tests/snappy_inputgen.py, against the CPU oracle.

The inputs are those tests/test_snappy_inputgen_cpu.py checks on the CPU: each is written from a plan that says
which lane of a trip of the encoder's straight path every element starts and hits at, which lanes share a hash-map
slot, what the hash map holds -- the situations a data-driven corpus meets by luck.  The compressed bytes must not
depend on the path an element took: kernel bytes == oracle bytes for EVERY case, nothing is sampled, and a failure
lists the names of all cases that differ.

All per-case chunks of all families go into one call, shuffled (so that the grid meets unlike chunks one after
another); the chunks of beyond_64k and composed go into a second call.  Inputs lie in a guarded arena
(tests/decode_guard.py) at any-byte offsets, outputs in guarded slots of max_output_chunk_size(largest chunk of the call) bytes -- the C API's
contract.  Asserted: bytes and sizes equal the oracle's, no guard byte changed, the input arena unchanged, the GPU
decoder returns every input with status 0, the size pass reports every length; where oracle/_ref exists the
reference build compresses the same batch to the same bytes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_guard as G
import snappy_inputgen as IG
from conftest import compare_with_reference

pytestmark = pytest.mark.gpu

ANY_BYTE = (0, 1, 3, 5, 7, 9, 13, 15, 4, 8, 2, 11)
LARGE = ("beyond_64k", "composed")


def _calls(seed):
    """[[(name, input)]]: the per-case chunks of all families shuffled, then the large chunks shuffled."""
    rng = np.random.default_rng(seed)
    calls = []
    for large in (False, True):
        part = [(n, d) for fam in IG.FAMILIES if (fam in LARGE) == large for n, d, _ in IG.family(fam)]
        calls.append([part[i] for i in rng.permutation(len(part))])
    return calls


def _compress(hc, torch, cuda, cases, seed, turn, lib=None):
    """One batched compress from a guarded arena into guarded slots -> {name: compressed bytes}, after the asserts
    that need the arenas (guards, input unchanged, round trip, size pass)."""
    chunks = [d for _, d in cases]
    n = len(chunks)
    largest = max(len(d) for d in chunks)
    codec = hc.batch.Codec("Snappy", lib=lib)
    cap = codec.max_output_chunk_size(largest)
    inp = G.GuardedSlots(torch, [len(d) for d in chunks], cuda, offsets=ANY_BYTE, turn=turn, seed=seed + 1,
                         chunks=chunks)
    out = G.GuardedSlots(torch, [cap] * n, cuda, offsets=ANY_BYTE, turn=turn + 5, seed=seed + 2)
    dst = out.batch(hc)
    temp = torch.zeros(max(codec.compress_temp_size(n, largest), 8), dtype=torch.uint8, device=cuda)
    assert codec.compress_async(inp.batch(hc), largest, temp, dst) == 0
    torch.cuda.synchronize()
    got = out.after()
    bad = out.first_guard_change(got)
    assert bad is None, f"compress wrote outside its slots: {bad}"
    assert inp.unchanged() is None, f"compress wrote into its input: {inp.unchanged()}"
    sizes = dst.sizes.cpu().tolist()
    assert all(0 < s <= cap for s in sizes), "a reported size is outside the slot"
    if lib is None:
        sized = codec.get_decompress_size(dst).cpu().tolist()
        wrong = [name for (name, d), s in zip(cases, sized) if s != len(d)]
        assert not wrong, f"size pass: {len(wrong)} lengths wrong: {wrong[:20]}"
        dec, actual, statuses = codec.decompress(dst, max(largest, 1))
        torch.cuda.synchronize()
        st, ac = statuses.cpu().tolist(), actual.cpu().tolist()
        wrong = [name for i, (name, d) in enumerate(cases)
                 if st[i] != 0 or ac[i] != len(d) or dec.chunk_bytes(i, len(d)) != d]
        assert not wrong, f"round trip: {len(wrong)} of {n} inputs not returned with status 0: {wrong[:20]}"
    return {name: out.slot_bytes(got, i, sizes[i]) for i, (name, _) in enumerate(cases)}


def _against_oracle(oracle, cases, got, what):
    wrong = []
    for name, d in cases:
        want = oracle.snappy_compress(d)
        if got[name] != want:
            wrong.append(f"{name} ({len(got[name])} bytes, oracle {len(want)})")
    by_family = sorted({w.split("/")[0] for w in wrong})
    assert not wrong, (f"{what}: {len(wrong)} of {len(cases)} cases differ from the oracle (families {by_family}): "
                       + ", ".join(wrong))


def test_every_planned_case_compresses_to_the_oracle_bytes(hc, oracle, reflib, cuda):
    import torch
    total = 0
    for j, cases in enumerate(_calls(29)):
        total += len(cases)
        print(f"Snappy call {j}: {len(cases)} chunks, {sum(len(d) for _, d in cases)} input bytes")
        got = _compress(hc, torch, cuda, cases, 300 + 10 * j, turn=j)
        _against_oracle(oracle, cases, got, f"call {j}")
    assert total == sum(len(IG.family(f)) for f in IG.FAMILIES)

    def check(reflib):
        for j, cases in enumerate(_calls(29)):
            want = {n: oracle.snappy_compress(d) for n, d in cases}
            # (the reference build: plain batches -- its reads are not bounded the way the guarded arena asks for)
            src = hc.batch.from_host_chunks([d for _, d in cases], "cuda:0")
            r = hc.batch.Codec("Snappy", lib=reflib).compress(src)
            torch.cuda.synchronize()
            refgot = r.to_host_chunks()
            wrong = [n for i, (n, _) in enumerate(cases) if refgot[i] != want[n]]
            assert not wrong, f"reference build, call {j}: {len(wrong)} cases differ from the oracle: {wrong}"
    compare_with_reference(reflib, "Snappy planned inputs", check)


def test_second_run_with_another_shuffle_gives_the_same_bytes(hc, oracle, cuda):
    """The same batch twice in one process, the second time in another order and at other offsets: what one chunk
    leaves behind (the hash map in LDS, the slot) must not reach the next."""
    import torch
    for j in range(2):
        first = _compress(hc, torch, cuda, _calls(29)[j], 400 + 10 * j, turn=0)
        again_cases = _calls(31)[j]
        again = _compress(hc, torch, cuda, again_cases, 500 + 10 * j, turn=7)
        assert [n for n, _ in again_cases] != [n for n, _ in _calls(29)[j]]
        wrong = sorted(n for n in first if first[n] != again[n])
        assert not wrong, f"call {j}: {len(wrong)} cases compress differently the second time: {wrong}"
        _against_oracle(oracle, again_cases, again, f"second run, call {j}")


def test_parity_sweep_over_chunk_sizes(cuda):
    """scripts/parity_sweep_snappy.py: text, integers, runs, vocabulary, periodic and small-alphabet data at eleven
    chunk sizes around the straight path's margin and the 64 KiB line -- kernel bytes == oracle bytes, round trip."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "parity_sweep_snappy.py")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "TOTAL BAD 0" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
