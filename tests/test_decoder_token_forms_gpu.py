"""The batched LZ4 and Snappy decoders on every legal token form, against the plain reference.

The streams come from tests/streamgen.py at the seeds tests/test_streamgen_cpu.py checks on the CPU: every LZ4
family in both kinds (conforming and reference-accepted), liblz4's own streams where liblz4 is present, every
Snappy family.  The expected output is streamgen's plain loop (matches one byte at a time); nothing is sampled.

All families of a codec go into one call (streams of more than 64 KiB in a second call of their own, so that the
guarded arena stays small), shuffled, so that the persistent LZ4 ticket grid and the Snappy grid meet unlike chunks
one after another.  Outputs lie in guarded slots (tests/decode_guard.py) at varying offsets from 16-byte
boundaries, at three capacities:
  * exact: cap = len(expected) for every chunk (the last steps of a chunk run with less than 64 bytes of room);
  * roomy: cap = the largest expected size of the call, for every chunk;
  * short: cap = len(expected) - 1 (0 for an empty output) -- status, reported size and on success the bytes must
    be the oracle's at that capacity.  (Snappy reads a capacity of 0 as "the size the stream declares", so the
    streams of 0 and 1 output bytes decode in full there, on both sides; every other stream is one byte short.)
At the first two every chunk must report status 0 and its size and hold exactly the expected bytes, and the size
pass must report every expected size; at all three no guard byte may change.  Where oracle/_ref exists the
reference build decodes the same streams to the same bytes.
"""
import numpy as np
import pytest

import decode_guard as G
import streamgen as SG
from conftest import compare_with_reference

pytestmark = pytest.mark.gpu

ANY_BYTE = (0, 1, 3, 5, 7, 9, 13, 15, 4, 8, 2, 11)
SMALL = 65536


def _cases(codec):
    """[(name, stream, expected)] of every family of the codec."""
    out = []
    if codec == "LZ4":
        for conforming in (True, False):
            for fam in SG.LZ4_FAMILIES:
                for k, (s, e, _) in enumerate(SG.lz4_family(fam, conforming)):
                    out.append((f"{fam}/{'conforming' if conforming else 'accepted'}/{k}", s, e))
    else:
        for fam in SG.SNAPPY_FAMILIES:
            out += [(f"{fam}/{k}", s, e) for k, (s, e, _) in enumerate(SG.snappy_family(fam))]
    return out


def _calls(codec, seed):
    """The cases split by expected size (<= 64 KiB, larger) and shuffled within each call."""
    cases = _cases(codec)
    rng = np.random.default_rng(seed)
    calls = []
    for pick in (lambda e: len(e) <= SMALL, lambda e: len(e) > SMALL):
        part = [c for c in cases if pick(c[2])]
        calls.append([part[i] for i in rng.permutation(len(part))])
    return calls


def _decode(hc, torch, cuda, codec, cases, caps, seed, lib=None):
    """One batched decode into guarded slots -> (slots, arena bytes after, statuses, actual sizes)."""
    n = len(cases)
    streams = [s for _, s, _ in cases]
    inp = G.GuardedSlots(torch, [len(s) for s in streams], cuda, offsets=ANY_BYTE, turn=5, seed=seed + 1,
                         chunks=streams)
    # (Snappy: capacity 0 means the size the stream declares -- snappy_kernels.hip, and the oracle)
    region = [len(e) if codec == "Snappy" and c == 0 else c for (_, _, e), c in zip(cases, caps)]
    out = G.GuardedSlots(torch, caps, cuda, offsets=ANY_BYTE, seed=seed + 2, region=region)
    actual = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    c = hc.batch.Codec(codec, lib=lib)
    temp = None
    if codec == "LZ4":   # (a temp buffer: the persistent grid draws chunks from its ticket counter)
        temp = torch.zeros(max(c.decompress_temp_size(n, max(caps + [1])), 8), dtype=torch.uint8, device=cuda)
    assert c.decompress_async(inp.batch(hc), out.caps_t, actual, temp, out.batch(hc), statuses) == 0
    torch.cuda.synchronize()
    assert inp.unchanged() is None, f"{codec}: the compressed input was written: {inp.unchanged()}"
    return inp, out, out.after(), statuses.cpu().tolist(), actual.cpu().tolist()


def _check_valid(hc, torch, cuda, codec, cases, caps, what, seed):
    inp, out, got, st, ac = _decode(hc, torch, cuda, codec, cases, caps, seed)
    bad = out.first_guard_change(got)
    assert bad is None, f"{codec} {what}: {bad}"
    wrong = []
    for i, (name, s, e) in enumerate(cases):
        if st[i] != 0 or ac[i] != len(e) or out.slot_bytes(got, i, len(e)) != e:
            wrong.append(f"{name} (status {st[i]}, size {ac[i]} of {len(e)})")
    assert not wrong, f"{codec} {what}: {len(wrong)} of {len(cases)} streams wrong, first {wrong[:5]}"
    return inp


@pytest.mark.parametrize("codec", ["LZ4", "Snappy"])
def test_every_token_form_decodes_to_the_plain_reference(hc, oracle, reflib, cuda, codec):
    import torch
    total = 0
    for j, cases in enumerate(_calls(codec, 17)):
        if not cases:
            continue
        total += len(cases)
        exact = [len(e) for _, _, e in cases]
        print(f"{codec} call {j}: {len(cases)} streams, {sum(exact)} output bytes, largest {max(exact)}")
        inp = _check_valid(hc, torch, cuda, codec, cases, exact, "cap = len(expected)", 100 + 10 * j)
        got = hc.batch.Codec(codec).get_decompress_size(inp.batch(hc)).cpu().tolist()
        wrong = [cases[i][0] for i in range(len(cases)) if got[i] != exact[i]]
        assert not wrong, f"{codec} size pass: {len(wrong)} streams wrong, first {wrong[:5]}"
        _check_valid(hc, torch, cuda, codec, cases, [max(exact)] * len(cases), "cap = max", 103 + 10 * j)

        short = [max(n - 1, 0) for n in exact]
        want = [(oracle.lz4_decompress if codec == "LZ4" else oracle.snappy_decompress)(s, c)
                for (_, s, _), c in zip(cases, short)]
        _, out, got, st, ac = _decode(hc, torch, cuda, codec, cases, short, 106 + 10 * j)
        bad = out.first_guard_change(got)
        assert bad is None, f"{codec} cap = len(expected) - 1: {bad}"
        wrong = [f"{cases[i][0]} ({st[i]}, {ac[i]}) != oracle ({w[0]}, {len(w[1])})" for i, w in enumerate(want)
                 if (st[i], ac[i]) != (w[0], len(w[1]))
                 or (w[0] == 0 and out.slot_bytes(got, i, len(w[1])) != w[1])]
        assert not wrong, f"{codec} cap = len(expected) - 1: {len(wrong)} streams wrong, first {wrong[:5]}"
    assert total == len(_cases(codec))

    def check(reflib):
        for j, cases in enumerate(_calls(codec, 17)):
            if not cases:
                continue
            exact = [len(e) for _, _, e in cases]
            # (4 KiB behind every stream: the reference's reads of a stream are not bounded by its length)
            streams = [s for _, s, _ in cases]
            rb = hc.batch.from_host_chunks(streams, "cuda:0", stride=max(len(s) for s in streams) + 4096)
            dec, actual, statuses = hc.batch.Codec(codec, lib=reflib).decompress(rb, max(exact))
            torch.cuda.synchronize()
            st, ac = statuses.cpu().tolist(), actual.cpu().tolist()
            wrong = [name for i, (name, s, e) in enumerate(cases)
                     if st[i] != 0 or ac[i] != len(e) or dec.chunk_bytes(i, len(e)) != e]
            assert not wrong, f"{codec} reference build: {len(wrong)} streams differ, first {wrong[:5]}"
    compare_with_reference(reflib, f"{codec} token-form streams", check)
