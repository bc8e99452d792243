"""The batched Cascaded decoder on legal streams its encoder never writes, against the plain reference.

The streams are the whole corpus of tests/cascaded_streamgen.py (empty runs, every bit width, frames of reference
that wrap, arrays inside, across and behind the staged first KiB of a sub-chunk, slack, ragged sub-chunks, every
depth the metadata block allows, raw partitions); tests/test_cascaded_streamgen_cpu.py has the oracle decode every
one of them to the planner's expected() first.  The expected output is the planner's plain loop; nothing is sampled.

One shuffled batch per element width, with both types of the width in it, streams and outputs at every offset
from a 16-byte boundary that is a multiple of max(size, 4); and one batch of all eight types mixed (the four
launches of a decode, one per width, each leave the other widths' partitions alone), at offsets 0 and 8.  Outputs
lie in guarded slots (tests/decode_guard.py), at three capacities:
  * exact: cap = len(expected) for every chunk;
  * roomy: cap = the largest expected size of the batch, for every chunk;
  * short: cap = len(expected) - one element (0 for an empty output): status and size must be the oracle's.
At the first two every chunk must report status 0 and its size and hold exactly the expected bytes, and the size
pass must report every expected size; at all three no guard byte may change and the input must be unchanged.

The reference build (oracle/_ref) is NOT run on these streams: its decoder does not bound its reads and writes on
forms its own encoder never writes, it cannot decode D > R >= 1, and it loops on a delta layer over 0 elements.
The oracle is the pinned restatement of it, and the CPU test is what ties the planner to the oracle.
"""
import numpy as np
import pytest

import cascaded_streamgen as CS
import decode_guard as G

pytestmark = pytest.mark.gpu


def _batch(sizes, seed):
    """The corpus entries of the given element sizes, shuffled."""
    part = [c for c in CS.corpus() if c[0].size in sizes]
    return [part[i] for i in np.random.default_rng(seed).permutation(len(part))]


def _decode(hc, torch, cuda, cases, caps, offsets, seed):
    n = len(cases)
    streams = [s for _, s, _ in cases]
    inp = G.GuardedSlots(torch, [len(s) for s in streams], cuda, offsets=offsets, turn=1, seed=seed + 1, chunks=streams)
    out = G.GuardedSlots(torch, caps, cuda, offsets=offsets, seed=seed + 2)
    actual = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=cuda)
    assert hc.batch.Codec("Cascaded").decompress_async(inp.batch(hc), out.caps_t, actual, None, out.batch(hc), statuses) == 0
    torch.cuda.synchronize()
    assert inp.unchanged() is None, f"the compressed input was written: {inp.unchanged()}"
    got = out.after()
    bad = out.first_guard_change(got)
    return inp, out, got, bad, statuses.cpu().tolist(), actual.cpu().tolist()


def _report(what, wrong, cases):
    """Fails with the family and the plan's name of the first few wrong streams, and how many of how many."""
    fams = sorted({w.split("/")[0] for w in wrong})
    assert not wrong, f"{what}: {len(wrong)} of {len(cases)} streams wrong, in families {fams}, first {wrong[:8]}"


def _check(hc, oracle, torch, cuda, sizes, offsets, seed):
    cases = _batch(sizes, seed)
    exact = [len(e) for _, _, e in cases]
    print(f"sizes {sizes}: {len(cases)} streams, {sum(exact)} output bytes, largest {max(exact)}")
    for what, caps in (("cap = len(expected)", exact), ("cap = max", [max(exact)] * len(cases))):
        inp, out, got, bad, st, ac = _decode(hc, torch, cuda, cases, caps, offsets, seed)
        assert bad is None, f"{what}: {bad}"
        _report(what, [f"{p.name} (status {st[i]}, size {ac[i]} of {len(e)})" for i, (p, s, e) in enumerate(cases)
                       if st[i] != 0 or ac[i] != len(e) or out.slot_bytes(got, i, len(e)) != e], cases)
    sizes_got = hc.batch.Codec("Cascaded").get_decompress_size(inp.batch(hc)).cpu().tolist()
    _report("size pass", [p.name for i, (p, _, _) in enumerate(cases) if sizes_got[i] != exact[i]], cases)

    short = [max(len(e) - p.size, 0) for p, _, e in cases]
    want = [oracle.cascaded_decompress(s, c) for (_, s, _), c in zip(cases, short)]
    _, out, got, bad, st, ac = _decode(hc, torch, cuda, cases, short, offsets, seed + 5)
    assert bad is None, f"cap = one element short: {bad}"
    _report("cap = one element short",
            [f"{cases[i][0].name} ({st[i]}, {ac[i]}) != oracle ({w[0]}, {len(w[1])})" for i, w in enumerate(want)
             if (st[i], ac[i]) != (w[0], len(w[1])) or (w[0] == 0 and out.slot_bytes(got, i, len(w[1])) != w[1])], cases)
    return len(cases)


@pytest.mark.parametrize("size", [1, 2, 4, 8])
def test_every_planned_stream_of_a_width_decodes_to_the_plain_reference(hc, oracle, cuda, size):
    import torch
    n = _check(hc, oracle, torch, cuda, (size,), tuple(range(0, 16, max(size, 4))), 40 + size)
    assert n == sum(1 for p, _, _ in CS.corpus() if p.size == size)
    assert {p.type for p, _, _ in _batch((size,), 40 + size)} == {t for t in range(8) if CS.SIZE[t] == size}


def test_every_planned_stream_decodes_in_a_batch_of_all_types(hc, oracle, cuda):
    import torch
    n = _check(hc, oracle, torch, cuda, (1, 2, 4, 8), (0, 8), 50)
    assert n == len(CS.corpus()) == sum(len(CS.family(f)) for f in CS.FAMILIES)
