"""The batched decoders stay inside each chunk's capacity, on good and on damaged input.

The C API promises that chunk i writes only inside out_ptrs[i][0, out_caps[i]).  Every chunk here has a capacity of
its own, taken from its true (or, for a damaged stream, its declared) size: exact, -1, +1, -one element, +15, +16,
1, 0 and much larger; good and damaged streams are interleaved in one batch.  The outputs lie in guarded slots
(tests/decode_guard.py) at varying offsets from 16-byte boundaries, the compressed input in a guarded arena of its
own, and afterwards every guard byte must still hold its pseudo-random pattern, the input must be unchanged, and
status, reported size and (on success) the bytes must be the oracle's for that capacity.

Two batch sizes: a few thousand streams with sources up to 8 KiB (Cascaded: all eight types, so that the 4-byte
decoder and the generic one both run, under raw, RLE, delta, bit-pack, (2,1,1) and (3,2,1)), and a batch of
4 x 32 x CU-count small streams, where the LZ4 decoder draws chunks from its ticket counter and every Cascaded wave
decodes many partitions one after another -- a wave that has just given up on a damaged chunk goes on to a good one.
"""
import functools

import numpy as np
import pytest

import datagen
import decode_guard as G

pytestmark = pytest.mark.gpu

ANY_BYTE = (0, 1, 3, 5, 7, 9, 13, 15, 4, 8, 2, 11)


def _offsets(es):
    """Output offsets the C API allows: any byte for LZ4 and Snappy, element (and 4-byte) alignment for Cascaded."""
    step = max(es, 4) if es else 1
    return ANY_BYTE if es == 0 else tuple(range(0, 16, step))


class Spec:
    """One codec's oracle and size rules."""

    def __init__(self, oracle, name):
        self.name = name
        self.o = oracle
        self.dec = {"LZ4": oracle.lz4_decompress, "Snappy": oracle.snappy_decompress,
                    "Cascaded": oracle.cascaded_decompress}[name]

    @functools.lru_cache(maxsize=None)
    def want(self, s, cap):
        return self.dec(s, cap)

    def declared(self, s):
        """The size the stream itself declares (what the size query reports)."""
        if self.name == "LZ4":
            st, n = self.o.lz4_decompressed_size(s)
            return n if st == 0 else 0
        if self.name == "Snappy":
            return self.o.snappy_uncompressed_size(s)
        return self.o.cascaded_decompressed_size(s)

    def region(self, s, cap):
        """The bytes chunk s may write with capacity cap.  Snappy: capacity 0 means the size the stream declares
        (snappy_kernels.hip, reference decompression.hiph:148-149) -- the oracle does the same."""
        return self.declared(s) if self.name == "Snappy" and cap == 0 else cap


def _elem(spec, s):
    """The element size of the capacities' "-one element" (Cascaded: the stream's type; LZ4: the INT mode's)."""
    if spec.name == "Cascaded":
        return G.CASCADED_SIZE.get(s[3], 1) if len(s) > 3 else 1
    return 4 if spec.name == "LZ4" else 1


def _caps(spec, streams, truth):
    """Mixed capacities: chunk k gets capacity kind k % 9 of its true size -- or, for every other damaged stream,
    of the size the stream declares (a stream that declares one element less, decoded at exactly that capacity,
    is where one element too many shows)."""
    caps = []
    for k, (s, true_size) in enumerate(zip(streams, truth)):
        base = true_size
        if (k // 9) % 2:
            d = spec.declared(s)
            if d <= 2 * true_size + 4096:
                base = d
        cap = G.capacity_kinds(base, _elem(spec, s))[k % 9]
        # (Snappy, capacity 0: the slot is the declared size -- kept to streams that declare a sane one)
        if spec.name == "Snappy" and cap == 0 and spec.declared(s) > 2 * true_size + 4096:
            cap = true_size
        caps.append(cap)
    return caps


def _decode_and_check(hc, torch, cuda, spec, streams, caps, out_offsets, with_status=True, temp=None, seed=0):
    n = len(streams)
    inp = G.GuardedSlots(torch, [len(s) for s in streams], cuda, offsets=ANY_BYTE if spec.name != "Cascaded"
                         else out_offsets, turn=3, seed=seed + 1, chunks=streams)
    region = [spec.region(s, c) for s, c in zip(streams, caps)]
    out = G.GuardedSlots(torch, caps, cuda, offsets=out_offsets, seed=seed + 2, region=region)
    actual = torch.full((n,), -1, dtype=torch.int64, device=cuda) if with_status else None
    statuses = torch.full((n,), -1, dtype=torch.int32, device=cuda) if with_status else None
    codec = hc.batch.Codec(spec.name)
    assert codec.decompress_async(inp.batch(hc), out.caps_t, actual, temp, out.batch(hc), statuses) == 0
    torch.cuda.synchronize()
    what = f"{spec.name}, {n} streams"
    assert inp.unchanged() is None, f"{what}: the compressed input was written: {inp.unchanged()}"
    got = out.after()
    bad = out.first_guard_change(got)
    assert bad is None, f"{what}: {bad}"
    st = statuses.cpu().tolist() if with_status else None
    ac = actual.cpu().tolist() if with_status else None
    for i, s in enumerate(streams):
        ost, obytes = spec.want(s, caps[i])
        if with_status:
            assert (st[i], ac[i]) == (ost, len(obytes)), f"{what}: chunk {i}, capacity {caps[i]}: status/size"
        if ost == 0:
            assert out.slot_bytes(got, i, len(obytes)) == obytes, f"{what}: chunk {i}, capacity {caps[i]}: bytes"
    return inp


def _interleave(goods, bads, n, rng):
    """n corpus entries, good and damaged in turn."""
    out = []
    for k in range(n):
        pool = goods if k % 2 == 0 else bads
        out.append(pool[int(rng.integers(0, len(pool)))])
    return out


# ---------------------------------------------------------------------------------------------- sources

def _byte_sources(seed, big):
    """datagen sources, 8 KiB at most (big) or about 1 KiB at most."""
    if big:
        return [datagen.text_like(seed, 6000), datagen.harness_like_int32(seed + 1, 2000).tobytes(),
                datagen.sparse_repeats(seed + 2, 8000, 90, 7), datagen.random_runs_int32(seed + 3, 1500).tobytes(),
                datagen.tpch_lineitem_text(seed + 4, 5000), datagen.periodic_bytes(seed + 5, 4000, 3, 40),
                bytes(np.random.default_rng(seed).integers(0, 256, 3000, dtype=np.uint8)), b"x"]
    return [datagen.text_like(seed, 900), datagen.harness_like_int32(seed + 1, 200).tobytes(),
            datagen.vocabulary_text(seed + 2, 1000, 16, 8), datagen.random_runs_int32(seed + 3, 250).tobytes(),
            datagen.small_alphabet_bytes(seed + 4, 700, 3), datagen.periodic_bytes(seed + 5, 1024, 3, 40),
            bytes(np.random.default_rng(seed).integers(0, 256, 333, dtype=np.uint8)), b"ab"]


def _corpus(oracle, name, big, seed):
    """[(stream, true size, good?)]"""
    rng = np.random.default_rng(seed)
    out = []
    if name == "Cascaded":
        if big:
            return [(s, len(src), good) for s, src, t, good in G.cascaded_corpus(oracle, seed)]
        for t in range(8):
            dt = G.CASCADED_NP[t]
            r2 = np.random.default_rng(seed + t)
            srcs = [np.cumsum(r2.integers(0, 3, 1600 // G.CASCADED_SIZE[t])).astype(dt).tobytes(),
                    np.repeat(r2.integers(-9, 9, 300), r2.integers(1, 6, 300))[: 900 // G.CASCADED_SIZE[t]]
                    .astype(dt).tobytes()]
            for k, opts in enumerate(G.CASCADED_OPTS):
                src = srcs[k % 2]
                good = oracle.cascaded_compress(src, t, *opts)[0]
                out.append((good, len(src), True))
                out += [(s, len(src), False) for s in G.damaged("Cascaded", good, rng, 4)]
        return out
    for k, src in enumerate(_byte_sources(seed, big)):
        es = 4 if (name == "LZ4" and k % 2) else 1     # (LZ4: some streams from the INT mode of the encoder)
        good = oracle.lz4_compress(src, es, 65536) if name == "LZ4" else oracle.snappy_compress(src)
        out.append((good, len(src), True))
        out += [(s, len(src), False) for s in G.damaged(name, good, rng, 120 if big else 60)]
    return out


def _batch(oracle, spec, big, seed, n=None):
    corpus = _corpus(oracle, spec.name, big, seed)
    rng = np.random.default_rng(seed + 99)
    goods = [c for c in corpus if c[2]]
    bads = [c for c in corpus if not c[2]]
    if n is None:   # every stream once, good ones spread among the damaged ones
        order = rng.permutation(len(corpus))
        picked = [corpus[i] for i in order]
    else:
        picked = _interleave(goods, bads, n, rng)
    streams = [p[0] for p in picked]
    truth = [p[1] for p in picked]
    return streams, truth


def _sizes_match(hc, spec, inp, streams):
    got = hc.batch.Codec(spec.name).get_decompress_size(inp.batch(hc)).cpu().tolist()
    want = [spec.declared(s) for s in streams]
    assert got == want, f"{spec.name}: size pass differs at chunk {next(i for i in range(len(got)) if got[i] != want[i])}"


# ---------------------------------------------------------------------------------------------- tests

@pytest.mark.parametrize("name", ["LZ4", "Snappy", "Cascaded"])
def test_mixed_capacities_stay_inside_their_slots(hc, oracle, cuda, name):
    """A few thousand good and damaged streams, every chunk its own capacity; then the size pass, and (where the C
    API allows it: LZ4, Snappy) the same decode with null statuses and null actual sizes."""
    import torch
    spec = Spec(oracle, name)
    streams, truth = _batch(oracle, spec, True, 11)
    caps = _caps(spec, streams, truth)
    offs = _offsets(0 if name != "Cascaded" else 4)
    temp = None
    if name == "LZ4":
        temp = torch.empty(hc.batch.Codec("LZ4").decompress_temp_size(len(streams), 65536), dtype=torch.uint8,
                           device=cuda)
    inp = _decode_and_check(hc, torch, cuda, spec, streams, caps, offs, temp=temp, seed=10)
    _sizes_match(hc, spec, inp, streams)
    if name != "Cascaded":   # (Cascaded requires both arrays: hipcompBatchedCascadedDecompressAsync)
        _decode_and_check(hc, torch, cuda, spec, streams, caps, offs, with_status=False, temp=temp, seed=20)


@pytest.mark.parametrize("t", [1, 2, 4, 7])
def test_cascaded_capacities_at_element_alignment(hc, oracle, cuda, t):
    """Cascaded of one type per batch, slots at every element-aligned offset: the 4-byte decoder (t = 4) and the
    generic one (1, 2, 8 bytes), at capacities within one element of the declared size."""
    import torch
    spec = Spec(oracle, "Cascaded")
    rng = np.random.default_rng(500 + t)
    s = G.CASCADED_SIZE[t]
    streams, truth = [], []
    for k, opts in enumerate(G.CASCADED_OPTS):
        for src in G.cascaded_sources(t, 600 + 10 * t + k):
            good = oracle.cascaded_compress(src, t, *opts)[0]
            for d in [good] + G.damaged("Cascaded", good, rng, 2):
                streams.append(d)
                truth.append(len(src))
    caps = []
    for k, d in enumerate(streams):
        base = spec.declared(d) if spec.declared(d) <= 2 * truth[k] + 4096 else truth[k]
        caps.append(max(base + (-s, -1, 0, 0, 1, s)[k % 6], 0))
    offs = tuple(range(0, 16, max(s, 4)))
    _decode_and_check(hc, torch, cuda, spec, streams, caps, offs, seed=30 + t)


class _Span:
    """`size` bytes at a device address, as the Codec calls take a temp buffer (a torch view of 0 bytes has no
    address)."""

    def __init__(self, ptr, size):
        self.ptr, self.size = ptr, size

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.size


def _persistent_n(torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 4 * 32 * cus, cus


@pytest.mark.parametrize("name", ["LZ4", "Snappy", "Cascaded"])
def test_persistent_grid_reuse(hc, oracle, cuda, name):
    """4 x 32 x CU-count small streams, good and damaged in turn, mixed capacities: every wave of the persistent
    decoders takes both kinds one after another.  LZ4 twice: with a temp buffer of exactly
    hipcompBatchedLZ4DecompressGetTempSize bytes at base offsets 0, 1, 4, 13 mod 16 inside a guarded arena (the
    ticket counter runs and must stay inside the buffer), and without one (one chunk per wave: the C API refuses a
    null temp pointer, as the reference does -- LZ4Batch.cpp:112 -- so "none" is a buffer of 0 bytes).  Then the
    size pass of the same batch."""
    import torch
    n, cus = _persistent_n(torch)
    spec = Spec(oracle, name)
    streams, truth = _batch(oracle, spec, False, 40, n)
    assert max(truth) <= 8192
    caps = _caps(spec, streams, truth)
    offs = _offsets(0 if name != "Cascaded" else 4)
    print(f"{name}: {n} streams per batch, {cus} CUs")
    temps = [None]
    if name == "LZ4":
        tbytes = hc.batch.Codec("LZ4").decompress_temp_size(n, 65536)
        temps = [(base, tbytes) for base in (0, 1, 4, 13)] + [(5, 0)]
    for k, temp in enumerate(temps):
        arena = None
        if temp is not None:
            base, tbytes = temp
            arena = G.GuardedSlots(torch, [tbytes], cuda, offsets=(base,), seed=70 + k)
            temp = _Span(arena.data.data_ptr() + int(arena.at[0]), tbytes)
            assert temp.data_ptr() % 16 == base
        inp = _decode_and_check(hc, torch, cuda, spec, streams, caps, offs, temp=temp, seed=50 + 2 * k)
        bad = arena.first_guard_change() if arena is not None else None
        assert bad is None, f"temp buffer of {tbytes} bytes at {base} mod 16: {bad}"
    _sizes_match(hc, spec, inp, streams)
