"""Damaged and illegal Deflate streams on the GPU: the decoder returns a status for every one of them and stays
inside the chunk's two ranges.  zlib on the CPU decides every case: where `zlib.decompressobj(-15)` reaches `eof`
with an output that fits the capacity, the GPU reports success with zlib's bytes and size; everywhere else
hipcompErrorCannotDecompress and size 0.  In all cases no guard byte changes, around the outputs and around the
inputs (tests/decode_guard.py).  Damaged streams are an input class like any other here."""
import zlib

import numpy as np
import pytest

import deflate_streamgen as G
from test_deflate_gpu import CANNOT, OK, deflate, run

pytestmark = pytest.mark.gpu

DAMAGES_PER_KIND = 2000


def zlib_says(stream: bytes, cap: int):
    ok, out = G.zlib_verdict(stream)
    return (True, out) if ok and len(out) <= cap else (False, b"")


def check(hc, torch, dev, streams, caps, offsets=(0,)):
    expect = [zlib_says(s, c) for s, c in zip(streams, caps)]
    dst, got, actual, statuses, sizes = run(hc, torch, dev, streams, caps, in_offsets=offsets, out_offsets=offsets)
    for i, (ok, out) in enumerate(expect):
        what = (i, streams[i][:24].hex(), len(streams[i]), caps[i])
        if ok:
            assert statuses[i] == OK and actual[i] == len(out), (what, statuses[i], actual[i], len(out))
            assert dst.slot_bytes(got, i, len(out)) == out, what
            assert sizes[i] == len(out), what
        else:
            assert statuses[i] == CANNOT and actual[i] == 0, (what, statuses[i], actual[i])
            unbounded = G.zlib_verdict(streams[i])
            assert sizes[i] == (len(unbounded[1]) if unbounded[0] else 0), what
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    return sum(ok for ok, _ in expect)


def test_every_illegal_planned_stream(hc, cuda):
    import torch
    plans = G.illegal_plans()
    streams = [s for _, s in plans]
    for caps in ([300] * len(plans), [0] * len(plans), [70000 + 13 * i for i in range(len(plans))]):
        assert check(hc, torch, cuda, streams, caps, offsets=tuple(range(16))) == 0


def kinds_of_stream():
    """one good stream per kind of block structure"""
    text = G._text(2500, 31)
    rnd = np.random.default_rng(3)
    noise = rnd.integers(0, 256, 1500, dtype=np.uint8).tobytes()
    runs = bytes(np.repeat(rnd.integers(0, 256, 300, dtype=np.uint8), rnd.integers(1, 20, 300)))
    plans = {n: s for n, s, _ in G.legal_plans()}
    return {
        "stored": deflate(noise, 0),
        "fixed": deflate(text, 6, zlib.Z_FIXED),
        "dynamic": deflate(text + text[::-1], 9),
        "huffman_only": deflate(text, 6, zlib.Z_HUFFMAN_ONLY),
        "rle_with_flushes": deflate(runs, 6, zlib.Z_RLE, zlib.Z_SYNC_FLUSH),
        "mixed_blocks": plans["match_across_blocks"],
        "planned_200_blocks": plans["blocks_200"],
        "planned_max_alphabets": plans["max_alphabets_15_bit_codes"],
    }


def damage(rng, good: bytes, other: bytes, kind: int) -> bytes:
    b = bytearray(good)
    if kind == 0:      # byte flips
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif kind == 1:    # a bit flip (early bits, where the headers are, more often)
        at = int(rng.integers(0, min(len(b), 40))) if rng.integers(0, 2) else int(rng.integers(0, len(b)))
        b[at] ^= 1 << int(rng.integers(0, 8))
    elif kind == 2:    # truncation
        b = b[: int(rng.integers(0, len(b)))]
    elif kind == 3:    # a splice of two streams
        b = b[: int(rng.integers(0, len(b)))] + bytearray(other[int(rng.integers(0, len(other))):])
    else:              # a zeroed span
        at = int(rng.integers(0, len(b)))
        n = int(rng.integers(1, 64))
        b[at:at + n] = bytes(len(b[at:at + n]))
    return bytes(b)


@pytest.mark.parametrize("kind", list(kinds_of_stream()))
def test_random_damage(hc, cuda, kind):
    import torch
    goods = kinds_of_stream()
    good = goods[kind]
    names = list(goods)
    rng = np.random.default_rng(1000 + names.index(kind))
    true = len(zlib.decompress(good, -15))
    streams, caps = [good], [true]
    for k in range(DAMAGES_PER_KIND):
        other = goods[names[int(rng.integers(0, len(names)))]]
        streams.append(damage(rng, good, other, k % 5))
        caps.append(int(rng.choice([true, true, true + 100, max(true - 1, 0), 4 * true + 1000, 64, 0])))
    accepted = check(hc, torch, cuda, streams, caps, offsets=(0, 1, 2, 3, 5, 8, 13))
    assert accepted >= 1   # (the good stream; damage that zlib accepts is held to zlib's bytes)
