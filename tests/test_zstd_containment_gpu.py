"""Illegal and damaged Zstandard chunks on the GPU: the decoder returns a status for every one of them and stays
inside the chunk's two ranges and the temp space.  libzstd decided every case beforehand: the illegal planned
frames of tests/zstd_framegen.py are refused (tests/test_zstd_framegen_cpu.py holds them to libzstd on the CPU), the
damaged-frame fixture (tests/zstd_fixtures.py) carries libzstd's verdict and the MD5 of its output.  No guard byte
changes around the outputs, the inputs and the temp space, and a refused chunk's neighbours decode."""
import hashlib
import os

import pytest

import zstd_fixtures as F
import zstd_framegen as G
from test_zstd_gpu import CANNOT, OK, run

pytestmark = pytest.mark.gpu

GOOD = G.frame([("raw", b"a neighbour that must decode"), ("rle", 0x2E, 40)], checksum=True)


def test_every_illegal_planned_frame(hc, cuda):
    import torch
    with open(os.path.join(F.DIR, "huffman_last_symbol.zst"), "rb") as f:
        last_symbol = f.read()
    plans = (G.illegal_plans() + G.documented_differences() + [("overread", G.libzstd_frame_with_overread(F.load()[0])[0]),
                                                                ("huffman_last_symbol", last_symbol)])
    chunks, caps = [], []
    for _, c in plans:          # every refused chunk between two good ones
        chunks += [GOOD[0], c]
        caps += [len(GOOD[1]), 1 << 17]
    chunks.append(GOOD[0])
    caps.append(len(GOOD[1]))
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, chunks, caps)
    for i in range(len(chunks)):
        name = "neighbour" if i % 2 == 0 else plans[i // 2][0]
        if i % 2 == 0:
            assert statuses[i] == OK and actual[i] == len(GOOD[1]), (name, i, statuses[i])
            assert dst.slot_bytes(got, i, actual[i]) == GOOD[1]
        else:
            assert statuses[i] == CANNOT and actual[i] == 0, (name, statuses[i], actual[i])
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)


def test_damaged_frame_fixture(hc, cuda):
    import torch
    damaged = F.load()[1]
    accepted = {}
    for first in range(0, len(damaged), 512):      # batches of at most 512 chunks
        part = damaged[first:first + 512]
        dst, got, actual, statuses, sizes = run(hc, torch, cuda, [c for _, c, _, _, _ in part], [cap for _, _, cap, _, _ in part])
        for i, (kind, chunk, cap, size, md5) in enumerate(part):
            what = (first + i, kind, chunk[:16].hex(), len(chunk))
            if size is None:
                assert statuses[i] == CANNOT and actual[i] == 0, (what, statuses[i], actual[i])
            else:
                accepted[kind] = accepted.get(kind, 0) + 1
                assert statuses[i] == OK and actual[i] == size, (what, statuses[i], actual[i], size)
                assert hashlib.md5(dst.slot_bytes(got, i, size)).hexdigest() == md5, what
        assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    assert set(accepted) == {k for k, _, _, _, _ in damaged}      # every damage kind also takes the accept path
