"""Illegal and damaged Zstandard chunks and dictionaries on the GPU: the decoder with dictionaries returns a status for
every one of them and stays inside the chunk's two ranges, the blobs and the temp space.  libzstd decided every case
beforehand: the damaged-frame and damaged-dictionary fixture (tests/zstd_dict_fixtures.py) carries its verdict and the MD5
of its output, the illegal plans of tests/zstd_dictgen.py are refused (tests/test_zstd_dict_cpu.py holds both to libzstd
on the CPU).  No guard byte changes around the outputs, the inputs, the blobs and the temp space, and a refused chunk's
neighbours decode."""
import hashlib

import pytest

import zstd_dict_fixtures as F
import zstd_dictgen as D
from test_zstd_dict_gpu import CANNOT, OK, Prepared, run

pytestmark = pytest.mark.gpu


def test_damaged_frames_and_damaged_dictionaries(hc, cuda):
    import torch
    dicts, frames, damaged = F.load()
    loads = dict((d, ok) for _, _, _, d, _, _, ok in damaged)
    used = sorted(loads)
    assert len(used) >= 60 and True in loads.values() and False in loads.values()     # the damaged copies of dictionary "a", and "a" itself
    prepared = Prepared(hc, torch, cuda, used, [loads[d] for d in used])
    assert [s == OK for s in prepared.statuses] == [loads[d] for d in used]
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, [x[1] for x in damaged], [x[2] for x in damaged], [prepared.ptr(x[3]) for x in damaged])
    accepted = {}
    for i, (kind, chunk, cap, d, size, md5, _) in enumerate(damaged):
        what = (i, kind, chunk[:16].hex(), len(chunk))
        if size is None:
            assert statuses[i] == CANNOT and actual[i] == 0, (what, statuses[i], actual[i])
        else:
            accepted[kind] = accepted.get(kind, 0) + 1
            assert statuses[i] == OK and actual[i] == size, (what, statuses[i], actual[i], size)
            assert hashlib.md5(dst.slot_bytes(got, i, size)).hexdigest() == md5, what
            dst.region[i] = size
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
    assert set(accepted) == {x[0] for x in damaged}      # every damage kind also takes the accept path


def test_every_illegal_plan_between_good_neighbours(hc, cuda):
    import torch
    plans = [(n, c, d) for n, c, d, w in D.planned_frames() if w is None]
    good = next((c, d, w) for n, c, d, w in D.planned_frames() if n == "match_crosses_and_overruns_itself_formatted")
    named = D.planned_dictionaries()
    prepared = Prepared(hc, torch, cuda, [d for _, d, _ in named], [ok for _, _, ok in named])
    chunks, caps, blobs = [], [], []
    for _, c, d in plans:          # every refused chunk between two good ones
        chunks += [good[0], c]
        caps += [len(good[2]), 1 << 12]
        blobs += [prepared.ptr(good[1]), prepared.ptr(d)]
    chunks.append(good[0])
    caps.append(len(good[2]))
    blobs.append(prepared.ptr(good[1]))
    assert len(plans) >= 15
    dst, got, actual, statuses, sizes = run(hc, torch, cuda, chunks, caps, blobs)
    for i in range(len(chunks)):
        if i % 2 == 0:
            assert statuses[i] == OK and actual[i] == len(good[2]), ("neighbour", i, statuses[i])
            assert dst.slot_bytes(got, i, actual[i]) == good[2]
        else:
            assert statuses[i] == CANNOT and actual[i] == 0, (plans[i // 2][0], statuses[i], actual[i])
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)
