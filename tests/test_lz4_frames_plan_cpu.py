"""The arithmetic of a read of a batch of LZ4 frames (hipcomp-core_amd/csrc/lz4_frames_plan.hpp: decompress_frames of
the LZ4 manager): the scratch layout, the partition of the items' data blocks into passes, and the rule of the Arrow
length prefix.  tests/lz4_frames_plan_driver.cpp, a program of its own, prints it; it is compiled with g++ under the
address and undefined-behaviour sanitizers, without HIP, and held to the restatement below."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
ITEM, ENTRY = 160, 9 * 8 + 3 * 4 + 4
FRAMES, RAW, EMPTY, REFUSED = range(4)
NONE, ARROW = 0, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lz4_frames_plan") / "lz4_frames_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "lz4_frames_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, *args):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def _words(line):
    return dict(zip(line[0::2], (int(x) for x in line[1::2])))


# ---- the layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items,P", [(1, 2), (1, 1), (3, 7), (300, 2), (65, 262144), (1 << 20, 2)])
def test_layout(driver, items, P):
    lists = items * ITEM + 64 + 64
    want = lists + ENTRY * P
    room = want + 5
    w = _words(_run(driver, "layout", items, P, room, 1 << 18)[0])
    assert w["items_bytes"] == items * ITEM
    assert w["totals_at"] == items * ITEM and w["ticket_at"] == items * ITEM + 64 and w["lists_at"] == lists
    assert w["item_column_at"] == lists + (ENTRY - 4) * P
    assert w["scratch_bytes"] == want
    assert w["min_scratch_bytes"] == lists + 2 * ENTRY
    assert w["pass_entries"] == (min(P, 1 << 18) if P >= 2 else 0), "P entries fit, and no more, in P entries' room + 5"
    assert all(w[k] % 16 == 0 for k in ("totals_at", "ticket_at", "lists_at")), "every part is 16-byte aligned"
    # one byte below the minimum holds no pass; the minimum holds two entries; `most` bounds it
    assert _words(_run(driver, "layout", items, P, lists + 2 * ENTRY - 1, 100)[0])["pass_entries"] == 0
    assert _words(_run(driver, "layout", items, P, lists + 2 * ENTRY, 100)[0])["pass_entries"] == 2
    assert _words(_run(driver, "layout", items, P, lists + 1000 * ENTRY, 100)[0])["pass_entries"] == 100


# ---- the passes --------------------------------------------------------------------------------------------------
def _partition(counts, P):
    """the restatement: number the blocks through the batch, cut the numbering every P"""
    owner = [i for i, c in enumerate(counts) for _ in range(c)]
    passes = []
    for lo in range(0, len(owner), P):
        part, slices = owner[lo:lo + P], []
        for at, i in enumerate(part):
            if slices and slices[-1][0] == i:
                slices[-1][2] += 1
            else:
                slices.append([i, at, 1])
        passes.append((len(part), slices))
    return passes


@pytest.mark.parametrize("name,counts,P", [
    ("no_blocks", [0], 2), ("one_block", [1], 2), ("empty_items_around", [0, 3, 0], 2), ("one_item_three_passes", [5], 2),
    ("300_items_of_one_block", [1] * 300, 2), ("300_items_one_pass", [1] * 300, 512),
    ("the_passes_test", [5, 0, 1, 1, 1, 3], 2), ("exact_multiple", [2, 2], 2), ("mixed", [3, 0, 0, 4, 1, 0, 6], 4)])
def test_passes(driver, name, counts, P):
    lines = _run(driver, "passes", P, *counts)
    want = _partition(counts, P)
    assert _words(lines[0]) == {"total": sum(counts), "passes": len(want)}
    got, k = [], -1
    for ln in lines[1:]:
        w = _words(ln)
        if "item" in w:
            assert w["pass"] == k
            got[-1][1].append([w["item"], w["at"], w["count"]])
        else:
            k += 1
            assert w["pass"] == k
            got.append((w["count"], []))
    assert got == want
    # every block is in exactly one pass, in item order, and no slice leaves its pass
    for count, slices in got:
        assert sum(c for _, _, c in slices) == count <= P
        assert all(at + c <= count for _, at, c in slices)


# ---- the prefix --------------------------------------------------------------------------------------------------
def _prefix(prefix, nbytes, word, capacity):
    """the table of the issue, row by row: (kind, payload_at, expected or -1)"""
    if prefix == NONE:
        return FRAMES, 0, -1
    if nbytes == 0:
        return EMPTY, 0, 0
    if nbytes < 8:
        return REFUSED, 0, -1
    if word == -1:
        return (RAW, 8, nbytes - 8) if nbytes - 8 <= capacity else (REFUSED, 8, -1)
    if word < -1 or word > capacity:
        return REFUSED, 8, -1
    return FRAMES, 8, word


@pytest.mark.parametrize("nbytes", [0, 1, 7, 8, 9, 100])
@pytest.mark.parametrize("word", [-(1 << 63), -2, -1, 0, 1, 50, 51, (1 << 63) - 1])
@pytest.mark.parametrize("prefix", [NONE, ARROW])
def test_prefix(driver, prefix, nbytes, word, capacity=50):
    w = _words(_run(driver, "prefix", prefix, nbytes, word, capacity)[0])
    assert (w["kind"], w["payload_at"], w["expected"]) == _prefix(prefix, nbytes, word, capacity)
    size = 0 if nbytes < 8 else nbytes - 8 if word == -1 else 0 if word < -1 else word
    assert w["size"] == size, "the size query: the prefix and nothing else"


def test_prefix_stored_item_capacity(driver):
    """-1: the bytes behind the prefix are the buffer; they have to fit the capacity like any other"""
    assert _words(_run(driver, "prefix", ARROW, 8 + 50, -1, 50)[0])["kind"] == RAW
    assert _words(_run(driver, "prefix", ARROW, 8 + 51, -1, 50)[0])["kind"] == REFUSED
    assert _words(_run(driver, "prefix", ARROW, 8, -1, 0)[0]) == {"kind": RAW, "payload_at": 8, "expected": 0, "size": 0}
