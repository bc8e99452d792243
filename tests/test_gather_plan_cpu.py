"""The arithmetic of a read of many ranges (hipcomp-core_amd/csrc/gather_plan.hpp: decompress_ranges of the
high-level managers) on the CPU.  The header is compiled with tests/gather_plan_driver.cpp alone (g++, standard
headers, no HIP), which prints it for a table of cases; here it is compared with a restatement that walks every
range byte by byte and every rank one by one.  The same driver is built once more as a program of its own with
-fsanitize=address,undefined and run over the same cases."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
M64 = (1 << 64) - 1
LIST_BYTES, FIXED_BYTES, RANK_GROUP = 52, 224, 1024


def _build(directory, name, *flags):
    exe = str(directory / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", *flags, "-I", CSRC,
                        os.path.join(TESTS, "gather_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe, r = _build(tmp_path_factory.mktemp("gather_plan"), "gather_plan_driver")
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, cases):
    """cases: (word, numbers ...) -> per case the printed lines as lists of words"""
    text = "".join(c[0] + " " + " ".join(str(v & M64) for v in c[1:]) + "\n" for c in cases)
    r = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = [], []
    for line in r.stdout.splitlines():
        if line == "end":
            out.append(cur)
            cur = []
        else:
            cur.append(line.split())
    assert len(out) == len(cases)
    return out


def _fields(words, start=0):
    return {k: int(v) for k, v in zip(words[start::2], words[start + 1::2])}


# ---- the restatement ----
def restated_range(d, c, first, num, elem):
    """None (refused), [] (empty) or the pieces, found byte by byte"""
    if first + num > d or first % elem or num % elem:
        return None
    by_chunk = {}
    for b in range(first, first + num):
        by_chunk.setdefault(b // c, []).append(b)
    return [dict(chunk=k, src=bs[0] - k * c, bytes=len(bs), dst=bs[0] - first, cap=min(c, d - k * c)) for k, bs in sorted(by_chunk.items())]


def compare_ranges(driver, cases):
    for case, lines in zip(cases, ask(driver, [("range",) + c for c in cases])):
        want = restated_range(*case)
        if want is None:
            assert lines == [["refused"]], case
        elif not want:
            assert lines == [["range", "empty"]], case
        else:
            head = _fields(lines[0], 1)
            assert (head["c0"], head["c1"]) == (want[0]["chunk"], want[-1]["chunk"]), case
            assert [_fields(w, 1) for w in lines[1:]] == want, case
            at = 0
            for p in want:                               # the pieces tile [0, num) exactly once, in order
                assert p["dst"] == at and 0 < p["bytes"] and p["src"] + p["bytes"] <= p["cap"]
                at += p["bytes"]
            assert at == case[3]


def restated_tables(ranges, chunks):
    r16 = lambda x: (x + 15) // 16 * 16
    w = (chunks + 31) // 32
    return r16(8 * (ranges + 1)) + r16(4 * ranges) + 2 * r16(4 * w) + r16(4 * ((w + RANK_GROUP - 1) // RANK_GROUP))


# ---- the tests ----
def test_every_range_of_a_five_chunk_buffer(driver):
    d, c = 4 * 7 + 5, 7                                  # five chunks of 7, the last one short
    cases = [(d, c, f, n, 1) for f in range(d + 2) for n in range(d + 3 - f)]
    assert len(cases) > 600
    compare_ranges(driver, cases)
    got = ask(driver, [("range",) + k for k in cases])
    assert sum(g == [["refused"]] for g in got) == sum(f + n > d for (_, _, f, n, _) in cases) > 0
    # a range that ends exactly at decomp_bytes, in the short last chunk and across it
    assert ask(driver, [("range", d, c, d - 1, 1, 1), ("range", d, c, d - 6, 6, 1)]) == [
        [["range", "c0", "4", "c1", "4"], "piece chunk 4 src 4 bytes 1 dst 0 cap 5".split()],
        [["range", "c0", "3", "c1", "4"], "piece chunk 3 src 6 bytes 1 dst 0 cap 7".split(), "piece chunk 4 src 0 bytes 5 dst 1 cap 5".split()]]


def test_refusals_whole_elements_and_wrapping(driver):
    d, c = 100, 8
    refused = [(d, c, d + 1, 0, 1), (d, c, 0, d + 1, 1), (d, c, 99, 2, 1),
               (d, c, 1, M64, 1),                        # first + num wraps to 0
               (d, c, 50, M64 - 49 + 10, 1),             # ... wraps to 10
               (d, c, M64, 2, 1), (0, c, 0, 1, 1),
               (d, c, 1, 4, 4), (d, c, 4, 6, 4), (d, c, 2, 2, 4), (d, c, 3, 2, 2)]
    assert ask(driver, [("range",) + k for k in refused]) == [[["refused"]]] * len(refused)
    compare_ranges(driver, refused)
    fine = [(d, c, 0, 0, 1), (d, c, d, 0, 1), (0, c, 0, 0, 1), (d, c, 96, 4, 4), (d, c, 4, 8, 4), (d, c, 98, 2, 2), (d, c, 0, d, 4)]
    assert all(g != [["refused"]] for g in ask(driver, [("range",) + k for k in fine]))
    compare_ranges(driver, fine)
    for elem in (2, 4, 8):
        compare_ranges(driver, [(96, 16, f, n, elem) for f in range(0, 40) for n in (0, 1, 2, 4, 8, 17, 24, 96 - f)])


def test_sizes_up_to_two_to_the_63(driver):
    big = 1 << 63
    got = ask(driver, [("range", big, 65536, 0, big, 1), ("range", big, 65536, big - 70000, 70000, 1),
                       ("range", big - 1, (1 << 62) + 5, 3, big - 5, 1), ("range", big, 1, big - 3, 3, 1),
                       ("range", big, 65536, big, 1, 1), ("range", big, 65536, 1, big, 1)])
    assert _fields(got[0][0], 1) == {"c0": 0, "c1": big // 65536 - 1} and len(got[0]) == 17
    assert all(_fields(w, 1)["bytes"] == 65536 and _fields(w, 1)["src"] == 0 for w in got[0][1:])
    assert _fields(got[0][-1], 1)["dst"] == big - 65536
    assert [_fields(w, 1) for w in got[1][1:]] == [
        dict(chunk=big // 65536 - 2, src=65536 - 4464, bytes=4464, dst=0, cap=65536),
        dict(chunk=big // 65536 - 1, src=0, bytes=65536, dst=4464, cap=65536)]
    assert [_fields(w, 1)["bytes"] for w in got[2][1:]] == [(1 << 62) + 2, big - 5 - (1 << 62) - 2]
    assert [_fields(w, 1)["chunk"] for w in got[3][1:]] == [big - 3, big - 2, big - 1]
    assert got[4] == [["refused"]] and got[5] == [["refused"]]
    # ranks and rooms of that size
    (head, *rows), = ask(driver, [("rank", big - 10, 5, 30, 1 << 40, (big - 10) >> 40)])
    assert _fields(head, 1) == {"lo": 5, "hi": 5 + 10}
    assert _fields(rows[-1]) == {"chunk": 14, "rank": big - 1, "pass": (big - 1) >> 40, "slot": (big - 1) & ((1 << 40) - 1)}
    (room,), = ask(driver, [("room", big, 65536, 1 << 30, 1 << 32, big)])
    t = restated_tables(1 << 30, 1 << 32)
    assert _fields(room, 1) == {"tables": t, "slots": (big - FIXED_BYTES - t) // (65536 + LIST_BYTES),
                                "back": FIXED_BYTES + t + (big - FIXED_BYTES - t) // (65536 + LIST_BYTES) * (65536 + LIST_BYTES)}


def test_pass_and_slot_of_every_rank(driver):
    cases = []
    for S in (1, 2, 3, 5, 8):
        for rank0 in (0, 1, 4, 7, 9):
            for span in (1, 2, 3, 6, 11):
                for p in range(0, 5):
                    cases.append(("rank", rank0, 100, 100 + span - 1, S, p))
    for case, lines in zip(cases, ask(driver, cases)):
        _, rank0, c0, c1, S, p = case
        want = [dict(chunk=c, rank=rank0 + c - c0, **{"pass": (rank0 + c - c0) // S, "slot": (rank0 + c - c0) % S})
                for c in range(c0, c1 + 1) if (rank0 + c - c0) // S == p]
        head = _fields(lines[0], 1)
        assert [_fields(w) for w in lines[1:]] == want, case
        if want:
            assert (head["lo"], head["hi"]) == (want[0]["chunk"], want[-1]["chunk"] + 1), case
            assert len({w["slot"] for w in want}) == len(want)           # no slot twice in a pass
        else:
            assert head["lo"] >= head["hi"], case
    for touched in (1, 2, 5, 6, 7, 64):
        for S in (1, 2, 3, 6, 7, 100):
            (head, *counts), = ask(driver, [("pass", touched, S)])
            ranks = list(range(touched))
            want = [sum(1 for r in ranks if r // S == p) for p in range((touched + S - 1) // S)]
            assert int(head[2]) == len(want) and [int(w[1]) for w in counts] == want, (touched, S)


def test_slots_from_a_room(driver):
    cases = [("room", room, stride, ranges, chunks, cap)
             for stride in (16, 512, 65536) for ranges in (1, 7, 5000) for chunks in (1, 10, 33, 100000)
             for cap in (2, 262144)
             for room in (0, 100, FIXED_BYTES, FIXED_BYTES + restated_tables(ranges, chunks) - 1,
                          FIXED_BYTES + restated_tables(ranges, chunks) + 2 * (stride + LIST_BYTES) - 1,
                          FIXED_BYTES + restated_tables(ranges, chunks) + 2 * (stride + LIST_BYTES), 1 << 20, 1 << 30)]
    for case, ((line,),) in zip(cases, zip(ask(driver, cases))):
        _, room, stride, ranges, chunks, cap = case
        t = restated_tables(ranges, chunks)
        s = 0
        while s < cap and FIXED_BYTES + t + (s + 1) * (stride + LIST_BYTES) <= room:   # one slot at a time
            s += 1
            if s > 70000:
                s = min(cap, (room - FIXED_BYTES - t) // (stride + LIST_BYTES))
                break
        got = _fields(line, 1)
        assert got["tables"] == t and got["slots"] == s, case
        assert got["back"] == FIXED_BYTES + t + s * (stride + LIST_BYTES) and (s == 0 or got["back"] <= room), case


def test_saturating_sum_and_bits(driver):
    cases = [("sat", a, b) for a in (0, 1, 5, M64 - 1, M64, 1 << 63) for b in (0, 1, 4, M64 - 5, M64, 1 << 63)]
    for (_, a, b), ((w,),) in zip(cases, zip(ask(driver, cases))):
        assert int(w[1]) == min(a + b, M64) and int(w[3]) == int(a > b or a == M64), (a, b)
    cases = [("bits", word, bit) for word in (0, 1, 0x80000000, 0xFFFFFFFF, 0xA5A5A5A5, 0x00010001) for bit in range(32)]
    for (_, word, bit), ((w,),) in zip(cases, zip(ask(driver, cases))):
        assert int(w[1]) == sum(1 for k in range(bit) if word >> k & 1), (word, bit)


def test_sanitized_driver_runs_clean(tmp_path):
    exe, r = _build(tmp_path, "gather_plan_driver_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert r.returncode == 0, "the sanitizer runtime does not link here:\n" + r.stderr
    big = 1 << 63
    cases = [("range", 33, 7, f, n, 1) for f in range(35) for n in (0, 1, 7, 8, 33 - f if f <= 33 else 3)]
    cases += [("range", big, 65536, big - 70000, 70000, 1), ("range", 100, 8, 1, M64, 1), ("range", big, 1, big - 3, 3, 1),
              ("rank", big - 10, 5, 30, 1 << 40, (big - 10) >> 40), ("rank", 3, 10, 20, 4, 1), ("pass", 64, 7),
              ("room", big, 65536, 1 << 30, 1 << 32, big), ("room", 100, 512, 5, 10, 2), ("sat", M64, M64), ("bits", 0xFFFFFFFF, 31)]
    assert ask(exe, cases)
    compare_ranges(exe, [c[1:] for c in cases if c[0] == "range" and c[1] == 33])
