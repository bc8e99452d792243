"""The plan of a ranged read (hipcomp-core_amd/csrc/range_plan.hpp: decompress_range of the high-level managers) on
the CPU.  The header is compiled with tests/range_plan_driver.cpp alone (g++, standard headers, no HIP), which prints
the plan; here it is compared with a restatement that walks the range byte by byte, and its invariants are asserted
for every case: the spans tile [0, num_bytes) exactly once, no chunk outside [first_byte / chunk, (first_byte +
num_bytes - 1) / chunk] appears, at most two edge chunks where the alignment permits, a pass holds no more chunks
than its lists and no more edge chunks than there are slots."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("range_plan") / "range_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", CSRC, os.path.join(TESTS, "range_plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def plans(driver, cases):
    """cases: (decomp, chunk, first, num, slab, slots, align, out_mod, elem) -> None (refused) or (head, [chunk dicts])"""
    text = "".join(" ".join(str(v & M64) for v in c) + "\n" for c in cases)
    r = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out, cur = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "refused":
            cur = None
        elif w[0] == "plan":
            cur = ({k: int(v) for k, v in zip(w[1::2], w[2::2])}, [])
        elif w[0] == "chunk":
            cur[1].append({k: int(v) for k, v in zip(w[0::2], w[1::2])})
        elif w[0] == "end":
            out.append(cur)
    assert len(out) == len(cases)
    return out


def restated(d, c, first, num, slab, slots, align, mod, elem):
    """the same plan, byte by byte"""
    if first + num > d or first % elem or num % elem:
        return None
    by_chunk = {}
    for b in range(first, first + num):
        by_chunk.setdefault(b // c, []).append(b)
    rows = [dict(chunk=k, src=bs[0] - k * c, dst=bs[0] - first, bytes=len(bs), cap=min(c, d - k * c)) for k, bs in sorted(by_chunk.items())]
    all_edge = any(r["bytes"] == r["cap"] and (mod + r["dst"]) % align for r in rows)
    per_pass = min(slab, slots) if all_edge else slab
    for r in rows:
        at = r["chunk"] - rows[0]["chunk"]
        r["edge"] = int(all_edge or r["bytes"] != r["cap"])
        r["pass"] = at // per_pass
        r["slot"] = at % per_pass if all_edge else int(at != 0)
    return rows, all_edge, per_pass


def check_invariants(case, got):
    d, c, first, num, slab, slots, align, mod, elem = case
    head, rows = got
    assert head["chunks"] == (0 if num == 0 else (first + num - 1) // c - first // c + 1)
    assert head["passes"] == (head["chunks"] + head["per_pass"] - 1) // head["per_pass"] if head["chunks"] else head["passes"] == 0
    if head["chunks"] <= 64:
        assert len(rows) == head["chunks"]
        at = 0
        for r in rows:                                   # the spans tile [0, num) exactly once, in order
            assert r["dst"] == at and r["bytes"] > 0, (case, r)
            at += r["bytes"]
        assert at == num, case
    seen = {}
    for r in rows:
        assert first // c <= r["chunk"] <= (first + num - 1) // c, (case, r)
        assert r["cap"] == min(c, d - r["chunk"] * c) and r["src"] + r["bytes"] <= r["cap"]
        assert r["chunk"] * c + r["src"] - first == r["dst"]
        assert r["pass"] == (r["chunk"] - head["first_chunk"]) // head["per_pass"]
        if r["edge"]:
            assert r["slot"] < (head["per_pass"] if head["all_edge"] else 2) and r["slot"] < max(slots, 2)
            assert (r["pass"], r["slot"]) not in seen, (case, r)    # no slot twice in a pass
            seen[(r["pass"], r["slot"])] = r["chunk"]
        else:                                            # decoded in place: whole, and where the decoder may write
            assert r["src"] == 0 and r["bytes"] == r["cap"] and (mod + r["dst"]) % align == 0, (case, r)
    assert head["per_pass"] <= slab and (not head["all_edge"] or head["per_pass"] <= max(slots, 2))
    if not head["all_edge"]:
        assert sum(r["edge"] for r in rows) <= 2, case


def compare(driver, cases):
    for case, got in zip(cases, plans(driver, cases)):
        want = restated(*case)
        if want is None:
            assert got is None, case
            continue
        assert got is not None, case
        rows, all_edge, per_pass = want
        head, got_rows = got
        check_invariants(case, got)
        assert head["all_edge"] == int(all_edge), case
        if rows:
            assert head["per_pass"] == per_pass and head["first_chunk"] == rows[0]["chunk"], case
        assert [{k: r[k] for k in ("chunk", "pass", "edge", "slot", "src", "dst", "bytes", "cap")} for r in got_rows] == \
               [{k: r[k] for k in ("chunk", "pass", "edge", "slot", "src", "dst", "bytes", "cap")} for r in rows], case


def test_every_range_of_a_five_chunk_buffer(driver):
    d, c = 4 * 7 + 5, 7                                  # five chunks of 7, the last one short
    cases = [(d, c, f, n, 4, 2, 1, 0, 1) for f in range(d + 2) for n in range(d + 3 - f)]
    assert len(cases) > 600
    compare(driver, cases)
    got = plans(driver, cases)
    assert sum(g is None for g in got) == sum(f + n > d for (_, _, f, n, *_) in cases) > 0


def test_chunk_and_pass_boundaries(driver):
    d, c, slab = 11 * 16 + 3, 16, 4
    cases = []
    for start in (0, 1, 15, 16, 17, 63, 64, 65):
        for end in (16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 176, 177, d - 1, d):
            for delta in (-1, 0, 1):
                if start < end + delta <= d:
                    cases.append((d, c, start, end + delta - start, slab, 2, 1, 0, 1))
    compare(driver, cases)
    # a range of exactly one pass, and one chunk more
    (head, rows), (head2, rows2) = plans(driver, [(d, c, 16, 64, slab, 2, 1, 0, 1), (d, c, 16, 65, slab, 2, 1, 0, 1)])
    assert (head["passes"], head2["passes"]) == (1, 2) and not any(r["edge"] for r in rows)
    assert [r["edge"] for r in rows2] == [0, 0, 0, 0, 1] and rows2[4]["pass"] == 1 and rows2[4]["slot"] == 1


def test_empty_and_refused_ranges(driver):
    d, c = 100, 8
    got = plans(driver, [(d, c, 0, 0, 4, 2, 1, 0, 1), (d, c, 50, 0, 4, 2, 1, 0, 1), (d, c, d, 0, 4, 2, 1, 0, 1),
                         (0, c, 0, 0, 4, 2, 1, 0, 1)])
    for head, rows in got:
        assert head["chunks"] == 0 and head["passes"] == 0 and rows == []
    refused = [(d, c, d + 1, 0, 4, 2, 1, 0, 1), (d, c, 0, d + 1, 4, 2, 1, 0, 1), (d, c, 99, 2, 4, 2, 1, 0, 1),
               (d, c, 1, M64, 4, 2, 1, 0, 1),            # first_byte + num_bytes wraps to 0
               (d, c, 50, M64 - 49 + 10, 4, 2, 1, 0, 1),  # ... wraps to 10
               (d, c, M64, 2, 4, 2, 1, 0, 1), (0, c, 0, 1, 4, 2, 1, 0, 1)]
    assert plans(driver, refused) == [None] * len(refused)


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_alignment_four_with_every_element_size(driver, elem):
    align = max(4, elem)
    cases = []
    for c in sorted({8 * elem, 16, 24} | ({6, 10} if elem <= 2 else set())):   # (chunks of whole elements)
        d = 6 * c + c // 2 // elem * elem
        for f in range(0, 3 * c + 1, elem):
            for n in (elem, c, 2 * c, 3 * c + elem, d - f):
                if n % elem == 0 and f + n <= d:
                    for mod in range(0, align, elem):
                        for slots in (2, 3, 100):
                            cases.append((d, c, f, n, 4, slots, align, mod, elem))
    compare(driver, cases)
    got = plans(driver, cases)
    # (whole elements of 4 or 8 bytes always land aligned; those of 1 or 2 bytes need not)
    assert any(g[0]["all_edge"] for g in got) == (elem < 4)
    assert any(not g[0]["all_edge"] and g[0]["chunks"] > 2 for g in got)
    # first_byte or num_bytes that is not whole elements
    if elem > 1:
        assert plans(driver, [(64, 16, 1, elem, 4, 2, align, 0, elem), (64, 16, 0, elem + 1, 4, 2, align, 0, elem)]) == [None, None]


def test_sizes_up_to_two_to_the_63(driver):
    big = 1 << 63
    cases = [(big, 65536, 0, big, 262144, 2, 1, 0, 1), (big, 65536, big - 70000, 70000, 262144, 2, 1, 0, 1),
             (big - 1, (1 << 62) + 5, 3, big - 5, 262144, 2, 1, 0, 1), (big, 1, big - 3, 3, 2, 2, 4, 1, 1),
             (big, 4096, 4098, big - 4098 - 2, 262144, 1000, 4, 0, 2)]
    got = plans(driver, cases)
    for case, g in zip(cases, got):
        assert g is not None, case
        check_invariants(case, g)
    assert got[0][0]["chunks"] == big // 65536 and got[0][0]["passes"] == big // 65536 // 262144
    assert [r["chunk"] for r in got[1][1]] == [big // 65536 - 2, big // 65536 - 1] and got[1][1][0]["edge"] == 1
    assert got[2][0]["chunks"] == 2 and [r["bytes"] for r in got[2][1]] == [(1 << 62) + 2, big - 5 - (1 << 62) - 2]
    assert got[4][0]["all_edge"] == 1 and got[4][0]["per_pass"] == 1000
    assert plans(driver, [(big, 65536, big, 1, 4, 2, 1, 0, 1), (big, 65536, 1, big, 4, 2, 1, 0, 1)]) == [None, None]
