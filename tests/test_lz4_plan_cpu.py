"""The LZ4 launch plan (hipcomp-core_amd/csrc/lz4_plan.cpp) on the CPU.  A wrong geometry still gives the right
bytes, only slower, so the parity suites cannot see one: this pins the plan itself.  The planner is compiled with
tests/lz4_plan_driver.cpp alone (standard headers, no HIP), which prints it.

* lz4_plan_table.json: every launch of a grid of calls (element size, max chunk, batch, temp buffer size and
  address, CU count, forced shape, placement), as the launch code computed them before the planner existed.
  A change of a threshold shows here as the rows it moves.
* The geometries DESIGN.md §3.4 states, by name.
* The temp layout's invariants, and the knobs build of the planner."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
CXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC]

DENSE, SPARSE, WIDE = 1, 2, 3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lz4_plan") / "lz4_plan_driver")
    r = subprocess.run(CXX + ["-O1", os.path.join(TESTS, "lz4_plan_driver.cpp"), os.path.join(CSRC, "lz4_plan.cpp"),
                              "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_plan_reproduces_the_pinned_table(driver):
    table = json.load(open(os.path.join(TESTS, "lz4_plan_table.json")))
    records = table["records"]
    lines = _run(driver, "table").splitlines()
    calls = [line for line in lines if "|" in line]
    assert len(calls) == len(table["calls"])
    moved = []
    for line, want in zip(calls, table["calls"]):
        key, got = line.split("|", 1)
        want = ";".join(records[int(i)] for i in want.split())
        if got.rstrip(";") != want:
            moved.append(f"{key}\n  was {want}\n  now {got}")
    assert not moved, f"{len(moved)} of {len(calls)} calls launch otherwise, e.g.\n" + "\n".join(moved[:5])
    used = [line for line in lines if line.startswith("U ")]
    assert [int(x) for x in used[0].split()[1:]] == table["temp_bytes_used"]


def _plan(driver, ht, batch, elem_size, max_chunk, cus=256, mode=0, temp=None):
    """{"routed": ..., "lds": {...}, 1: {...far class...}, ...} of one compress call (temp: the contract size)"""
    temp = ht * 2 * batch if temp is None else temp
    out = {}
    for line in _run(driver, "plan", ht, batch, elem_size, max_chunk, mode, cus, 0, temp).splitlines():
        words = line.split()
        if words[0].startswith("far"):
            out[int(words[0][3:])] = {k: int(v) for k, v in zip(words[1::2], words[2::2])}
        elif words[0] == "lds":
            out["lds"] = {k: int(v) for k, v in zip(words[1::2], words[2::2])}
        else:
            out.update({k: int(v) for k, v in zip(words[0::2], words[1::2])})
    return out


def _split(far):
    return far["per_cu"], far["near"], far["far"]


@pytest.mark.parametrize("cus", [256, 80])
def test_far_splits_of_design_md(driver, cus):
    """64 KiB chunks 4 x (1 + 7), sparse 2 x (2 + 5); 8 KiB chunks 8 x (1 + 3); chunks of 2 KiB and
    less 8 x (4 + 0) -- workgroups per CU x (LDS-table + device-table waves), batches far beyond the chip."""
    p = _plan(driver, 16384, 100000, 1, 65536, cus)
    assert p["routed"] == 1
    assert _split(p[DENSE]) == (4, 1, 7) and _split(p[WIDE]) == (4, 1, 7) and _split(p[SPARSE]) == (2, 2, 5)
    assert p[DENSE]["span"] == 64 and p[SPARSE]["span"] == 40 and p[WIDE]["span"] == 40
    p = _plan(driver, 8192, 100000, 1, 8192, cus)
    assert _split(p[DENSE]) == (8, 1, 3) and _split(p[WIDE]) == (8, 1, 3)
    for ht in (2048, 512):
        p = _plan(driver, ht, 100000, 1, ht, cus)
        assert all(_split(p[c]) == (8, 4, 0) for c in (DENSE, SPARSE, WIDE)), ht


@pytest.mark.parametrize("cus", [256, 80])
def test_pair_thresholds(driver, cus):
    """Pairs for >= 2 x 3 chunks per CU (1536 at 256 CUs) of more than 32 KiB and at most 64 KiB; with the tags in
    the positions (4-byte elements) for >= 4 per CU (1024) of more than 16 KiB."""
    def pair(batch, elem_size, max_chunk):
        return _plan(driver, 16384, batch, elem_size, max_chunk, cus)["lds"]["pair"]
    assert pair(6 * cus, 1, 65536) == 1 and pair(6 * cus, 2, 32769) == 1
    assert pair(6 * cus - 1, 1, 65536) == 0
    assert pair(6 * cus, 1, 32768) == 0 and pair(6 * cus, 1, 65537) == 0
    assert pair(4 * cus, 4, 16385) == 1 and pair(4 * cus - 1, 4, 16385) == 0 and pair(4 * cus, 4, 16384) == 0
    p = _plan(driver, 16384, 6 * cus, 1, 65536, cus)["lds"]
    assert (p["pair_tags"], p["waves"], p["grid"]) == (1, 2, 3 * cus)     # a tag table: 3 pairs per CU
    p = _plan(driver, 16384, 4 * cus, 4, 65536, cus)["lds"]
    assert (p["pair_tags"], p["inpos"], p["grid"]) == (2, 1, 4 * cus)     # tags in the positions: 4


@pytest.mark.parametrize("cus", [256, 80])
def test_small_batches_of_64k_chunks_get_lds_table_waves_only(driver, cus):
    """batches of at most 4 chunks per CU, one LDS-table wave per chunk."""
    p = _plan(driver, 16384, 4 * cus, 1, 65536, cus)
    for c in (DENSE, SPARSE, WIDE):
        assert (p[c]["near"], p[c]["far"], p[c]["groups"], p[c]["slots"]) == (1, 0, 4 * cus, 2048)
    p = _plan(driver, 16384, 4 * cus + 1, 1, 65536, cus)
    assert all(p[c]["far"] > 0 for c in (DENSE, SPARSE, WIDE))


def test_temp_layout_holds_every_part_wherever_the_buffer_lies(driver):
    """A buffer of lz4_compress_temp_bytes_used(ht, batch) bytes at any address modulo 16 holds the header, the
    class lists, the retry list and min(batch, 8192) tables, aligned, apart, and inside the buffer."""
    assert _run(driver, "layout") == ""


def test_planner_compiles_in_the_knobs_build(tmp_path):
    r = subprocess.run(CXX + ["-DHC_MEASUREMENT_KNOBS", "-c", os.path.join(CSRC, "lz4_plan.cpp"),
                              "-o", str(tmp_path / "lz4_plan.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
