"""Batches of LZ4 frames in one call (hipcomp/lz4.hpp: decompress_frames and get_frames_decompressed_sizes of the LZ4
manager; INTEGRATION.md, "Batches of LZ4 frames", has the contract), through tests/lz4_frames_driver.cpp, a C++ program
written against include/ and linked to libhipcomp.so.  The driver works through a list of cases per process, each
process under a timeout; it puts guard bytes on both sides of every output and behind a caller-owned scratch buffer.

Equivalence: every fixture of tests/golden/lz4_frame/ and every planned frame of lz4_framegen, legal and hostile, gives
as a one-item batch what configure_frame_decompression + decompress_frame give for the same bytes in the same process,
and what the plan says, under each ChecksumPolicy.  Isolation: in batches of 1, 3, 65 and 300 items with hostile items
first, in the middle and last, and capacities exact, one short and oversize, every item's result is its one-item
result.  Passes: a scratch bounded to two entries per pass gives what the large one gives.  Arrow: the bodies of
tests/golden/arrow_ipc/ decode, buffer for buffer, to the manifest's hashes, and the prefix table holds row by row."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

import arrow_bodygen as A
import lz4_framegen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lz4_frame")
POLICIES = range(5)
NONE, ARROW = 0, 1
ITEM_BYTES, ENTRY_BYTES = 160, 9 * 8 + 3 * 4 + 4   # hipcomp-core_amd/csrc/lz4_frames_plan.hpp


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    assert os.path.exists(os.path.join(LIB, "libhipcomp.so")), "run __graft_entry__.build()"
    exe = str(tmp_path_factory.mktemp("lz4_frames") / "lz4_frames_driver")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "lz4_frames_driver.cpp"), "-L", LIB, "-lhipcomp",
                        "-Wl,-rpath," + LIB, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def _words(stdout):
    return [dict(zip(w[0::2], (int(x) for x in w[1::2]))) for w in (ln.split() for ln in stdout.splitlines())]


def _simple(driver, *args, timeout=120):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return _words(r.stdout)


class Case:
    """items: [(file, offset, length, capacity word)]"""
    def __init__(self, policy, prefix, items, scratch="own", pass_entries=0, sandwich=0):
        self.policy, self.prefix, self.items = policy, prefix, items
        self.scratch, self.pass_entries, self.sandwich = scratch, pass_entries, sandwich


def _run_cases(driver, tmp, cases, timeout=300):
    """name -> (per-item words, the case's words, the outputs item by item)"""
    lines = []
    for name, c in cases.items():
        lines.append("case %d %d %s %d %d %s %d" % (c.policy, c.prefix, c.scratch, c.pass_entries, c.sandwich,
                                                    tmp / (name + ".out"), len(c.items)))
        lines += ["%s %d %d %s" % it for it in c.items]
    (tmp / "cases.list").write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, "batch", str(tmp / "cases.list")], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    words, results, at = _words(r.stdout), {}, 0
    for name, c in cases.items():
        items, case = words[at:at + len(c.items)], words[at + len(c.items)]
        at += len(c.items) + 1
        assert [w["item"] for w in items] == list(range(len(c.items))) and "case" in case
        blob, outs, pos = (tmp / (name + ".out")).read_bytes(), [], 0
        for w in items:
            outs.append(blob[pos:pos + w["size"]])
            pos += w["size"]
        assert pos == len(blob)
        results[name] = (items, case, outs)
    assert at == len(words)
    return results


# ---- the pool: liblz4's own frames and the planned ones -----------------------------------------------------------
def _pool():
    """[(name, plan)]; a fixture's plan carries the manifest's word as its content"""
    pool = [(p.name, p) for p in G.all_plans()]
    manifest = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    for name, m in manifest.items():
        if name == "liblz4":
            continue
        frame = open(os.path.join(GOLDEN, name + ".lz4"), "rb").read()
        assert hashlib.sha256(frame).hexdigest() == m["frame_sha256"], name
        pool.append(("golden_" + name, G.Plan("golden_" + name, frame, content=m, blocks=m["blocks"], bare=m["bare"])))
    return pool


def _write_pool(tmp):
    files = {}
    for k, (name, p) in enumerate(_pool()):
        files[name] = tmp / ("%d.lz4" % k)
        files[name].write_bytes(p.data)
    return files


def _content_ok(p, got):
    if isinstance(p.content, dict):
        return len(got) == p.content["content_bytes"] and hashlib.sha256(got).hexdigest() == p.content["content_sha256"]
    return got == p.content


def _check_item(p, policy, w, got, capacity="E"):
    """one item of a batch: what the plan says, what the single read gave, what the one-item batch gave"""
    assert w["guards"] == 1, ("bytes outside an output's capacity were written", p.name, w)
    want = p.status(policy)
    exact = w["query"]
    if capacity == "S" and exact > 0 and want in (G.SUCCESS, G.CANNOT_VERIFY):
        assert w["status"] == w["one_status"] == G.CANNOT_DECOMPRESS and w["size"] == w["one_size"] == 0, (p.name, w)
        return
    assert w["status"] == want, (p.name, p.reason, p.flipped, w)
    assert w["one_status"] == want and w["one_size"] == w["size"] and w["eq_one"] == 1, (p.name, w)
    assert w["single_status"] == want, ("decompress_frame itself says otherwise", p.name, w)
    if want in (G.SUCCESS, G.CANNOT_VERIFY):
        assert w["size"] == w["single_size"] == exact == len(got) and w["eq_single"] == 1, (p.name, w)
        assert _content_ok(p, got), p.name
    else:
        assert w["size"] == 0 and got == b"", ("a failing item has no size", p.name, w)


# ---- 1. equivalence -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def equivalence(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frames_eq")
    files = _write_pool(tmp)
    cases = {"p%d" % policy: Case(policy, NONE, [(files[name], 0, -1, "E") for name, _ in _pool()],
                                 scratch="scratch" if policy == 0 else "own", sandwich=1) for policy in POLICIES}
    return _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("policy", POLICIES)
def test_one_item_batches_equal_decompress_frame(equivalence, policy):
    items, case, outs = equivalence["p%d" % policy]
    pool = _pool()
    assert case["items"] == len(pool) and case["scratch_guard"] == 1 and case["passes"] >= 1
    assert case["blocks"] >= sum(p.blocks for _, p in pool if p.reason == "ok"), "the data blocks of the legal items at least"
    assert any(name == "linked_overlap" for name, _ in pool), "the smallest linked frame whose second block copies from its first"
    for (name, p), w, got in zip(pool, items, outs):
        _check_item(p, policy, w, got)
    assert case["sandwich"] == 1, "decompress_frame behind the batch does not give what it gave in front of it"


# ---- 2. isolation -------------------------------------------------------------------------------------------------
def _isolation_batches():
    """name -> [(pool name, capacity word)]: hostile items first, in the middle and last; every third legal item one
    byte short, every third oversize"""
    pool = _pool()
    legal = [n for n, p in pool if p.reason == "ok" and not p.flipped and not n.startswith("golden_harness")]
    # (the ones with a wrong checksum and the unsupported ones in front: every batch of 65 has them)
    hostile = sorted((n for n, p in pool if p.reason != "ok" or p.flipped),
                     key=lambda n: (not dict(pool)[n].flipped, dict(pool)[n].reason not in G.NOT_SUPPORTED_REASONS))
    batches = {"n1": [(legal[5], "E")], "n3": [(hostile[0], "E"), (legal[7], "O"), (hostile[1], "E")]}
    for n in (65, 300):
        row = []
        for k in range(n):
            if k in (0, n // 2, n - 1) or k % 7 == 3:
                row.append((hostile[sum(1 for _, c in row if c == "H") % len(hostile)], "H"))
            else:
                row.append((legal[(k * 3 + n) % len(legal)], "ESO"[k % 3]))
        batches["n%d" % n] = [(name, "E" if cap == "H" else cap) for name, cap in row]
    return batches


@pytest.fixture(scope="module")
def isolation(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frames_iso")
    files = _write_pool(tmp)
    cases = {}
    for name, row in _isolation_batches().items():
        for policy in (3, 4):
            cases["%s_p%d" % (name, policy)] = Case(policy, NONE, [(files[n], 0, -1, cap) for n, cap in row])
    return _run_cases(driver, tmp, cases, timeout=600)


@pytest.mark.parametrize("policy", (3, 4))
@pytest.mark.parametrize("name", list(_isolation_batches()))
def test_items_do_not_touch_each_other(isolation, name, policy):
    items, case, outs = isolation["%s_p%d" % (name, policy)]
    row, plans = _isolation_batches()[name], dict(_pool())
    assert case["items"] == len(row) and case["scratch_guard"] == 1
    kinds = set()
    for (n, cap), w, got in zip(row, items, outs):
        _check_item(plans[n], policy, w, got, cap)
        kinds.add((cap, w["status"]))
    if len(row) >= 65:
        assert ("S", G.CANNOT_DECOMPRESS) in kinds and kinds & {("O", G.SUCCESS), ("O", G.CANNOT_VERIFY)} \
            and ("E", G.BAD_CHECKSUM) in kinds and ("E", G.NOT_SUPPORTED) in kinds, kinds


# ---- 3. passes ----------------------------------------------------------------------------------------------------
def _passes_items():
    """a 5-block linked frame whose blocks reach back into the ones before them, an empty item, three 1-block items, a
    3-block independent frame with block checksums: 11 data blocks"""
    content, blocks = bytearray(b"0123456789abcdef"), [(b"0123456789abcdef", True)]
    for k in range(4):
        b = G.sequence(bytes([65 + k]) * 3, 11 + k, 9 + k) + G.sequence(b"<%03d>" % k)
        content += G.decode_block(b, bytes(content))
        blocks.append((b, False))
    linked = G.frame(blocks, 4, True, False, True, len(content), bytes(content))
    ones = [G.frame([(b"stored-%d" % k, True)], 4) if k != 1 else G.frame([(G.sequence(b"abcd", 4, 12) + G.sequence(b"vwxyz"), False)], 5)
            for k in range(3)]
    one_contents = [b"stored-0", G.decode_block(G.sequence(b"abcd", 4, 12) + G.sequence(b"vwxyz")), b"stored-2"]
    ind_blocks = [G.sequence(b"block-%d " % k, 8, 40 + k) + G.sequence(b"tail!") for k in range(3)]
    ind_content = b"".join(G.decode_block(b) for b in ind_blocks)
    independent = G.frame([(b, False) for b in ind_blocks], 4, False, True, False, len(ind_content))
    return [(linked, bytes(content)), (b"", b"")] + list(zip(ones, one_contents)) + [(independent, ind_content)]


@pytest.fixture(scope="module")
def passes(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frames_passes")
    rows = []
    for k, (data, _) in enumerate(_passes_items()):
        (tmp / ("%d.lz4" % k)).write_bytes(data)
        rows.append((tmp / ("%d.lz4" % k), 0, -1, "E"))
    cases = {"two_entries": Case(3, NONE, rows, scratch="scratch", pass_entries=2), "large": Case(3, NONE, rows),
             "three_entries_p4": Case(4, NONE, rows, pass_entries=3)}
    return _run_cases(driver, tmp, cases)


def test_blocks_of_items_span_passes(passes):
    want = _passes_items()
    small, large, three = passes["two_entries"], passes["large"], passes["three_entries_p4"]
    assert (small[1]["blocks"], small[1]["passes"], small[1]["pass_entries"], small[1]["scratch_guard"]) == (11, 6, 2, 1), small[1]
    assert (large[1]["blocks"], large[1]["passes"]) == (11, 1) and large[1]["pass_entries"] >= 11
    assert (three[1]["blocks"], three[1]["passes"], three[1]["pass_entries"]) == (11, 4, 3)
    for (_, content), ws, wl, gs, gl in zip(want, small[0], large[0], small[2], large[2]):
        assert ws["status"] == wl["status"] == G.SUCCESS and ws["guards"] == wl["guards"] == 1, (ws, wl)
        assert ws["size"] == wl["size"] == ws["query"] == len(content) and gs == gl == content
        assert ws["eq_single"] == 1 and ws["single_status"] == G.SUCCESS
    # ComputeAndVerify: the linked frame and the checksummed one verify, the bare ones cannot
    assert [w["status"] for w in three[0]] == [G.SUCCESS, G.SUCCESS] + [G.CANNOT_VERIFY] * 3 + [G.SUCCESS]
    assert three[2] == [c for _, c in want]


def test_caller_scratch_below_the_minimum_throws(driver):
    """A caller's scratch is get_required_scratch_buffer_size() bytes by contract: set_scratch_buffer takes no size, so
    no test can hand the manager a buffer one byte smaller.  What a batch needs of it grows with its items, 160 bytes
    each, so the limit is met from the other side and in steps of an item: the most items whose state and two entries
    fit are read; one more -- a need between 1 and 160 bytes above what the buffer has -- throws.  The byte boundary
    itself (one byte below the minimum holds no pass) is tests/test_lz4_frames_plan_cpu.py's, on the arithmetic that
    the manager calls.  The throw comes before anything is launched: the head of the scratch, where the items' state
    would go, and the result arrays are as they were, and the call counts no items."""
    first = _simple(driver, "limit", 1024, 1)[0]
    assert first["threw"] == 0 and first["worst_status"] == 0 and first["scratch_guard"] == 1
    assert first["untouched"] == 0 and first["stats_items"] == 1, "a call that runs writes its state and its results"
    room = first["scratch_bytes"] - 16
    most = (room - 128 - 2 * ENTRY_BYTES) // ITEM_BYTES
    assert 1 < most < 1 << 20, "the limit of 2^20 items comes first: this manager's scratch does not show the scratch's limit"
    assert most * ITEM_BYTES + 128 + 2 * ENTRY_BYTES <= room < (most + 1) * ITEM_BYTES + 128 + 2 * ENTRY_BYTES
    fits, over = _simple(driver, "limit", 1024, most)[0], _simple(driver, "limit", 1024, most + 1)[0]
    assert fits["threw"] == 0 and fits["worst_status"] == 0 and fits["scratch_guard"] == 1 and fits["stats_items"] == most, fits
    assert over["threw"] == 1 and over["scratch_guard"] == 1, over
    assert over["untouched"] == 1 and over["stats_items"] == 0, ("the call that threw launched something", over)


# ---- 4. Arrow -----------------------------------------------------------------------------------------------------
def _prefix_rows():
    """name -> (item bytes, capacity word, status, decoded bytes, whether a bare frame or a buffer stored whole was read:
    ComputeAndVerify cannot verify those) around one small frame of 11 bytes"""
    data = b"hello arrow"
    f = G.frame([(data, True)], 4)
    q = lambda p: struct.pack("<q", p)
    return {
        "true_size": (q(11) + f, "E", G.SUCCESS, data, True),
        "one_more": (q(12) + f, "E", G.CANNOT_DECOMPRESS, b"", False),
        "one_less": (q(10) + f, "E", G.CANNOT_DECOMPRESS, b"", False),
        "above_capacity": (q(11) + f, "10", G.CANNOT_DECOMPRESS, b"", False),
        "oversize_capacity": (q(11) + f, "O", G.SUCCESS, data, True),
        "stored": (q(-1) + data, "E", G.SUCCESS, data, True),
        "stored_above_capacity": (q(-1) + data, "10", G.CANNOT_DECOMPRESS, b"", False),
        "stored_nothing": (q(-1), "E", G.SUCCESS, b"", True),
        "minus_two": (q(-2) + f, "E", G.CANNOT_DECOMPRESS, b"", False),
        "no_bytes": (b"", "E", G.SUCCESS, b"", False),
        "seven_bytes": (q(11)[:7], "E", G.CANNOT_DECOMPRESS, b"", False),
        "eight_bytes_zero": (q(0), "E", G.SUCCESS, b"", False),
        "eight_bytes_five": (q(5), "E", G.CANNOT_DECOMPRESS, b"", False),
        "two_frames": (q(22) + f + G.skippable(b"..") + f, "E", G.SUCCESS, data * 2, True),
        "not_a_frame": (q(11) + b"\x00" * 20, "E", G.CANNOT_DECOMPRESS, b"", False),
    }


def _framed(items):
    """the items of a manifest that are a prefix and a frame: not the empty ones, not the ones stored whole"""
    return [it for it in items if it["length"] and not it["stored"]]


def _prefix_query(item):
    if len(item) < 8:
        return 0
    p, = struct.unpack_from("<q", item)
    return len(item) - 8 if p == -1 else max(p, 0)


@pytest.fixture(scope="module")
def arrow(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lz4_frames_arrow")
    cases = {}
    for name in A.FIXTURES:
        body, items = A.load(name)
        (tmp / (name + ".body")).write_bytes(body)
        for policy, cap in ((0, "E"), (3, "O"), (4, "E")):
            cases["%s_p%d" % (name, policy)] = Case(policy, ARROW, [(tmp / (name + ".body"), it["offset"], it["length"], cap)
                                                                   for it in items], scratch="scratch" if policy == 3 else "own")
        # the frames alone, without their prefixes: the size query has to parse them (no content size, linked blocks)
        cases["%s_frames" % name] = Case(3, NONE, [(tmp / (name + ".body"), it["offset"] + 8, it["length"] - 8, "E")
                                                   for it in _framed(items)])
    blob, rows = b"", []
    for name, (item, cap, _, _, _) in _prefix_rows().items():
        rows.append((tmp / "prefix.bin", len(blob), len(item), cap))
        blob += item + b"\xee" * 5
    (tmp / "prefix.bin").write_bytes(blob)
    for policy in (0, 4):
        cases["prefix_p%d" % policy] = Case(policy, ARROW, rows)
    cases["all_empty"] = Case(0, ARROW, [(tmp / "prefix.bin", 3, 0, "O")] * 5)
    # the size query without a prefix: a declared size, none, a false one
    data = b"hello arrow"
    for k, f in enumerate((G.frame([(data, True)], 4, content_size=11), G.frame([(data, True)], 4), G.frame([(data, True)], 4, content_size=12),
                           G.frame([(data, True)], 4, content_size=11) + G.frame([(G.sequence(b"ab", 2, 30) + G.sequence(b"12345"), False)], 4))):
        (tmp / ("q%d.lz4" % k)).write_bytes(f)
    cases["query_none"] = Case(0, NONE, [(tmp / ("q%d.lz4" % k), 0, -1, "E") for k in range(4)])
    return _run_cases(driver, tmp, cases)


@pytest.mark.parametrize("policy", (0, 3, 4))
@pytest.mark.parametrize("name", A.FIXTURES)
def test_arrow_body(arrow, name, policy):
    _, manifest = A.load(name)
    items, case, outs = arrow["%s_p%d" % (name, policy)]
    assert case["items"] == len(manifest) and case["scratch_guard"] == 1 and case["passes"] == 1
    for it, w, got in zip(manifest, items, outs):
        # (Arrow's frames carry no checksum, and a buffer stored whole has none to carry)
        want = G.CANNOT_VERIFY if policy == 4 and it["length"] else G.SUCCESS
        assert w["status"] == w["one_status"] == want and w["guards"] == 1, (it, w)
        assert w["size"] == w["one_size"] == w["query"] == it["decoded_size"] == len(got), (it, w)
        assert hashlib.sha256(got).hexdigest() == it["sha256"], it


@pytest.mark.parametrize("name", A.FIXTURES)
def test_arrow_frames_without_prefix(arrow, name):
    """LZ4FramePrefix::None on what Arrow writes: the size query finds every buffer's size by the parse (walk, token
    walk of the linked blocks, the batched decoder's parse-only pass), all items in one pass, and the decode gives the
    manifest's bytes"""
    manifest = _framed(A.load(name)[1])
    items, case, outs = arrow["%s_frames" % name]
    assert len(manifest) >= 4 and case["items"] == len(manifest) and case["passes"] == 1 and case["scratch_guard"] == 1
    assert case["blocks"] >= len(manifest) + 3, "several of the buffers have more than one block"
    for it, w, got in zip(manifest, items, outs):
        assert w["query"] == it["decoded_size"], ("the size query without a prefix", it, w)
        assert w["status"] == w["one_status"] == w["single_status"] == G.SUCCESS and w["guards"] == 1, (it, w)
        assert w["size"] == w["one_size"] == w["single_size"] == it["decoded_size"] == len(got), (it, w)
        assert w["eq_single"] == 1 and w["eq_one"] == 1 and hashlib.sha256(got).hexdigest() == it["sha256"], it


@pytest.mark.parametrize("policy", (0, 4))
def test_prefix_table(arrow, policy):
    items, case, outs = arrow["prefix_p%d" % policy]
    for (name, (item, cap, status, data, bare)), w, got in zip(_prefix_rows().items(), items, outs):
        if policy == 4 and bare:
            status = G.CANNOT_VERIFY
        assert w["status"] == w["one_status"] == status and w["guards"] == 1, (name, w)
        assert w["size"] == w["one_size"] == len(data) and got == data, (name, w)
        assert w["query"] == _prefix_query(item), (name, "the size query reads the prefix and nothing else", w)


def test_all_empty_batch_launches_no_pass(arrow, driver):
    items, case, outs = arrow["all_empty"]
    assert (case["items"], case["blocks"], case["passes"], case["scratch_guard"]) == (5, 0, 0, 1)
    assert all(w["status"] == 0 and w["size"] == 0 and w["query"] == 0 and w["guards"] == 1 for w in items)
    w = _simple(driver, "nothing")[0]
    assert w == {"threw": 0, "items": 0, "misuse_threw": 2}, "num_items == 0 succeeds; a null array or 2^20 + 1 items throw"


def test_size_query_without_prefix(arrow):
    items, _, outs = arrow["query_none"]
    data, tail = b"hello arrow", b"ab" * 16 + b"12345"
    assert [w["query"] for w in items] == [11, 11, 12, 11 + len(tail)], "declared, parsed, declared falsely, one of two frames declares"
    assert [w["single_size"] for w in items] == [w["query"] for w in items], "configure_frame_decompression says the same"
    assert [w["status"] for w in items] == [0, 0, G.CANNOT_DECOMPRESS, 0] == [w["single_status"] for w in items]
    assert outs == [data, data, b"", data + tail]


# ---- 6. the paths that were there -----------------------------------------------------------------------------------
def test_frame_and_range_reads_are_unchanged_by_a_batch(driver, tmp_path):
    (tmp_path / "text.bin").write_bytes(G._text(200000, 5))
    w = _simple(driver, "unchanged", tmp_path / "text.bin")[0]
    assert w == {"frame_same": 1, "range_same": 1, "batch_worst": 0}, w
