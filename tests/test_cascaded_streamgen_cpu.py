"""tests/cascaded_streamgen.py against the oracle, and a census of what its families reach (CPU only).

The planner's expected() is three plain loops on Python ints; the oracle (oracle/cascaded_oracle.c) is the pinned
restatement of the reference decoder.  Every planned stream must decode in the oracle to exactly expected(), which
proves the stream legal and the expectation right before tests/test_cascaded_stream_forms_gpu.py shows it to a
GPU.  The census computes from the plans and the written streams -- not from any decoder -- whether each family
meets the forms it is there for, at every element width.
"""
import itertools

import pytest

import cascaded_streamgen as CS
import decode_guard as G

WIDTHS = (1, 2, 4, 8)


def _by_width(family):
    """{element size: [plan]} of a family."""
    out = {s: [] for s in WIDTHS}
    for p in CS.family(family):
        out[p.size].append(p)
    return out


def test_the_corpus_is_small_named_and_keeps_neighbouring_runs_apart():
    corpus = CS.corpus()
    assert 2000 <= len(corpus) <= 5000
    names = [p.name for p, _, _ in corpus]
    assert len(set(names)) == len(names)
    assert {p.family for p, _, _ in corpus} == set(CS.FAMILIES)
    for fam in CS.FAMILIES:
        assert {p.type for p in CS.family(fam)} == set(range(8)), fam
    for p, stream, e in corpus:
        assert len(p.subs) <= 4, p.name
        assert len(e) <= 4 * CS.SUB_CHUNK, p.name
        assert CS.runs_differ(p), p.name


def test_the_oracle_decodes_every_planned_stream_to_the_expected_bytes(oracle):
    wrong = []
    for p, stream, e in CS.corpus():
        st, got = oracle.cascaded_decompress(stream, len(e))
        size = oracle.cascaded_decompressed_size(stream)
        if (st, got, size) != (0, e, len(e)):
            wrong.append(f"{p.name} (status {st}, {len(got)} of {len(e)} bytes, size pass {size})")
    assert not wrong, f"{len(wrong)} of {len(CS.corpus())} streams wrong, first {wrong[:5]}"


def test_the_oracle_refuses_every_stream_at_one_element_short(oracle):
    wrong, seen = [], 0
    for p, stream, e in CS.corpus():
        if e:
            seen += 1
            if oracle.cascaded_decompress(stream, len(e) - p.size) != (12, b""):
                wrong.append(p.name)
    assert not wrong and seen > 2000, f"{len(wrong)} streams wrong, first {wrong[:5]}"


# ------------------------------------------------------------------------------------------------------- census

def _zero_positions(c, ce):
    """The positions of the issue's list an array of run lengths has an empty run at."""
    n, got = len(c), set()
    empty = [i for i in range(n) if c[i] == 0]
    for i in empty:
        if i == 0:
            got.add("first")
        if i + 1 < n and c[i + 1] > 0:
            got |= {"mod16"} if i % 16 == 15 else set()
            got |= {"mod64"} if i % 64 == 63 else set()
        if i + 1 < n and c[i + 1] == 0:
            got.add("multi")
            if i % 64 == 63:
                got.add("round64")   # (runs 63 and 64: the last of one round of 64 runs and the first of the next)
        if i == n - 1:
            got.add("last_full" if sum(c) == ce else "last_short")
    return got


def _array_kind(plan, a):
    if not plan.bp:
        return "raw"
    if a.fr == 0 and a.bw <= 12:
        return "packed12"
    return "packed16" if a.fr == 0 and 13 <= a.bw <= 16 else "other"


def test_census_zero_runs():
    positions = ("first", "mod16", "mod64", "last_full", "last_short", "multi", "round64")
    # (R, D, layer): R = 1 without and under a delta layer; R = 2 outer and inner layer, without a delta layer and
    # with one fused behind the inner expansion
    layers = ((1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1))
    for s, plans in _by_width("zero_runs").items():
        met = set()
        for p in plans:
            for sub in p.subs:
                for l, a in enumerate(sub.runs):
                    for where in _zero_positions(a.values, CS.SUB_CHUNK // s):
                        met.add((where, _array_kind(p, a), p.R, p.D, l))
        for where, kind, (R, D, l) in itertools.product(positions, ("raw", "packed12", "packed16"), layers):
            if where == "last_full" and l >= 1 and l - 1 < D:
                continue   # (the expansion feeds a delta layer, which adds an element: it cannot fill the sub-chunk)
            assert (where, kind, R, D, l) in met, (s, where, kind, R, D, l)


def _lower_marker_wins(plan):
    """The suspected fault as a model: an empty run's value covers the run behind it."""
    M = 1 << (8 * plan.size)
    out = []
    for sub in plan.subs:
        x = list(sub.final.values)
        for l in range(max(plan.R, plan.D) - 1, -1, -1):
            if l < plan.D:
                acc, y = sub.heads[l], []
                for v in x:
                    y.append(acc)
                    acc = (acc + v) % M
                x = y + [acc]
            if l < plan.R:
                y, held = [], None
                for cnt, v in zip(sub.runs[l].values, x):
                    if cnt == 0:
                        held = v if held is None else held
                    else:
                        y += [v if held is None else held] * cnt
                        held = None
                x = y
        out += x
    return out


def test_every_zero_runs_stream_can_show_the_lower_marker_fault():
    same = [p.name for p in CS.family("zero_runs") if _lower_marker_wins(p) == CS.decoded(p)]
    assert not same, f"{len(same)} streams decode alike under the fault, first {same[:5]}"
    assert all(_lower_marker_wins(p) == CS.decoded(p) for p in CS.family("encoder_like"))   # (the model itself)


def test_census_widths():
    for s, plans in _by_width("widths").items():
        M = 1 << (8 * s)
        exact, wide, lengths, zero_width = set(), set(), set(), False
        for p in plans:
            assert p.bp
            for sub in p.subs:
                a = sub.final
                if a.values:
                    need = max((v - a.fr) % M for v in a.values).bit_length()
                    (exact if need == a.bw else wide).add(a.bw)
                    assert need <= a.bw
                    zero_width |= a.bw == 0
                lengths |= {r.bw for r in sub.runs if r.values}
        assert exact == set(range(8 * s + 1)), (s, sorted(set(range(8 * s + 1)) - exact))
        assert wide == set(range(1, 8 * s + 1)), (s, sorted(set(range(1, 8 * s + 1)) - wide))
        assert lengths == set(range(17)), (s, sorted(lengths))
        assert zero_width


def test_census_frames_of_reference():
    for s, plans in _by_width("frames_of_reference").items():
        M = 1 << (8 * s)
        wraps, negative, over_none, over_some = False, set(), False, False
        for p in plans:
            for sub in p.subs:
                a = sub.final
                if any(a.fr + (v - a.fr) % M >= M for v in a.values):
                    wraps = True
                    if a.fr >= M // 2:
                        negative.add(p.type)
                for r in sub.runs:
                    if r.values and r.fr + (1 << r.bw) - 1 > 0xFFFF:
                        wrapped = [r.fr + (v - r.fr) % 65536 > 0xFFFF for v in r.values]
                        over_none |= not any(wrapped)
                        over_some |= any(wrapped)
        assert wraps and over_none and over_some, (s, wraps, over_none, over_some)
        assert negative >= {t for t in CS.SIGNED if CS.SIZE[t] == s}, (s, negative)


def _staged(rel, nbytes):
    """The decoder's array_staged(): the array lies within the first 1 KiB of its sub-chunk."""
    return rel + ((nbytes + 3) & ~3) <= 1024


def test_census_placement():
    for s, plans in _by_width("placement").items():
        met, slack, csz = set(), set(), False
        for p in plans:
            _, R, _, _, _, subs = G.cascaded_layout(CS.encode(p))
            assert len(subs) == len(p.subs), p.name
            for (pos, meta, at), sub in zip(subs, p.subs):
                for j, a in enumerate(sub.runs + [sub.final]):
                    rel, nbytes = at[j] - pos, meta[j + 1]
                    kind = "final" if j == R else "lengths"
                    where = "inside" if _staged(rel, nbytes) else ("straddle" if rel < 1024 else "behind")
                    met.add((kind, where))
                    if kind == "lengths" and (nbytes + 3) // 4 * 4 > 1024:
                        met.add(("lengths", "large", "raw" if not p.bp else "packed"))
                    if a.slack:
                        slack.add("raw" if not p.bp else "packed")
                csz |= sub.csz_slack % 4 != 0
        want = set(itertools.product(("final", "lengths"), ("inside", "straddle", "behind")))
        want |= {("lengths", "large", "raw"), ("lengths", "large", "packed")}
        assert met >= want, (s, sorted(want - met))
        assert slack == {"raw", "packed"}, (s, slack)
        assert csz


def _sizes(plan):
    """Elements each sub-chunk of a plan decodes to."""
    return [len(CS.decoded(CS.Plan("", "", plan.type, plan.R, plan.D, plan.bp, [sub]))) for sub in plan.subs]


def test_census_ragged():
    for s, plans in _by_width("ragged").items():
        ce, E = CS.SUB_CHUNK // s, 8 if s == 8 else 16
        orders, tiny, empty_packed, over_empty, to_full = set(), False, False, False, set()
        for p in plans:
            sizes = _sizes(p)
            if set(sizes) == {0, 1, E - 1, E}:
                orders.add(tuple(sizes))
            if 0 in sizes[1:-1] and max(sizes) == E:
                orders.add("empty in the middle")
            tiny |= len(sizes) == 4 and 1 <= min(sizes) and max(sizes) <= 3
            for sub, n in zip(p.subs, sizes):
                for a, es in [(r, 2) for r in sub.runs] + [(sub.final, s)]:
                    empty_packed |= bool(p.bp) and not a.values and a.bw > 8 * es and a.fr != 0
                over_empty |= p.D >= 1 and not sub.final.values and n == 1
                if p.D >= 1 and n == ce:
                    to_full.add(p.R > 0)
        assert len(orders) >= 4 and "empty in the middle" in orders, (s, orders)
        assert tiny and empty_packed and over_empty and to_full == {False, True}, (s, tiny, empty_packed, over_empty, to_full)
        assert any(not p.subs for p in plans)


def _metadata_size(s, R, D):
    """The decoder's chunk_metadata_size(): R + 2 size words, padded to the element, then D heads, padded to a word."""
    return (4 * (R + 2) + s - 1) // s * s + (s * D + 3) // 4 * 4


def test_census_depth():
    for s, plans in _by_width("depth").items():
        met = {(p.R, p.D) for p in plans}
        for R in range(8):
            fits = [D for D in range(64) if _metadata_size(s, R, D) <= 64 and (R, D) != (0, 0)]
            full = [D for D in fits if _metadata_size(s, R, D) == 64]
            below = [D for D in fits if _metadata_size(s, R, D) < 64]
            assert full or below
            for D in full + ([max(below)] if below else []):
                assert (R, D) in met, (s, R, D)
        assert max(D for R, D in met if R == 0) == {1: 56, 2: 28, 4: 14, 8: 7}[s]
        assert any(D > R >= 1 for R, D in met) and any(R > D >= 1 for R, D in met)
        assert any(R == 0 and D >= 1 for R, D in met) and any(R == 7 for R, D in met)
        assert all(_metadata_size(s, p.R, p.D) <= 64 and p.subs for p in plans)


def test_census_encoder_like_and_raw():
    for s, plans in _by_width("encoder_like").items():
        ce = CS.SUB_CHUNK // s
        for p in plans:
            assert _sizes(p)[:-1] == [ce] * (len(p.subs) - 1), p.name   # full sub-chunks but for the last
            for sub in p.subs:
                assert not sub.csz_slack and all(a.slack == 0 for a in sub.runs + [sub.final])
                assert all(min(r.values) >= 1 for r in sub.runs)
                if p.bp:
                    assert all((r.fr, r.bw) == (min(r.values), (max(r.values) - min(r.values)).bit_length())
                               for r in sub.runs)
        assert {(p.R > 0, p.D > 0, p.bp > 0) for p in plans} >= {(True, False, False), (False, True, False),
                                                                 (False, False, True), (True, True, True)}
    for s, plans in _by_width("raw").items():
        assert all((p.R, p.D, p.bp) == (0, 0, 0) for p in plans)
        assert any(p.raw and p.tail for p in plans) and any(not p.raw for p in plans)
        assert any(len(p.raw) > CS.SUB_CHUNK for p in plans)
