"""tests/snappy_inputgen.py checked without a GPU, at the seeds tests/test_snappy_encoder_forms_gpu.py uses: the
oracle's stream of EVERY case has exactly the elements the case's plan lists (no case is left out: a plan the oracle
does not reproduce is a bug of the generator), decodes back to the input through streamgen's plain loop, and fits
the size bound; the census says that every parameter value a family lists occurs; the same seed gives the same
bytes."""
import pytest

import snappy_inputgen as IG
import streamgen as SG


def _decode_plain(elements, stream):
    """The stream's elements applied one byte at a time (streamgen.expected_snappy's loop, literal bytes taken
    from the stream)."""
    plan = []
    i = len(SG.varint(IG.parse_elements(stream)[0]))
    for e in elements:
        if e[0] == "L":
            hdr = 1 if e[1] <= 60 else 2 if e[1] <= 256 else 3
            plan.append(("L", stream[i + hdr:i + hdr + e[1]], 0))
            i += hdr + e[1]
        else:
            plan.append(("C", 2, e[1], e[2]))
            i += 2 if e[1] < 12 and e[2] < 2048 else 3
    assert i == len(stream)
    return SG.expected_snappy(plan)


@pytest.mark.parametrize("name", list(IG.FAMILIES))
def test_oracle_reproduces_every_plan(oracle, name):
    cases = IG.family(name)
    assert cases
    assert len({c[0] for c in cases}) == len(cases), "case names repeat"
    wrong, checked = [], 0
    for case, data, plan in cases:
        stream = oracle.snappy_compress(data)
        assert len(stream) <= oracle.snappy_max_compressed_size(len(data)), case
        size, elements = IG.parse_elements(stream)
        assert size == len(data), case
        assert _decode_plain(elements, stream) == data, f"{case}: the oracle's stream does not decode to the input"
        checked += 1
        if elements != list(plan):
            k = next((i for i, (a, b) in enumerate(zip(elements, plan)) if a != b), min(len(elements), len(plan)))
            wrong.append(f"{case}: element {k}: oracle {elements[k:k + 3]} planned {list(plan)[k:k + 3]}")
    print(f"\n{name}: {len(cases)} cases, {sum(len(c[1]) for c in cases)} input bytes, "
          f"left out of the element check: {len(cases) - checked}")
    assert checked == len(cases)
    assert not wrong, f"{len(wrong)} of {len(cases)} plans not reproduced:\n" + "\n".join(wrong[:20])


def _tags(name):
    return [plan.tags for _, _, plan in IG.family(name)]


def _behind_reset(oracle, data):
    """From the ORACLE's stream of a case whose first copy is the reset: the elements behind that copy as
    [(trip lane of the hit, copy length, distance)] up to the first copy of 16 bytes or more (included), lanes
    counted from the reset's end -- what the tags claim, measured on the bytes."""
    _, elements = IG.parse_elements(oracle.snappy_compress(data))
    first = next(i for i, e in enumerate(elements) if e[0] == "C")
    assert elements[first][1] == IG.RESET_LEN
    lane, out = 0, []
    for e in elements[first + 1:]:
        if e[0] == "L":
            lane += e[1]
        else:
            out.append((lane, e[1], e[2]))
            lane += e[1]
            if e[1] >= 16:
                break
    return out


def test_census(oracle):
    # the lanes, lengths, distances and lane sums of the tags, measured on the oracle's streams
    for name, data, plan in IG.family("hit_lane_by_length"):
        got, t = _behind_reset(oracle, data), plan.tags
        if "L" in t:
            assert got[0] == (t["lane"], min(t["L"], 64), t["D"]), (name, got[:2])
        else:
            assert got == [], (name, got)
    for name, data, plan in IG.family("trips"):
        got, t = _behind_reset(oracle, data), plan.tags
        short = [g for g in got if g[1] < 16]
        assert [lane + ln for lane, ln, _ in short] == t["sums"], (name, got)
        assert sum(1 for _, ln, d in short if ln < 12 and d < 2048) == t["twos"], name
        assert (len(got) > len(short)) == (t["ended_after"] is not None), name
    for name, data, plan in IG.family("matchless_windows"):
        got, t = _behind_reset(oracle, data), plan.tags
        if "stretch" in t:
            assert got[0][0] == t["stretch"], (name, got)
        if "window" in t:
            assert got[0][0] == 64 * (t["window"] - 1) + t["lane"], (name, got)
    # a last window with lanes that have no 4-byte word: every chunk that ends less than 67 bytes behind the start
    # of its last search window -- counted on the oracle's elements
    short_last = 0
    for name, data, plan in IG.family("chunk_ends"):
        _, elements = IG.parse_elements(oracle.snappy_compress(data))
        if elements and elements[-1][0] == "L" and elements[-1][1] % 64 != 0 or elements and elements[-1][0] == "C":
            short_last += 1
    hit = _tags("hit_lane_by_length")
    lanes = {t["lane"] for t in hit if "L" in t}
    lengths = {t["L"] for t in hit if "L" in t}
    dists = {t["D"] for t in hit if "L" in t}
    none = {t["no_hit_D"] for t in hit if "no_hit_D" in t}
    overlapping = sum(1 for t in hit if "L" in t and t["D"] < t["L"])
    tr = _tags("trips")
    sums = {s for t in tr for s in t["sums"]}
    last_sums = {t["sums"][-1] for t in tr if t["sums"]}
    counts = {t["elements"] for t in tr}
    sh = {t["layout"] for t in _tags("shared_hashes")}
    ml = _tags("matchless_windows")
    stretches = {t["stretch"] for t in ml if "stretch" in t}
    windows = {(t["window"], t["lane"]) for t in ml if "window" in t}
    quirk = {t["quirk_lane"]: t["quirk_found"] for t in ml if "quirk_lane" in t}
    en = _tags("chunk_ends")
    totals = {t["total"] for t in en if "total" in t}
    backs = {(t["start_back"], bool(t.get("after_short")), bool(t.get("after_general"))) for t in en
             if "start_back" in t}
    left = {t["left_behind_match"] for t in en if "left_behind_match" in t}
    cut = {t["match60_cut"] for t in en if "match60_cut" in t}
    lastl = {t["last_literals"] for t in en if "last_literals" in t}
    be = {t["kind"] for t in _tags("beyond_64k")}
    print("\nSnappy planned-input census")
    for name in IG.FAMILIES:
        cs = IG.family(name)
        print(f"  {name}: {len(cs)} cases, {sum(len(c[1]) for c in cs)} bytes")
    print(f"  hit_lane_by_length: lanes {sorted(lanes)}; L {sorted(lengths)}; D {sorted(dists)} "
          f"({overlapping} overlapping); no hit at D {sorted(none)}")
    print(f"  trips: elements per trip {sorted(counts)}; lane sums met {sorted(s for s in sums if s in IG.TRIP_SUMS)}"
          f"; trips ending at {sorted(last_sums)}; chained k = 0: {sum(t['k0_chain'] for t in tr)}; two-byte / "
          f"three-byte copies {sum(t['twos'] for t in tr)} / {sum(t['threes'] for t in tr)}; ended by a long match "
          f"after {sorted({t['ended_after'] for t in tr if t['ended_after'] is not None})} short ones")
    print(f"  shared_hashes: {sorted(sh)}")
    print(f"  matchless_windows: stretches {sorted(stretches)}; (window, lane) {sorted(windows)}; lane-0 quirk, "
          f"source lane -> found: {quirk}")
    print(f"  chunk_ends: totals {sorted(totals)}; element starts (back, after short, after general) {sorted(backs)}; "
          f"bytes left behind a last match {sorted(left)}; Match60 cut at {sorted(cut)}; last literals {sorted(lastl)}")
    print(f"  chunk_ends: {short_last} chunks whose last window has lanes without a 4-byte word")
    print(f"  beyond_64k: {sorted(be)}")
    co = IG.family("composed")
    for name, data, plan in co:
        print(f"  {name}: {len(data)} bytes, {len(plan.tags['situations'])} situations {plan.tags['per_family']}, "
              f"{len(plan)} elements, gave up {plan.tags['gave_up']}")

    assert lanes >= set(IG.HIT_LANES) and lengths >= set(IG.HIT_LENGTHS) and dists >= set(IG.HIT_DISTANCES)
    assert none >= set(IG.NO_HIT_DISTANCES) and overlapping >= 6
    assert set(IG.TRIP_SUMS) <= last_sums and counts >= {2, 5, 9, 12}
    assert sum(t["k0_chain"] for t in tr) >= 6 and sum(1 for t in tr if t["twos"] and t["threes"]) >= 12
    assert {t["ended_after"] for t in tr if t["ended_after"] is not None} == {0, 1, 4}
    assert sh >= {"b_in_front_of_hit", "three_on_one_slot", "b_is_hit_lane", "b_inside_match", "a_is_hit_lane",
                  "stale_different_words", "stale_equal_words", "equal_words_in_front_of_hit",
                  "equal_words_same_window", "staying_lane_is_later_source", "inside_match_not_posted",
                  "hit_lane_posted", "equal_words_a_is_hit_lane", "equal_words_b_inside_match",
                  "three_equal_words", "stale_equal_words_late", "equal_words_in_front_of_hit_late",
                  "equal_words_b_is_hit_lane"}
    assert stretches >= set(IG.STRETCHES)
    assert windows >= {(w, lane) for w in (2, 3, 4) for lane in IG.WINDOW_LANES}
    assert quirk == {0: True, 1: False, 63: False}      # (the outcomes the plan lists; the oracle agreed above)
    assert totals >= set(IG.END_LENGTHS)
    assert backs >= {(b, s, False) for b in (143, 144, 145) for s in (False, True)}
    assert backs >= {(b, False, True) for b in (143, 144, 145)}
    assert left >= set(range(6)) and cut >= {0, 1, 30, 59} and lastl >= {1, 2, 3, 4}
    assert be >= {"source_before_line", "source_after_line", "far_source_over_line", "three_lines_on",
                  "stored_equals_pos0_low_bits_lane0_65536_back", "stored_equals_pos0_low_bits_lane3",
                  "alias_same_word", "alias_other_word"}
    assert short_last >= 40
    assert sorted(len(d) for _, d, _ in co) == sorted(IG.COMPOSED_SIZES)
    for name, data, plan in co:
        fams = set(plan.tags["per_family"])
        assert fams >= {"hit_lane_by_length", "trips", "shared_hashes", "matchless_windows", "chunk_ends"}, name
        assert len(plan.tags["situations"]) >= 60, name
    big = [plan for _, d, plan in co if len(d) == 1 << 20][0]
    assert "beyond_64k" in big.tags["per_family"]
    assert any(s.startswith("beyond/alias") or s.startswith("beyond/stored") for s in big.tags["situations"])


def test_generator_is_deterministic():
    for name in IG.FAMILIES:
        a = IG.FAMILIES[name](IG.SEEDS[name])
        b = IG.family(name)
        assert [(n, d, list(p)) for n, d, p in a] == [(n, d, list(p)) for n, d, p in b], name
    other = IG.FAMILIES["trips"](IG.SEEDS["trips"] + 1)
    assert [d for _, d, _ in other] != [d for _, d, _ in IG.family("trips")]
