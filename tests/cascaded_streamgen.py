"""Seeded planner of legal Cascaded partitions in forms the encoder never writes (CPU only: plain Python).

The Cascaded decoder promises to decode every stream the format allows; the encoder writes a narrow part of them
(minimal bit widths, the signed minimum as frame of reference, runs of at least one element, full sub-chunks, no
slack).  Every stream here is written from an explicit Plan: the type byte, R (RLE layers), D (delta layers), the
bit-pack byte and a list of sub-chunks (Sub), each with its delta heads, one run-length array per RLE layer and the
final value array.  An array (Arr) says how it is written: its elements, and where the partition is bit-packed the
frame of reference and the bit width chosen for it; `slack` is what its meta[] length claims beyond what it needs,
Sub.csz_slack what the sub-chunk's size word claims beyond the sub-chunk.  Every plan is valid by construction
(nothing is drawn and then discarded: a value that must differ from another is drawn from the range without it).

    encode(plan)   -> the wire format (don't-care bytes and bits hold seeded non-zero filler)
    expected(plan) -> the decoded bytes, the layers undone in the plainest loops there are, on Python ints
                      modulo 2^(8 size)

Neither shares code with oracle/ or the kernels.  Layer l of the encoder is RLE_l then Delta_l, so a sub-chunk is
decoded for l = max(R, D) - 1 .. 0 by: undo Delta_l (if l < D), then expand RLE_l (if l < R).

Neighbouring runs carry different values, so that a misplaced run shows in the bytes: the values that enter an RLE
layer are either the final array (drawn with unequal neighbours), or the sums of a delta layer over non-zero
elements (heads are chosen so that sums which feed another delta layer are non-zero too), or the output of another
expansion -- and then the inner of the two layers has lengths of 0 and 1 only, or the outer one is all ones
(runs_differ() says so for a plan; tests/test_cascaded_streamgen_cpu.py holds every plan to it).

Families (FAMILIES; family(name) -> [Plan], corpus() -> all of them, every family over all eight types):
encoder_like, zero_runs, widths, frames_of_reference, placement, ragged, depth, raw -- see each function.  Streams
are small: four sub-chunks at most, sub-chunks of at most 4096 / size elements.

Used by tests/test_cascaded_streamgen_cpu.py (the planner against the oracle, and its census) and
tests/test_cascaded_stream_forms_gpu.py (the batched decoder against expected()).
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

SIZE = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 8, 7: 8}
SIGNED = (0, 2, 4, 6)
SUB_CHUNK = 4096
FAMILIES = ("encoder_like", "zero_runs", "widths", "frames_of_reference", "placement", "ragged", "depth", "raw")


def ru(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def metadata_size(s: int, R: int, D: int) -> int:
    return ru(4 + 4 * (R + 1), s) + ru(s * D, 4)


@dataclass
class Arr:
    values: List[int]          # the elements (unsigned, below 2^(8 element size))
    fr: int = 0                # bit-packed: frame of reference (unsigned) ...
    bw: int = 0                # ... and bit width: (value - fr) mod 2^(8 es) < 2^bw for every element
    slack: int = 0             # bytes its meta[] length claims beyond the array


@dataclass
class Sub:
    heads: List[int]           # D delta heads
    runs: List[Arr]            # R arrays of run lengths (16-bit elements), layer 0 first
    final: Arr
    csz_slack: int = 0         # bytes the size word claims beyond the sub-chunk


@dataclass
class Plan:
    family: str
    name: str
    type: int
    R: int
    D: int
    bp: int
    subs: List[Sub] = field(default_factory=list)
    raw: bytes = b""           # R = D = bp = 0: the data
    tail: int = 0              # bytes behind the last sub-chunk (fewer than a word), or behind the raw data
    seed: int = 0              # of the filler

    @property
    def size(self) -> int:
        return SIZE[self.type]


# ------------------------------------------------------------------------------------------ encode / expected

def _filler(rnd, n: int) -> bytes:
    return bytes(rnd.randrange(1, 256) for _ in range(n))


def _array_bytes(a: Arr, es: int, packed: bool, rnd) -> bytes:
    """The array as written, slack included: len() of it is its meta[] length."""
    M = 1 << (8 * es)
    if not packed:
        assert a.slack < es, "a raw array's length is its element count"
        return b"".join(v.to_bytes(es, "little") for v in a.values) + _filler(rnd, a.slack)
    hdr, w_off, n = ru(es + 4, es if es > 4 else 4), ru(es, 4), len(a.values)
    head = bytearray(_filler(rnd, hdr))
    head[0:es] = (a.fr % M).to_bytes(es, "little")
    head[w_off:w_off + 4] = ((a.bw << 16) | n).to_bytes(4, "little")
    data = b""
    if n:
        assert a.bw <= 8 * es
        acc = 0
        for i, v in enumerate(a.values):
            r = (v - a.fr) % M
            assert r < (1 << a.bw), (v, a.fr, a.bw)
            acc |= r << (i * a.bw)
        bits = n * a.bw
        words = (bits + 31) // 32
        acc |= rnd.getrandbits(32) >> (32 - (words * 32 - bits)) << bits if words * 32 > bits else 0
        data = acc.to_bytes(words * 4, "little")
    return bytes(head) + data + _filler(rnd, a.slack)


def decoded(plan: Plan) -> List[int]:
    """The elements a plan decodes to (cached on the plan)."""
    got = getattr(plan, "_decoded", None)
    if got is not None:
        return got
    M = 1 << (8 * plan.size)
    out: List[int] = []
    for sub in plan.subs:
        x = list(sub.final.values)
        for l in range(max(plan.R, plan.D) - 1, -1, -1):
            if l < plan.D:
                acc, y = sub.heads[l], []
                for v in x:
                    y.append(acc)
                    acc = (acc + v) % M
                y.append(acc)
                x = y
            if l < plan.R:
                c = sub.runs[l].values
                assert len(c) == len(x)
                y = []
                for cnt, v in zip(c, x):
                    for _ in range(cnt):
                        y.append(v)
                x = y
        assert len(x) <= SUB_CHUNK // plan.size
        out += x
    plan._decoded = out
    return out


def expected(plan: Plan) -> bytes:
    if plan.R == 0 and plan.D == 0 and plan.bp == 0:
        return plan.raw
    s = plan.size
    return b"".join(v.to_bytes(s, "little") for v in decoded(plan))


def encode(plan: Plan) -> bytes:
    s, R, D = plan.size, plan.R, plan.D
    rnd = random.Random(plan.seed)
    out = bytearray([R, D, plan.bp, plan.type]) + len(expected(plan)).to_bytes(4, "little")
    out += _filler(rnd, ru(8, s) - 8)
    if R == 0 and D == 0 and plan.bp == 0:
        return bytes(out + plan.raw + _filler(rnd, plan.tail))
    msz, dh_off = metadata_size(s, R, D), ru(4 + 4 * (R + 1), s)
    for k, sub in enumerate(plan.subs):
        pos = len(out)
        assert pos % max(s, 4) == 0
        arrays = [(a, 2) for a in sub.runs] + [(sub.final, s)]
        body, meta = bytearray(), [0]
        for i, (a, es) in enumerate(arrays):
            blob = _array_bytes(a, es, bool(plan.bp), rnd)
            meta.append(len(blob))
            body += blob
            body += _filler(rnd, ru(len(body), max(s, 4) if i == R - 1 else 4) - len(body))
        meta[0] = ru(msz + len(body), s) + sub.csz_slack
        head = bytearray(_filler(rnd, msz))
        for j, m in enumerate(meta):
            head[4 * j:4 * j + 4] = m.to_bytes(4, "little")
        for j, h in enumerate(sub.heads):
            head[dh_off + j * s:dh_off + (j + 1) * s] = h.to_bytes(s, "little")
        out += head + body
        if k + 1 < len(plan.subs):
            nxt = ru(pos + meta[0] // 4 * 4, s)   # where the decoder looks for the next sub-chunk
        else:
            nxt = pos + meta[0] + plan.tail
            assert (pos + meta[0]) % 4 + plan.tail < 4
        out += _filler(rnd, nxt - len(out))
    return bytes(out)


# ------------------------------------------------------------------------------------------------ building blocks

def _draw(rnd, lo: int, hi: int, without=()) -> int:
    """Uniform in [lo, hi) without the given values."""
    ex = sorted(e for e in set(without) if lo <= e < hi)
    assert hi - lo > len(ex), "nothing left to draw from"
    k = rnd.randrange(lo, hi - len(ex))
    for e in ex:
        if k >= e:
            k += 1
    return k


def ones(rnd, n, room):
    return [1] * n


def spread(fill: bool = False, extra: Optional[int] = None) -> Callable:
    """Run lengths of at least 1: their sum is `room` exactly (fill), or at most n + extra (all of the room by
    default)."""
    def f(rnd, n, room):
        assert n <= room
        if n == 0:
            return []
        top = room if extra is None else min(room, n + extra)
        rem = (room if fill else rnd.randint(n, top)) - n
        c = [1] * n
        while rem > 0:
            a = rnd.randint(1, max(1, rem // 3))
            c[rnd.randrange(n)] += a
            rem -= a
        return c
    return f


def _value_array(rnd, s: int, n: int, need: set, packed: bool, spec: Optional[dict]) -> Arr:
    """The final array: n values fr + r, r below 2^bw ("exact": the first r has bit bw - 1 set and no r is wider;
    "wide": every r is below 2^(bw - 1)); a raw array has no fr and bw of its own, the spec's then only say
    which values to draw.  need: "nonzero": no value is 0; "distinct": a value differs from its neighbour (where
    there are 8 values and more to draw from: from the 6 in front of it, so that runs on both sides of a few empty
    ones differ as well)."""
    M = 1 << (8 * s)
    spec = dict(spec or {})
    bw = spec.get("bw", rnd.randint(2, min(8 * s, 12)) if packed else 8 * s)
    mode = spec.get("mode", "any")
    hi = 1 << (bw - 1) if mode == "wide" else 1 << bw
    if "fr" in spec:
        fr = spec["fr"] % M
    elif not packed and "bw" not in spec:
        fr = 0
    else:   # (no value wraps to 0: fr + r < M, fr > 0 -- at the full width any fr will do, 0's r is left out)
        fr = rnd.randrange(1, M - hi + 1) if M > hi else rnd.randrange(M)
    zero = (-fr) % M
    r: List[int] = []
    for i in range(n):
        without = []
        if "nonzero" in need:
            without.append(zero)
        if "distinct" in need:
            without += r[-6:] if hi >= 8 else r[-1:]
        if mode == "exact" and i == 1 and 0 not in without:
            r.append(0)   # (with the first one: the width is the one the encoder would choose for this fr)
            continue
        lo = hi // 2 if (mode == "exact" and i == 0) else 0
        r.append(_draw(rnd, lo, hi, without))
    return Arr([(fr + x) % M for x in r], fr if packed else 0, bw if packed else 0)


def _head(rnd, x: List[int], M: int, nonzero: bool) -> int:
    """A delta head; nonzero: no sum head + x[0] + .. + x[j] is 0 (the first head from a seeded start that fits:
    fewer than M sums)."""
    h = rnd.randrange(M)
    if nonzero:
        assert len(x) + 1 < M
        acc, bad = 0, {0}
        for v in x:
            acc = (acc + v) % M
            bad.add((-acc) % M)
        while h in bad:
            h = (h + 1) % M
    return h


def minimal_pack(rnd, c: List[int]):
    """(fr, bw) as the encoder chooses them for run lengths."""
    if not c:
        return 0, 0
    return min(c), (max(c) - min(c)).bit_length()


def build_sub(rnd, t: int, R: int, D: int, bp: int, nf: int, lengths: Optional[Dict[int, Callable]] = None,
              final: Optional[dict] = None, packs: Optional[Dict[int, Callable]] = None,
              slack: Optional[Dict[int, int]] = None, csz_slack: int = 0) -> Sub:
    """A sub-chunk from the bottom up: nf final values, then for l = max(R, D) - 1 .. 0 the head of Delta_l and the
    lengths of RLE_l, lengths[l](rnd, runs, room) (default: spread() for l <= D, ones above -- see the module
    docstring) written as packs[l](rnd, lengths) -> (fr, bw) says (default: as the encoder).  slack[i]: of array i
    (the final array is i = R)."""
    s = SIZE[t]
    M, ce = 1 << (8 * s), SUB_CHUNK // s
    ops = [(k, l) for l in range(max(R, D) - 1, -1, -1) for k in "dr" if l < (D if k == "d" else R)]
    # the final values reach the first delta layer through expansions only, and an RLE layer if that comes first
    need = ({"nonzero"} if D else set()) | ({"distinct"} if ops and ops[0][0] == "r" else set())
    fin = _value_array(rnd, s, nf, need, bool(bp), final)
    x = list(fin.values)
    heads, runs = [0] * D, [None] * R
    for kind, l in ops:
        if kind == "d":
            assert len(x) + 1 <= ce
            heads[l] = _head(rnd, x, M, l >= 1)
            acc, y = heads[l], []
            for v in x:
                y.append(acc)
                acc = (acc + v) % M
            x = y + [acc]
        else:
            room = ce - min(l, D)
            c = (lengths or {}).get(l, spread() if l <= D else ones)(rnd, len(x), room)
            assert len(c) == len(x) and sum(c) <= room and all(0 <= v < 65536 for v in c)
            fr, bw = (packs or {}).get(l, minimal_pack)(rnd, c) if bp else (0, 0)
            runs[l] = Arr(c, fr, bw)
            x = [v for cnt, v in zip(c, x) for _ in range(cnt)]
    for i, extra in (slack or {}).items():
        (runs + [fin])[i].slack = extra
    return Sub(heads, runs, fin, csz_slack)


def runs_differ(plan: Plan) -> bool:
    """At every RLE layer of every sub-chunk: a run and the next run that is not empty carry different values, or
    every length of the layer is 1."""
    M = 1 << (8 * plan.size)
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
                c = sub.runs[l].values
                if any(v != 1 for v in c):
                    for i in range(len(c) - 1):
                        j = i + 1
                        while j < len(c) - 1 and c[j] == 0:
                            j += 1
                        if c[j] and x[i] == x[j]:
                            return False
                x = [v for cnt, v in zip(c, x) for _ in range(cnt)]
    return True


def _rnd(family: str, t: int) -> random.Random:
    return random.Random(1000 * FAMILIES.index(family) + t)


def _inner_cap(s: int, D: int) -> Optional[int]:
    """How far the layers l >= 1 may grow a sub-chunk of 1-byte elements when two delta layers stack (a head that
    keeps every sum non-zero exists for fewer than 256 sums)."""
    return 40 if (s == 1 and D >= 2) else None


# ------------------------------------------------------------------------------------------------------ families

def encoder_like(t: int) -> List[Plan]:
    """The shapes the encoder writes: full sub-chunks and a shorter last one, runs of at least 1, the minimal
    bit width, the smallest value as frame of reference, no slack."""
    s, rnd, out = SIZE[t], _rnd("encoder_like", t), []
    ce = SUB_CHUNK // s
    for R, D, bp in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (2, 1, 1), (2, 2, 1), (3, 2, 1),
                     (2, 0, 1), (1, 2, 1), (2, 1, 0)):
        cap = _inner_cap(s, D)
        subs = []
        for k in range(3):
            last = k == 2
            lengths = {l: (spread(extra=cap) if cap is not None else spread()) for l in range(1, min(D, R - 1) + 1)}
            if R:
                lengths[0] = spread(fill=not last)
                nf = rnd.randint(1, 30 if cap is not None else ce // 8)
            else:
                nf = rnd.randint(1, ce // 2) if last else ce - D
                if cap is not None:
                    nf = min(nf, 200)
            mn = None
            if bp:   # the encoder's frame of reference: the smallest value, signed
                bw = rnd.randint(2, min(8 * s, 11))
                mn = dict(bw=bw, mode="exact", fr=rnd.randrange(1, (1 << (8 * s - 1)) - (1 << bw)) if 8 * s - 1 > bw
                          else 1)
            subs.append(build_sub(rnd, t, R, D, bp, nf, lengths, mn))
        out.append(Plan("encoder_like", f"encoder_like/t{t}/R{R}D{D}bp{bp}", t, R, D, bp, subs, seed=rnd.getrandbits(30)))
    return out


ZERO_POSITIONS = ("first", "mod16", "mod64", "last_full", "last_short", "multi", "round64")
ZERO_KINDS = ("raw", "packed12", "packed16")
# (R, D, the layer with the empty runs): R = 1 alone and under a delta layer; R = 2, outer and inner layer, without
# a delta layer and with one fused behind the inner expansion
ZERO_LAYERS = ((1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1))


def _zero_lengths(where: str, ce: int) -> Callable:
    def f(rnd, n, room):
        assert n >= 70
        if where == "first":
            zeros = {0}
        elif where == "mod16":
            zeros = {16 * rnd.randrange(0, (n - 1) // 16) + 15}
        elif where == "mod64":
            zeros = {63}
        elif where in ("last_full", "last_short"):   # (and one in the middle, with a run behind it)
            zeros = {n - 1, 16 * rnd.randrange(1, 4) + rnd.randrange(1, 14)}
        elif where == "multi":
            j = rnd.randrange(1, n - 5)
            zeros = set(range(j, j + rnd.randint(2, 4)))
        else:
            zeros = {63, 64} | ({62, 65} if rnd.randrange(2) else set())
        live = [i for i in range(n) if i not in zeros]
        if where == "last_full":
            assert room == ce
        c = spread(fill=where == "last_full", extra=None if where == "last_full" else 40)(rnd, len(live), room)
        out = [0] * n
        for i, v in zip(live, c):
            out[i] = v
        return out
    return f


def zero_runs(t: int) -> List[Plan]:
    """Runs of length 0 at every position of ZERO_POSITIONS, in every array kind of ZERO_KINDS (raw; bit-packed
    with frame of reference 0 and a width up to 12; the same with a width of 13 .. 16) and every layer of
    ZERO_LAYERS.  (A sub-chunk cannot be full in front of a delta layer: no last_full there.)"""
    s, rnd, out = SIZE[t], _rnd("zero_runs", t), []
    ce = SUB_CHUNK // s
    for R, D, layer in ZERO_LAYERS:
        for kind in ZERO_KINDS:
            for where in ZERO_POSITIONS:
                if where == "last_full" and layer >= 1 and layer - 1 < D:
                    continue
                bp = 0 if kind == "raw" else 1
                lengths = {l: ones for l in range(R)}
                lengths[layer] = _zero_lengths(where, ce)
                if kind == "packed12":
                    packs = {layer: lambda rnd, c: (0, rnd.randint(max(c).bit_length(), 12))}
                else:
                    packs = {layer: lambda rnd, c: (0, rnd.randint(13, 16))}
                # (small values: the sums of a delta layer over a few of them in a row do not wrap to 0)
                small = dict(bw=4, fr=rnd.randrange(1, (1 << (8 * s)) // 8 - 15))
                subs = [build_sub(rnd, t, R, D, bp, rnd.randint(72, 140), lengths, small, packs)
                        for _ in range(rnd.randint(1, 2))]
                out.append(Plan("zero_runs", f"zero_runs/t{t}/R{R}D{D}/layer{layer}/{kind}/{where}", t, R, D, bp, subs,
                                seed=rnd.getrandbits(30)))
    return out


def _width_lengths(bw: int) -> Callable:
    """Run lengths base + r with r below 2^bw: r = 0 and, where the sub-chunk has the room, r = 2^bw - 1 occur."""
    def f(rnd, n, room):
        base = rnd.randint(1, 2)
        c = [base] * n
        rem = room - base * n
        assert rem >= 0 and n >= 2
        top = (1 << bw) - 1
        if top <= rem // 2:
            c[rnd.randrange(1, n)] += top
            rem -= top
        for i in range(1, n):
            a = rnd.randint(0, min(top, rem // 8)) if c[i] == base else 0
            c[i] += a
            rem -= a
        return c
    return f


def widths(t: int) -> List[Plan]:
    """Values at every bit width 0 .. 8 size, exact (an element needs the whole width) and wider than the data
    needs, a few and many elements; run lengths at every width 0 .. 16 (frame of reference: the smallest length)."""
    s, rnd, out = SIZE[t], _rnd("widths", t), []
    ce = SUB_CHUNK // s
    shapes = ((0, 0), (0, 1), (1, 0), (1, 1))
    k = 0
    for bw in range(8 * s + 1):
        for mode in ("exact", "wide") if bw else ("exact",):
            for big in (False, True):
                R, D = shapes[k % 4]
                k += 1
                if R > D and (1 << bw if mode == "exact" else 1 << (bw - 1)) < 2:
                    D = 1   # (one value only: no unequal neighbours to put under an RLE layer)
                nf = rnd.randint(ce // 2, ce - 1 - D) if big else rnd.randint(1, 70)
                lengths = {0: spread(extra=ce - nf - 1 if big else 100)}
                sub = build_sub(rnd, t, R, D, 1, nf, lengths, dict(bw=bw, mode=mode))
                out.append(Plan("widths", f"widths/t{t}/values/bw{bw}/{mode}/n{nf}/R{R}D{D}", t, R, D, 1, [sub],
                                seed=rnd.getrandbits(30)))
    for bw in range(17):
        for D in (0, 1):
            nf = rnd.randint(20, 60) if bw > 4 else rnd.randint(70, 200)
            packs = {0: lambda rnd, c, bw=bw: (min(c), bw)}
            sub = build_sub(rnd, t, 1, D, 1, min(nf, ce // 4), {0: _width_lengths(bw)}, None, packs)
            out.append(Plan("widths", f"widths/t{t}/lengths/bw{bw}/D{D}", t, 1, D, 1, [sub], seed=rnd.getrandbits(30)))
    return out


def frames_of_reference(t: int) -> List[Plan]:
    """Frames of reference an encoder would not choose.  Values: fr + r wraps the element's width for some
    elements (fr is negative for the signed types).  Run lengths: fr + 2^bw - 1 > 0xFFFF with no length that wraps
    16 bits (bw = 16, fr up to the smallest length), with every length wrapping (fr just below 2^16) and with some."""
    s, rnd, out = SIZE[t], _rnd("frames_of_reference", t), []
    M = 1 << (8 * s)
    for bw in sorted({3, 4 * s, 8 * s - 1, 8 * s}):
        for R, D in ((0, 0), (1, 0), (1, 1), (0, 2)):
            fr = M - rnd.randint(1, max(1, (1 << bw) // 2 - 1))   # (with r = 2^bw - 1 first: that one wraps)
            sub = build_sub(rnd, t, R, D, 1, rnd.randint(20, 90), None, dict(bw=bw, mode="exact", fr=fr))
            out.append(Plan("frames_of_reference", f"frames_of_reference/t{t}/values/bw{bw}/R{R}D{D}", t, R, D, 1, [sub],
                            seed=rnd.getrandbits(30)))

    def lengths_from(lo):
        return lambda rnd, n, room: [rnd.randint(lo, lo + 5) for _ in range(n)]
    cases = (
        ("nowrap", lengths_from(2), lambda rnd, c: (rnd.randint(1, min(c)), 16)),
        ("allwrap16", lengths_from(1), lambda rnd, c: (65536 - rnd.randint(1, 60000), 16)),
        ("allwrap12", lengths_from(1), lambda rnd, c: (65536 - rnd.randint(1, 4000), 12)),
        ("allwrap5", lengths_from(1), lambda rnd, c: (65536 - rnd.randint(1, 25), 5)),
        ("allwrap14", lengths_from(1), lambda rnd, c: (65536 - rnd.randint(1, 16000), 14)),
        ("somewrap", lambda rnd, n, room: [3 * (i % 2) + rnd.randint(i % 2 ^ 1, 2) for i in range(n)],
         lambda rnd, c: (3, 16)),
    )
    for name, lens, pack in cases:
        for R, D, layer in ((1, 0, 0), (1, 1, 0), (2, 1, 1)):
            lengths = {l: ones for l in range(R)}
            lengths[layer] = lens
            sub = build_sub(rnd, t, R, D, 1, rnd.randint(30, 60), lengths, None, {layer: pack})
            out.append(Plan("frames_of_reference", f"frames_of_reference/t{t}/lengths/{name}/R{R}D{D}", t, R, D, 1, [sub],
                            seed=rnd.getrandbits(30)))
    return out


def placement(t: int) -> List[Plan]:
    """The final array and a run-length array inside the first 1 KiB of the sub-chunk, across its end and behind
    it; a run-length array of more than 1 KiB; slack in meta[] lengths; slack in the size word, no multiple of 4."""
    s, rnd, out = SIZE[t], _rnd("placement", t), []
    ce = SUB_CHUNK // s

    def add(name, R, D, bp, *subs, tail=0):
        out.append(Plan("placement", f"placement/t{t}/{name}", t, R, D, bp, list(subs), tail=tail, seed=rnd.getrandbits(30)))
    big = min(ce - 2, 1600 // s + 16)   # elements of a final array that crosses 1 KiB
    for bp in (0, 1):
        wide = dict(bw=8 * s - 1) if bp else None
        # the final array: inside, across, behind (a run-length array of 1 KiB and more in front of it)
        add(f"final/inside/bp{bp}", 1, 1, bp, build_sub(rnd, t, 1, 1, bp, 40))
        add(f"final/straddle/bp{bp}", 0, 1, bp, build_sub(rnd, t, 0, 1, bp, big, None, wide))
        add(f"final/rle/bp{bp}", 1, 0, bp, build_sub(rnd, t, 1, 0, bp, big, {0: spread(extra=30)}, wide))
        add(f"final/behind/bp{bp}", 1, 0, bp, build_sub(rnd, t, 1, 0, bp, min(ce, 600), {0: ones},
                                                        packs={0: lambda rnd, c: (0, 16)}))
        # a run-length array: inside (above), across, behind, larger than 1 KiB
        add(f"lengths/straddle/bp{bp}", 2, 1, bp, build_sub(rnd, t, 2, 1, bp, 480 // (1 + bp), {0: ones, 1: spread(extra=20)},
                                                            slack={0: 900} if bp else None))
        add(f"lengths/large/bp{bp}", 1, 0, bp, build_sub(rnd, t, 1, 0, bp, min(ce, 700), {0: spread(extra=60)},
                                                         packs={0: lambda rnd, c: (0, 16)}, slack={0: 1 - bp}), tail=3 * bp)
    # bit-packed arrays with slack: a large one pushes what follows behind 1 KiB
    add("lengths/behind/slack", 2, 1, 1, build_sub(rnd, t, 2, 1, 1, 50, {0: spread(extra=30), 1: spread(extra=30)},
                                                   slack={0: 1100, 1: 7, 2: 5}))
    add("lengths/large/slack", 2, 2, 1, build_sub(rnd, t, 2, 2, 1, 30, {0: spread(extra=30), 1: spread(extra=9)},
                                                  slack={1: 1500, 2: 1030}))
    add("final/behind/slack", 1, 0, 1, build_sub(rnd, t, 1, 0, 1, 300 // s, {0: spread(extra=50)}, slack={0: 1020, 1: 3}))
    for k, cs in enumerate((1, 2, 3, 5, 4 * s + 2, 1027)):
        subs = [build_sub(rnd, t, 1, 1, k % 2, rnd.randint(5, 60), slack={1: min(cs, s - 1)} if k % 2 == 0 else {0: cs, 1: cs},
                          csz_slack=cs + 4 * j) for j in range(3)]
        add(f"csz_slack{cs}", 1, 1, k % 2, *subs, tail=3 - (subs[-1].csz_slack % 4))
    if s > 1:   # a raw array whose length is no multiple of its element size
        add("raw_slack", 1, 1, 0, build_sub(rnd, t, 1, 1, 0, 33, slack={0: 1, 1: s - 1}),
            build_sub(rnd, t, 1, 1, 0, 18, slack={0: 1, 1: 1}))
    return out


def ragged(t: int) -> List[Plan]:
    """Sub-chunks of 0, 1, E - 1 and E elements (E: the elements a lane holds, 16 or 8) in every order of a
    partition; many tiny sub-chunks; empty bit-packed arrays with arbitrary frame of reference and width bytes; a
    delta layer over an empty final array; a delta layer that lands exactly on a full sub-chunk; a partition of
    no sub-chunk at all."""
    s, rnd, out = SIZE[t], _rnd("ragged", t), []
    M, ce, E = 1 << (8 * s), SUB_CHUNK // s, 8 if s == 8 else 16

    def exactly(total):   # run lengths that sum to `total`
        return lambda rnd, n, room: spread(fill=True)(rnd, n, total)

    def sized(R, D, bp, total):
        if total == 0:
            sub = build_sub(rnd, t, R, D, bp, 0)
        elif R == 0:
            sub = build_sub(rnd, t, R, D, bp, total - D)
        else:   # (the runs of layer 0: 1 .. total of them, D of which come from the delta heads)
            n0 = rnd.randint(1 + min(D, 1), total) if total > 1 else 1
            sub = build_sub(rnd, t, R, D, bp, max(n0 - D, 0), {0: exactly(total), 1: ones})
        if bp and not sub.final.values:   # an empty bit-packed array: its header bytes are don't-care
            sub.final.fr, sub.final.bw = rnd.randrange(M), rnd.choice((0, 1, 8 * s, 8 * s + 1, 0xFFFF))
            for a in sub.runs:
                if not a.values:
                    a.fr, a.bw = rnd.randrange(65536), rnd.choice((0, 16, 17, 0xFFFF))
        return sub
    orders = ((0, 1, E - 1, E), (E, E - 1, 1, 0), (1, 0, E, E - 1), (E - 1, E, 0, 1), (0, 0, E, 0), (E, 0, 0, 1))
    for R, D, bp in ((1, 0, 0), (1, 0, 1), (0, 0, 1), (2, 0, 1), (1, 1, 1), (0, 1, 0), (2, 1, 1)):
        for k, order in enumerate(orders):
            if D and R == 0:
                order = tuple(max(v, D) for v in order)
            elif D:   # (layer 0 holds a run for the head of Delta_0: an output of 0 elements is a run of length 0)
                order = tuple(max(v, 1) for v in order)
            subs = [sized(R, D, bp, v) for v in order]
            out.append(Plan("ragged", f"ragged/t{t}/R{R}D{D}bp{bp}/order{k}", t, R, D, bp, subs, seed=rnd.getrandbits(30)))
        tiny = [sized(R, D, bp, rnd.randint(max(D, 1), 3)) for _ in range(4)]
        out.append(Plan("ragged", f"ragged/t{t}/R{R}D{D}bp{bp}/tiny", t, R, D, bp, tiny, seed=rnd.getrandbits(30)))
    for bp in (0, 1):
        for R in (0, 1, 2):
            # a delta layer over an empty final array: one element out (R: one run per layer on top of it)
            subs = [build_sub(rnd, t, R, 1 if R < 2 else 2, bp, 0) for _ in range(2)]
            for sub in subs:
                if bp:
                    sub.final.fr, sub.final.bw = rnd.randrange(M), rnd.choice((3, 8 * s, 0x7FFF))
            DD = 1 if R < 2 else 2
            out.append(Plan("ragged", f"ragged/t{t}/delta_over_empty/R{R}D{DD}bp{bp}", t, R, DD, bp, subs,
                            seed=rnd.getrandbits(30)))
        # a delta layer that lands exactly on a full sub-chunk, alone and fused behind an expansion
        out.append(Plan("ragged", f"ragged/t{t}/delta_to_full/R0D1bp{bp}", t, 0, 1, bp,
                        [build_sub(rnd, t, 0, 1, bp, ce - 1), build_sub(rnd, t, 0, 1, bp, 3)], seed=rnd.getrandbits(30)))
        out.append(Plan("ragged", f"ragged/t{t}/delta_to_full/R2D1bp{bp}", t, 2, 1, bp,
                        [build_sub(rnd, t, 2, 1, bp, 60, {0: ones, 1: exactly(ce - 1)})], seed=rnd.getrandbits(30)))
        out.append(Plan("ragged", f"ragged/t{t}/empty_partition/bp{bp}", t, 1, bp, bp, [], seed=rnd.getrandbits(30)))
        out.append(Plan("ragged", f"ragged/t{t}/empty_sub_chunks/bp{bp}", t, 1, 0, bp,
                        [sized(1, 0, bp, 0), sized(1, 0, bp, 0)], seed=rnd.getrandbits(30)))
    return out


def depth_shapes(s: int):
    """(R, D) for R = 0 .. 7: every D whose metadata block is exactly the 64 bytes the decoder allows, and the
    largest D whose block is smaller."""
    out = []
    for R in range(8):
        fits = [D for D in range(0, 64) if metadata_size(s, R, D) <= 64 and (R, D) != (0, 0)]
        full = [D for D in fits if metadata_size(s, R, D) == 64]
        below = [D for D in fits if metadata_size(s, R, D) < 64]
        out += [(R, D) for D in full] + ([(R, max(below))] if below else [])
    return out


def depth(t: int) -> List[Plan]:
    """Every shape of depth_shapes() and the smaller ones that bring D > R, R > D, D alone and R = 7 alone; small
    sub-chunks (each layer adds a few elements)."""
    s, rnd, out = SIZE[t], _rnd("depth", t), []
    shapes = depth_shapes(s) + [(7, 0), (7, 1), (3, 5), (5, 3), (0, 3), (4, 4), (1, 3)]
    for k, (R, D) in enumerate(sorted(set(shapes))):
        bp = k % 2
        lengths = {l: spread(extra=3) for l in range(0, min(D, R - 1) + 1)}
        subs = [build_sub(rnd, t, R, D, bp, rnd.randint(2, 9), lengths) for _ in range(2)]
        out.append(Plan("depth", f"depth/t{t}/R{R}D{D}bp{bp}", t, R, D, bp, subs, seed=rnd.getrandbits(30)))
    return out


def raw(t: int) -> List[Plan]:
    """R = D = bp = 0: the data as it is, with bytes behind it."""
    s, rnd, out = SIZE[t], _rnd("raw", t), []
    for n, tail in ((0, 0), (0, 5), (1, 1), (3, 2), (100, 3), (4096 // s + 1, 64), (10000 // s, 7)):
        data = bytes(rnd.getrandbits(8) for _ in range(n * s))
        out.append(Plan("raw", f"raw/t{t}/n{n}/tail{tail}", t, 0, 0, 0, raw=data, tail=tail, seed=rnd.getrandbits(30)))
    return out


@functools.lru_cache(maxsize=None)
def family(name: str):
    """-> (Plan, ...) of a family over all eight types."""
    return tuple(p for t in range(8) for p in globals()[name](t))


@functools.lru_cache(maxsize=None)
def corpus():
    """-> ((plan, stream, expected bytes), ...) of every family."""
    return tuple((p, encode(p), expected(p)) for name in FAMILIES for p in family(name))
