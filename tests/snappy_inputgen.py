"""Planned INPUTS for the Snappy encoder (plain Python and numpy, no GPU, nothing from the kernel sources).

tests/streamgen.py writes streams for the decoders; this module writes inputs for the encoder, each from an explicit
plan: steps (k literal bytes, a copy of L bytes from a chosen earlier position).  A case carries the element list
the plan intends -- ("L", n) and ("C", length, distance), in stream order -- and tests/test_snappy_inputgen_cpu.py
asserts that the oracle's stream of the case has exactly those elements, for every case.

What makes the outcome known by construction (the rules are those of oracle/snappy_oracle.c):
  * hash: snap_hash(v) = ((v * 0x102A6B) & 0xFFFFFFFF) >> 20, a 12-bit slot per 4-byte word;
  * literal bytes are chosen one at a time so that every word that starts in a literal occurs nowhere earlier in
    the chunk (no match the plan did not ask for) and, in a chunk of up to ~3.4 KiB, has a slot no other word of
    the chunk has (in longer chunks: none of the 130 words before it) -- so no two lanes of a window share a slot
    unless the plan says so.  Where the plan asks for sharing, two free bytes are enumerated (65 536 values, numpy)
    and the first value that meets the constraints is taken; there being none raises;
  * a search posts into the hash map the lanes up to and including its hit, and of a 64-byte window without a hit
    lane 0 only; positions inside a copy are never posted.  The builder keeps that map (`posted`) for one purpose:
    to assert, when a copy is planted, that the candidate the encoder will look at is the planned source;
  * a planted copy is followed by a byte that differs from the one behind its source: its length is exactly L;
  * a copy of 16 bytes or more ends a trip of the encoder's straight path, whose next window starts at the copy's
    end: reset() plants one (20 bytes, from the 24-byte pool at the head of the chunk or its latest copy), so the
    lanes of what follows count from there.  At the head of a chunk lanes count from 0 without it.

finish() verifies the uniqueness claim over the whole chunk with numpy and raises PlanError if it does not hold;
a family then builds the case again with the next salt of its seed (deterministic).
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
RESET_LEN = 20
POOL = 24
TAIL = 160          # literal bytes behind a planted situation: the straight path needs 144 ahead of a window
SMALL = 3500        # up to here every word of a chunk has a slot of its own


def snap_hash(v: int) -> int:
    return ((v * 0x102A6B) & M32) >> 20


def _hash_np(w: np.ndarray) -> np.ndarray:
    return ((w.astype(np.uint64) * np.uint64(0x102A6B)) & np.uint64(M32)) >> np.uint64(20)


class PlanError(Exception):
    pass


class NotRelocatable(Exception):
    pass


class Plan(list):
    """The planned elements of a case; `tags` say which listed parameter values the case holds (the census)."""

    def __init__(self, elems=(), tags=None):
        super().__init__(elems)
        self.tags = dict(tags or {})


class Chunk:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.buf = bytearray()
        self.is_lit = bytearray()
        self.slot_at = []          # slot of the word at every position that has one
        self.words = set()
        self.used = set()
        self.posted = {}           # slot -> position, as the encoder's hash map holds it (16 bits of it)
        self.pos0 = 0              # where the search that is being laid out started
        self.forbid = None         # the next byte must differ from this one
        self.exempt = set()        # literal positions whose word is planned to occur earlier (and not to be found)
        self.elems = []
        self.reset_last = None
        self.tags = {}
        self.wlog, self.ulog = [], []   # words / slots in the order they were first seen (rollback)
        self.composing = False     # several situations in one chunk (composed): finish() only notes the name
        self.sits = []

    # ---------------------------------------------------------------- bytes
    def __len__(self):
        return len(self.buf)

    def word(self, i):
        return int.from_bytes(self.buf[i:i + 4], "little")

    def slot(self, i):
        return snap_hash(self.word(i))

    def _put(self, b, lit):
        self.buf.append(b)
        self.is_lit.append(1 if lit else 0)
        self.forbid = None
        if len(self.buf) >= 4:
            w = self.word(len(self.buf) - 4)
            s = snap_hash(w)
            self.slot_at.append(s)
            self._see(w, s)

    def _see(self, w, s):
        if w not in self.words:
            self.words.add(w)
            self.wlog.append(w)
        if s not in self.used:
            self.used.add(s)
            self.ulog.append(s)

    def mark(self):
        return (len(self.buf), len(self.slot_at), len(self.elems), self.pos0, self.forbid, self.reset_last,
                dict(self.posted), set(self.exempt), len(self.wlog), len(self.ulog), len(self.sits))

    def rollback(self, m):
        n, ns, ne, self.pos0, self.forbid, self.reset_last, self.posted, self.exempt, nw, nu, nt = m
        del self.buf[n:], self.is_lit[n:], self.slot_at[ns:], self.elems[ne:], self.sits[nt:]
        self.words.difference_update(self.wlog[nw:])
        self.used.difference_update(self.ulog[nu:])
        del self.wlog[nw:], self.ulog[nu:]

    def _avoid(self):
        return self.used if len(self.buf) < SMALL else set(self.slot_at[-130:])

    def _choose(self):
        """One literal byte: the word it completes is new and has a slot of its own."""
        n = len(self.buf)
        if n < 3:
            for b in self.rng.permutation(256).tolist():
                if b != self.forbid:
                    return self._put(b, True)
        base = int.from_bytes(self.buf[n - 3:n], "little")
        avoid = self._avoid()
        for b in self.rng.permutation(256).tolist():
            w = base | (b << 24)
            if b != self.forbid and w not in self.words and snap_hash(w) not in avoid:
                return self._put(b, True)
        raise PlanError("no byte completes a new word with a slot of its own")

    def _choose_pair(self, target, differ_from):
        """Two literal bytes at n, n + 1 so that the word at n - 2 has slot `target` (and is new and is not
        `differ_from`), and the word at n - 3, which the first of them completes, is new with a slot of its own."""
        n = len(self.buf)
        assert n >= 3
        b2, b3 = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64), indexing="ij")
        lo = np.uint64(int.from_bytes(self.buf[n - 2:n], "little"))
        wx = lo | (b2 << np.uint64(16)) | (b3 << np.uint64(24))
        wprev = np.uint64(int.from_bytes(self.buf[n - 3:n], "little")) | (b2 << np.uint64(24))
        ok = (_hash_np(wx) == np.uint64(target)) & (wx != np.uint64(differ_from))
        avoid = np.fromiter(self._avoid(), dtype=np.uint64) if self._avoid() else np.zeros(0, np.uint64)
        ok &= ~np.isin(_hash_np(wprev), avoid)
        if self.forbid is not None:
            ok &= b2 != np.uint64(self.forbid)
        for i in np.flatnonzero(ok.ravel()).tolist():
            x, y = divmod(i, 256)
            if int(wx[x, y]) not in self.words and int(wprev[x, y]) not in self.words:
                self._put(x, True)
                self._put(y, True)
                return
        raise PlanError("no two bytes give the planned shared slot")

    def _roll(self):
        """A search without a hit ends after 256 literal bytes: lane 0 of each of its four windows is posted."""
        while len(self.buf) - self.pos0 >= 256 + 3:      # (the words of the posted lanes are complete)
            self._close_256()

    def _close_256(self):
        for p in range(self.pos0, self.pos0 + 256, 64):
            self.posted[self.slot(p)] = p
        self.elems.append(("L", 256))
        self.pos0 += 256

    def lit(self, k, share=None):
        """k literal bytes.  share: {b: a or ("slot", s)} with b, a offsets from the start of this stretch (a may be
        negative: an earlier position) -- the word at b gets the slot of the word at a, and differs from it."""
        start = len(self.buf)
        share = dict(share or {})
        j = 0
        while j < k:
            x = start + j - 2                        # the word whose last two bytes come next
            if (x - start) in share and j + 1 < k:
                a = share[x - start]
                if isinstance(a, tuple):
                    self._choose_pair(a[1], 1 << 40)
                else:
                    self._choose_pair(self.slot(start + a), self.word(start + a))
                j += 2
            else:
                self._choose()
                j += 1
            self._roll()
        return start

    def bulk(self, n):
        """n literal bytes at numpy speed: random, then every byte that completes a word seen earlier drawn again."""
        start = len(self.buf)
        new = self.rng.integers(0, 256, n, dtype=np.uint8)
        if self.forbid is not None and n and new[0] == self.forbid:
            new[0] ^= 0x55
        old = np.frombuffer(bytes(self.buf), dtype=np.uint8)
        for _ in range(64):
            a = np.concatenate([old, new]).astype(np.uint32)
            w = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
            _, first = np.unique(w, return_index=True)
            dup = np.ones(len(w), dtype=bool)
            dup[first] = False
            dup[:max(start - 3, 0)] = False
            at = np.flatnonzero(dup) + 3 - start     # the byte that completes the repeated word
            at = at[at >= (1 if self.forbid is not None else 0)]
            if at.size == 0:
                break
            new[at] = self.rng.integers(0, 256, at.size, dtype=np.uint8)
        else:
            raise PlanError("bulk literals keep repeating a word")
        self.buf += new.tobytes()
        self.is_lit += b"\x01" * n
        self.forbid = None
        a = np.frombuffer(bytes(self.buf), dtype=np.uint8).astype(np.uint32)
        w = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
        lo = len(self.slot_at)
        slots = _hash_np(w[lo:]).astype(np.int64).tolist()
        self.slot_at += slots
        for wi in w[lo:].tolist():
            if wi not in self.words:
                self.words.add(wi)
                self.wlog.append(wi)
        self._roll()
        return start

    # ---------------------------------------------------------------- the hash map, for the assert in copy()
    def candidate(self, p, slot):
        """The position a window at p reads out of `slot`: the 16 stored bits put below p (None: nothing there)."""
        v = self.posted.get(slot, 0) & 0xFFFF
        t = (p & ~0xFFFF) | v
        if t >= p:
            if t < 0x10000:
                return None
            t -= 0x10000
        return t

    def would_find(self, q, lane0):
        """What the search whose window starts at lane0 finds for the word at q (a source position or None), given
        that the lanes lane0 .. q - 1 did not hit."""
        s, w = self.slot(q), self.word(q)
        lower = [x for x in range(lane0, q) if self.slot_at[x] == s]
        if lower and self.word(lower[-1]) == w:
            return lower[-1]
        t = self.candidate(lane0, s)
        if t is not None and t + 32768 >= q and self.word(t) == w:
            return t
        return None

    def copy(self, L, src):
        """A copy of L <= 64 bytes from position src, at the end of the k literal bytes laid since the last element:
        the planned element(s) ("L", k), ("C", L, distance)."""
        q = len(self.buf)
        assert 4 <= L <= 64 and 0 <= src < q
        while q - self.pos0 >= 256:
            self._close_256()
        if self.forbid is not None and self.buf[src] == self.forbid:
            raise PlanError("the copy's first byte is the one that has to differ")
        head = []                                    # the literal words the copy's first bytes complete: new ones
        for i in range(3):
            head.append(self.buf[src + i] if src + i < q else head[src + i - q])
        for i in (1, 2, 3):
            if q - i >= 0 and self.is_lit[q - i] and q - i not in self.exempt \
                    and int.from_bytes(bytes(self.buf[q - i:q]) + bytes(head[:4 - i]), "little") in self.words:
                raise PlanError("a literal word that the copy completes occurs earlier")
        for i in range(L):
            self._put(self.buf[src + i], False)
        k = q - self.pos0
        lane0 = self.pos0 + k // 64 * 64
        for p in range(self.pos0, lane0, 64):        # the windows without a hit in front of it
            self.posted[self.slot(p)] = p
        found = self.would_find(q, lane0)
        if found != src:
            raise PlanError(f"the copy at {q} would find {found}, planned {src}")
        for x in range(lane0, q + 1):
            self.posted[self.slot_at[x]] = x
        if k:
            self.elems.append(("L", k))
        self.elems.append(("C", L, q - src))
        self.pos0 = q + L
        self.forbid = self.buf[src + L]
        return q

    def not_found(self, n, src, exempt=True):
        """n >= 4 literal bytes equal to those at src, which the plan says the encoder does NOT find."""
        q = len(self.buf)
        if self.forbid is not None and self.buf[src] == self.forbid:
            raise PlanError("first byte has to differ")
        for i in range(n):
            self._put(self.buf[src + i], True)
            self.exempt.add(q + i)
        self.forbid = self.buf[src + n]
        self._roll()
        return q

    def reset(self):
        """A 20-byte copy of the pool: ends the trip, the next one starts at its end."""
        if self.reset_last is None:
            assert len(self.buf) >= POOL
            src = 0
        else:
            src = self.reset_last
        q = self.copy(RESET_LEN, src)
        self.reset_last = q
        return q + RESET_LEN

    def next_lane0(self):
        """The next position at or behind the end that is lane 0 of a window if no hit comes before it."""
        return self.pos0 + (len(self.buf) - self.pos0 + 63) // 64 * 64

    def finish(self, name, tail=0):
        if self.composing:
            self.sits.append(name)
            return None
        if tail:
            self.lit(tail)
        n = len(self.buf)
        rest = n - self.pos0
        while rest > 0:
            self.elems.append(("L", min(rest, 256)))
            rest -= min(rest, 256)
        if n >= 5:
            a = np.frombuffer(bytes(self.buf), dtype=np.uint8).astype(np.uint32)
            w = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
            _, first = np.unique(w, return_index=True)
            rep = np.ones(len(w), dtype=bool)
            rep[first] = False
            rep &= np.frombuffer(bytes(self.is_lit), dtype=np.uint8)[:len(w)] == 1
            if self.exempt:
                ex = np.array([x for x in self.exempt if x < len(w)], dtype=np.int64)
                rep[ex] = False
            if rep.any():
                raise PlanError(f"{name}: a literal word at {int(np.flatnonzero(rep)[0])} occurs earlier")
        return name, bytes(self.buf), Plan(self.elems, self.tags)


_collect = None     # composed(): the families' recipes (seed, fn) instead of their cases


def _build(seed, fn, tries=40):
    """fn(Chunk) -> case, with the next salt of the seed whenever the plan cannot be laid out."""
    if _collect is not None:
        _collect.append(fn)
        return None
    err = None
    for salt in range(tries):
        try:
            return fn(Chunk([seed, salt]))
        except PlanError as e:
            err = e
    raise PlanError(f"no layout in {tries} salts: {err}")


def _head_for(c, k, D, L):
    """Literals from the start of the search under way (the head of the chunk, pool included, or the end of a copy)
    of such a length that, after a reset and k literals, the position D back is a posted one: lane 0 of a window
    of a stretch without a hit.  -> the source position."""
    base, done = c.pos0, len(c.buf) - c.pos0
    j = 1
    while True:
        n = 64 * j + D - RESET_LEN - k
        if n >= 64 * j + L + 8 + 192 and 64 * j >= done:
            break
        j += 1
    (c.bulk if n - done > 4000 else c.lit)(n - done)
    if n > 30000:                                     # the pool is out of reach: a posted one near the reset
        c.reset_last = base + (n - 30) // 64 * 64
    return base + 64 * j


# ----------------------------------------------------------------------------------------- hit_lane_by_length

HIT_LANES = (0, 1, 7, 8, 9, 47, 48, 49, 50, 51, 52, 53, 54, 55, 59, 60, 63)
HIT_LENGTHS = (4, 5, 11, 12, 15, 16, 17, 19, 20, 63, 64, 65, 67, 68, 100, 300)
HIT_DISTANCES = (1, 2, 3, 4, 5, 15, 16, 17, 2047, 2048, 32767, 32768)
NO_HIT_DISTANCES = (32769, 40000)


def _long_copy(c, L, src, local_period=0):
    """A match of L bytes as the encoder takes it: 64 at a time.  From a stretch of posted multiples of 64 every
    piece has the same distance; a run of period D (D divides 64) is found 64 back from the second piece on.
    Fewer than 4 bytes left over are literals of the next element."""
    q = c.copy(min(L, 64), src)
    done = min(L, 64)
    while L - done >= 4:
        n = min(L - done, 64)
        c.forbid = None                               # (the match goes on)
        c.copy(n, q + done - 64 if local_period else src + done)
        done += n
    if L - done:                                      # 1 .. 3 bytes of the match left: literals
        s = (q + done - 64) if local_period else (src + done)
        at = len(c.buf)
        c.forbid = None
        for i in range(L - done):
            c._put(c.buf[s + i], True)
        c.forbid = c.buf[s + L - done]
        c.exempt.update(range(at - 3, at + L - done))   # (their words are cut short by the byte that differs)


def _hit_case(seed, k, L, D):
    def fn(c):
        c.tags = {"lane": k, "L": L, "D": D}
        if D <= 17:                                   # the source is a literal lane of the same window
            assert k >= D
            c.lit(POOL + 16)
            c.reset()
            c.lit(k)
            _long_copy(c, L, len(c.buf) - D, local_period=D)
        else:
            src = _head_for(c, k, D, L)
            c.reset()
            c.lit(k)
            _long_copy(c, L, src)
        return c.finish(f"hit/lane{k}_L{L}_D{D}", TAIL)
    return _build(seed, fn)


def hit_lane_by_length(seed=1):
    far = [d for d in HIT_DISTANCES if d > 17]
    near = [d for d in HIT_DISTANCES if d <= 17]
    combos = []

    def add(i, k, L, D=None):
        if D is None:
            D = (near + far)[i % len(HIT_DISTANCES)]
        if D <= 17 and (k < D or (L > 64 and 64 % D)):
            D = far[i % len(far)]
        combos.append((k, L, D))
    for i, k in enumerate(HIT_LANES):
        add(i, k, HIT_LENGTHS[i % len(HIT_LENGTHS)])
        add(i + 5, k, HIT_LENGTHS[(3 * i + 7) % len(HIT_LENGTHS)])
    for i, L in enumerate(HIT_LENGTHS):
        add(i + 3, HIT_LANES[(5 * i + 2) % len(HIT_LANES)], L)
        add(i, 47 + i % 9, L, near[i % len(near)] if L <= 64 or 64 % near[i % len(near)] == 0 else 16)
    for i, D in enumerate(HIT_DISTANCES):
        for j in range(2):
            k = HIT_LANES[(7 * i + 3 * j + 4) % len(HIT_LANES)]
            if D <= 17 and k < D:
                k = 47 + (i + j) % 9
            add(i, k, (5, 11, 12, 15, 16, 20, 64)[(i + 3 * j) % 7], D)
    cases = [_hit_case([seed, n], *kld) for n, kld in enumerate(dict.fromkeys(combos))]

    def none(c, k, D):                                # a word again, too far back: literals
        c.tags = {"lane": k, "no_hit_D": D}
        src = _head_for(c, k, D, 12)
        c.reset()
        c.lit(k)
        c.not_found(12, src)
        return c.finish(f"hit/lane{k}_none_D{D}", TAIL)
    for n, D in enumerate(NO_HIT_DISTANCES):
        for k in (0, 9, 51):
            cases.append(_build([seed, 900 + n, k], lambda c, k=k, D=D: none(c, k, D)))
    return cases


# ------------------------------------------------------------------------------------------------------ trips

TRIP_SUMS = (51, 52, 53, 63, 64, 65, 66)


def _sources(c, n, far=0):
    """A head whose multiples of 64 (posted: lane 0 of windows without a hit) serve as sources, one per short copy:
    -> n positions less than 2048 bytes in front of where they are used; with far: (those, `far` positions more
    than 2048 bytes in front: three-byte copy elements whatever the length)."""
    far_srcs = []
    if far:
        s0 = c.next_lane0()
        c.lit(s0 - len(c.buf) + 64 * (far + 1))
        far_srcs = [s0 + 64 * (j + 1) for j in range(far)]
        c.lit(2048)
    base = c.next_lane0()
    c.lit(base - len(c.buf) + 64 * (n + 1) + 20)
    near = [base + 64 * (j + 1) for j in range(n)]
    return (near, far_srcs) if far else near


def _trip_case(seed, name, steps, end=None, far=()):
    """steps: [(k, L)] short elements of one trip behind a reset; end: (k, L >= 16) closes the trip."""
    def fn(c):
        n = len(steps) + (2 + end[1] // 64 if end else 0)   # (the long match's source: a stretch of its own)
        near_srcs, far_srcs = _sources(c, n, len(far)) if far else (_sources(c, n), [])
        c.reset()
        lane = 0
        sums = []
        twos = threes = 0
        for i, (k, L) in enumerate(steps):
            c.lit(k)
            src = far_srcs.pop() if i in far else near_srcs.pop()
            q = c.copy(L, src)
            if L < 12 and q - src < 2048:
                twos += 1
            else:
                threes += 1
            lane += k + L
            sums.append(lane)
        if end:
            c.lit(end[0])
            _long_copy(c, end[1], near_srcs[0])
        c.tags = {"elements": len(steps), "sums": sums, "k0_chain": sum(1 for k, _ in steps[1:] if k == 0),
                  "twos": twos, "threes": threes, "ended_after": len(steps) if end else None}
        return c.finish(name, TAIL)
    return _build(seed, fn)


def trips(seed=2):
    rng = np.random.default_rng([seed, 77])
    cases = []
    n = 0
    for total in TRIP_SUMS:                           # the last short element ends exactly at lane `total`
        for count in (2, 5, 9, 12):
            if count * 4 > total:
                continue
            Ls = rng.integers(4, 16, count)
            while int(Ls.sum()) > total:              # (shorter copies until they fit)
                i = int(rng.integers(0, count))
                Ls[i] = max(4, Ls[i] - 1)
            room = total - int(Ls.sum())
            cuts = np.sort(rng.integers(0, room + 1, count - 1)) if room else np.zeros(count - 1, int)
            ks = np.diff(np.concatenate([[0], cuts, [room]])).tolist()
            steps = list(zip(ks, Ls.tolist()))
            far = tuple(i for i in range(count) if (i + n) % 3 == 0)
            cases.append(_trip_case([seed, n], f"trips/sum{total}_n{count}", steps, far=far))
            n += 1
    cases.append(_trip_case([seed, 200], "trips/chain_k0", [(3, 4), (0, 5), (0, 11), (0, 12), (0, 15), (0, 4)]))
    cases.append(_trip_case([seed, 201], "trips/chain_k0_far", [(0, 4), (0, 11), (0, 12), (2, 7)], far=(1, 3)))
    for after, steps in ((0, []), (1, [(6, 9)]), (4, [(2, 5), (0, 12), (9, 15), (1, 4)])):
        for L in (16, 40, 64, 100):
            cases.append(_trip_case([seed, 300 + after, L], f"trips/ended_after{after}_L{L}", steps, end=(3, L)))
    return cases


# ---------------------------------------------------------------------------------------------- shared_hashes

def shared_hashes(seed=3):
    cases = []

    def add(name, fn, n):
        cases.append(_build([seed, n], lambda c: (fn(c), c.tags.setdefault("layout", name.split("/")[1]),
                                                  c.finish(name, TAIL))[2]))

    # different words on one slot, around a table hit at lane 20 (L = 8, short: the trip goes on)
    def around(share, klit=20, L=8):
        def fn(c):
            srcs = _sources(c, 2)
            c.reset()
            c.lit(klit, share=share)
            c.copy(L, srcs[0])
            c.lit(9)
            c.copy(6, srcs[1])
        return fn
    add("shared/b_in_front_of_hit", around({12: 4}), 0)
    add("shared/three_on_one_slot", around({8: 2, 14: 2}), 1)

    def b_is_hit(c):                                  # literal lane 5 has the slot of the hit lane's word
        srcs = _sources(c, 2)
        c.reset()
        c.lit(20, share={5: ("slot", c.slot(srcs[0]))})
        c.copy(8, srcs[0])
        c.lit(9)
        c.copy(6, srcs[1])
    add("shared/b_is_hit_lane", b_is_hit, 2)

    def b_inside_match(c):                            # literal lane 5 has the slot of a word inside the match
        srcs = _sources(c, 2)
        c.reset()
        c.lit(20, share={5: ("slot", c.slot(srcs[0] + 3))})
        c.copy(10, srcs[0])
        c.lit(9)
        c.copy(6, srcs[1])
    add("shared/b_inside_match", b_inside_match, 3)

    def a_is_hit(c):                                  # the source's words at +0 and +4 share a slot: hit lane and
        c.lit(40)                                     # a lane inside the match
        p = c.next_lane0()
        c.lit(p - len(c.buf))
        c.lit(84, share={4: 0})
        c.reset()
        c.lit(11)
        c.copy(12, p)
        c.lit(5)
    add("shared/a_is_hit_lane", a_is_hit, 4)

    def stale(c):                                     # lane 3 of element 1 and lane 16 of element 2 on one slot
        srcs = _sources(c, 3)
        c.reset()
        c.lit(8)
        c.copy(5, srcs[0])
        c.lit(9, share={3: -10})
        c.copy(6, srcs[1])
        c.lit(4)
        c.copy(7, srcs[2])
    add("shared/stale_different_words", stale, 5)

    def stale_equal(c):                               # element 2 repeats a word of element 1's literals: its
        srcs = _sources(c, 2)                         # source was posted by element 1 of the same trip
        at = c.reset()
        c.lit(8)
        c.copy(5, srcs[0])
        c.lit(3)
        c.copy(6, at + 3)
        c.lit(4)
        c.copy(7, srcs[1])
    add("shared/stale_equal_words", stale_equal, 6)

    def local_then_table(c):                          # a local hit (equal words 5 apart) in front of a table hit
        srcs = _sources(c, 1)
        c.reset()
        c.lit(12)
        c.copy(6, len(c.buf) - 5)
        c.lit(6)
        c.copy(9, srcs[0])
    add("shared/equal_words_in_front_of_hit", local_then_table, 7)

    def local_far_lane(c):                            # source inside the same window, distance below 64
        c.lit(POOL + 16)
        at = c.reset()
        c.lit(45)
        c.copy(13, at + 2)
    add("shared/equal_words_same_window", local_far_lane, 8)

    def staying_lane_source(c):                       # a staying literal lane shares its slot with a lane inside the
        srcs = _sources(c, 1)                         # match; later its word is planted again and must be found
        at = c.reset()
        c.lit(15, share={6: ("slot", c.slot(srcs[0] + 2))})
        c.copy(9, srcs[0])
        c.lit(30)
        c.reset()
        c.lit(7)
        c.copy(8, at + 6)
    add("shared/staying_lane_is_later_source", staying_lane_source, 9)

    def inside_not_posted(c):                         # words inside a match are not posted: a later copy of the
        srcs = _sources(c, 1)                         # source's 4th byte on finds the source, not the match
        c.reset()
        c.lit(10)
        c.copy(14, srcs[0])
        c.lit(6)
        c.copy(8, srcs[0] + 64)
        c.lit(12)
        c.reset()
        c.lit(5)
        c.not_found(9, srcs[0] + 4)                   # (the source's +4 is lane 4 of a window without a hit)
    add("shared/inside_match_not_posted", inside_not_posted, 10)

    def hit_lane_posted(c):                           # the hit lane IS posted: the same source again is found at the
        srcs = _sources(c, 1)                         # first copy
        c.reset()
        c.lit(10)
        q = c.copy(9, srcs[0])
        c.lit(20)
        c.reset()
        c.lit(4)
        c.copy(9, q)
    add("shared/hit_lane_posted", hit_lane_posted, 11)
    def equal_a_is_hit(c):                            # the hit lane of element 1 (posted by it) is the source of
        srcs = _sources(c, 2)                         # element 2, whose lane read the older entry before
        c.reset()
        c.lit(10)
        q = c.copy(6, srcs[0])
        c.lit(4)
        c.copy(6, q)
        c.lit(5)
        c.copy(7, srcs[1])
    add("shared/equal_words_a_is_hit_lane", equal_a_is_hit, 12)

    def equal_b_inside(c):                            # a literal lane holds a word of the inside of the match that
        srcs = _sources(c, 2)                         # follows (its source is lane 2 of a window: never posted)
        c.reset()
        c.lit(6)
        c.not_found(4, srcs[0] + 2)
        c.lit(7)
        c.copy(9, srcs[0])
        c.lit(5)
        c.copy(7, srcs[1])
    add("shared/equal_words_b_inside_match", equal_b_inside, 13)

    def three_equal(c):                               # one word at three lanes of a trip: each finds the one before
        srcs = _sources(c, 1)
        at = c.reset()
        c.lit(6)
        q = c.copy(5, at + 2)
        c.lit(5)
        c.copy(6, q)
        c.lit(4)
        c.copy(7, srcs[0])
    add("shared/three_equal_words", three_equal, 14)

    def stale_equal_late(c):                          # as stale_equal_words, at lanes 25 / 30 / 45 / 50
        srcs = _sources(c, 2)
        at = c.reset()
        c.lit(30)
        c.copy(5, srcs[0])
        c.lit(10)
        c.copy(5, at + 25)
        c.lit(0)
        c.copy(7, srcs[1])
    add("shared/stale_equal_words_late", stale_equal_late, 15)

    def local_then_table_late(c):                     # equal words at lanes 20 and 40, a table hit at lane 49
        srcs = _sources(c, 1)
        at = c.reset()
        c.lit(40)
        c.copy(5, at + 20)
        c.lit(4)
        c.copy(9, srcs[0])
    add("shared/equal_words_in_front_of_hit_late", local_then_table_late, 16)

    def b_is_hit_equal(c):                            # the hit lane's word also lies 7 lanes before it: the local
        srcs = _sources(c, 2)                         # one wins over the older entry; then a table hit
        c.reset()
        c.lit(12)
        q = c.copy(4, srcs[0])
        c.lit(3)
        c.copy(6, q)
        c.lit(2)
        c.copy(8, srcs[1])
    add("shared/equal_words_b_is_hit_lane", b_is_hit_equal, 17)
    return cases


# ------------------------------------------------------------------------------------------ matchless_windows

STRETCHES = (59, 60, 61, 63, 64, 65, 127, 128, 129, 192, 193, 194, 255, 256, 257, 512, 1000)
WINDOW_LANES = (0, 1, 7, 8, 63)


def matchless_windows(seed=4):
    cases = []

    def stretch(c, n):
        c.tags = {"stretch": n}
        srcs = _sources(c, 1)
        c.reset()
        c.lit(n)
        c.copy(10, srcs[0])
        return c.finish(f"matchless/stretch{n}", TAIL)
    for i, n in enumerate(STRETCHES):
        cases.append(_build([seed, i], lambda c, n=n: stretch(c, n)))

    def window(c, w, lane):
        c.tags = {"window": w + 1, "lane": lane}
        srcs = _sources(c, 1)
        c.reset()
        c.lit(64 * w + lane)
        c.copy(6 + lane % 11, srcs[0])
        return c.finish(f"matchless/window{w + 1}_lane{lane}", TAIL)
    for w in (1, 2, 3):
        for lane in WINDOW_LANES:
            cases.append(_build([seed, 100 + w, lane], lambda c, w=w, lane=lane: window(c, w, lane)))

    def quirk(c, lane):                               # only lane 0 of a window without a hit is posted
        c.tags = {"quirk_lane": lane}
        c.lit(POOL + 16)
        at = c.reset()
        c.lit(150)                                    # windows at `at`, at + 64 without a hit; the hit in the third
        c.reset()
        c.lit(6)
        if lane == 0:
            c.copy(9, at + 64)
            c.tags["quirk_found"] = True
        else:
            c.not_found(4, at + 64 + lane)               # (4 bytes: the next word is not lane 0 of the window behind)
            c.tags["quirk_found"] = False
        return c.finish(f"matchless/quirk_lane{lane}", TAIL)
    for lane in (0, 1, 63):
        cases.append(_build([seed, 200 + lane], lambda c, lane=lane: quirk(c, lane)))
    return cases


# ------------------------------------------------------------------------------------------------- chunk_ends

END_LENGTHS = tuple(range(9)) + (143, 144, 145, 146, 255, 256, 257, 258, 65535, 65536, 65537)


def chunk_ends(seed=5):
    cases = []

    def plain(c, n):
        c.tags = {"total": n}
        (c.bulk if n > 4000 else c.lit)(n)
        return c.finish(f"ends/total{n}")
    for i, n in enumerate(END_LENGTHS):
        cases.append(_build([seed, i], lambda c, n=n: plain(c, n)))

    def handover(c, back, first):
        """An element that starts `back` bytes before the end: the straight path from 144 on.  first: it follows a
        short element of a trip that started with more room (straight -> general), else a reset."""
        c.tags = {"start_back": back, "after_short": first}
        srcs = _sources(c, 2)
        c.reset()
        if first:
            c.lit(4)
            c.copy(7, srcs[1])
        c.lit(5)
        c.copy(8, srcs[0])
        return c.finish(f"ends/start{back}_{'trip' if first else 'reset'}", back - 13)
    for back in (143, 144, 145):
        for first in (False, True):
            cases.append(_build([seed, 100 + back, first], lambda c, b=back, f=first: handover(c, b, f)))

    def tail_general_then_straight(c, back):          # a long literal stretch (general path) whose match ends
        c.tags = {"start_back": back, "after_general": True}
        srcs = _sources(c, 2)
        c.reset()
        c.lit(70)
        c.copy(9, srcs[0])
        c.lit(3)
        c.copy(6, srcs[1])
        return c.finish(f"ends/general_then_{back}", back - 9)
    for back in (143, 144, 145):
        cases.append(_build([seed, 150 + back], lambda c, b=back: tail_general_then_straight(c, b)))

    def into_end(c, left, L):
        c.tags = {"left_behind_match": left, "ends_in_match": left == 0}
        srcs = _sources(c, 1)
        c.reset()
        c.lit(7)
        _long_copy(c, L, srcs[0])
        return c.finish(f"ends/match{L}_left{left}", left)
    for left in range(6):
        for L in (4, 30, 64):
            cases.append(_build([seed, 200 + left, L], lambda c, left=left, L=L: into_end(c, left, L)))

    def cut(c, n):                                    # the source goes on matching; the chunk ends n < 60 bytes in
        c.tags = {"match60_cut": n}
        c.lit(POOL + 16)
        p = c.next_lane0()
        c.lit(p - len(c.buf) + 64 + 80)
        c.reset()
        c.lit(3)
        c.copy(4 + n, p)
        return c.finish(f"ends/match60_cut{n}")
    for n in (0, 1, 30, 59):
        cases.append(_build([seed, 300 + n], lambda c, n=n: cut(c, n)))

    def lits_after(c, n):                             # a chunk ending in 1 .. 4 literal bytes
        c.tags = {"last_literals": n}
        srcs = _sources(c, 1)
        c.reset()
        c.lit(50)
        c.copy(20, srcs[0])
        return c.finish(f"ends/last_literals{n}", n)
    for n in (1, 2, 3, 4):
        cases.append(_build([seed, 400 + n], lambda c, n=n: lits_after(c, n)))
    return cases


# ------------------------------------------------------------------------------------------------- beyond_64k

def beyond_64k(seed=6):
    cases = []
    LINE = 65536

    def near(c, at, back, n, name):
        """Bulk literals, then a 20-byte copy (a trip's end) and k literals so that a copy lies at `at` whose
        source is the posted position `back` bytes in front of it."""
        if c.composing:
            raise NotRelocatable(name)                # (planned at absolute positions)
        c.tags = {"kind": name}
        k = 5
        src = at - back
        assert src % 64 == 0
        pre = at - k - RESET_LEN
        c.bulk(pre // 256 * 256)
        anchor = pre // 256 * 256 - 64 * 3 if back > 400 else src - 64
        c.lit(pre - len(c.buf))
        c.copy(RESET_LEN, anchor)
        c.lit(k)
        assert len(c.buf) == at
        c.copy(9, src)
        (c.bulk)(n - len(c.buf) - TAIL)
        return c.finish(f"beyond/{name}", TAIL)
    # sources just before / after the 64 KiB line relative to the match
    cases.append(_build([seed, 0], lambda c: near(c, LINE + 30, 30 + 64, 70000, "source_before_line")))
    cases.append(_build([seed, 1], lambda c: near(c, LINE + 64 * 5 + 30, 30 + 64, 70000, "source_after_line")))
    cases.append(_build([seed, 2], lambda c: near(c, 2 * LINE + 10, 32768 - 64 + 10, 140000, "far_source_over_line")))
    cases.append(_build([seed, 3], lambda c: near(c, 3 * LINE + 64 * 9 + 1, 32768 - 64 * 9 + 1 + 64 * 8, 262144,
                                                  "three_lines_on")))

    def refused(c, lane, name):
        """P is lane 0 of a search (posted, and no window start up to P + 65536 posts into its slot again); 65 536
        bytes on a window starts whose position has the 16 bits the slot holds: the candidate is put 64 KiB back,
        to P, and refused as out of reach.  P's word is planted at lane 0 of that window (65 536 back) or at its
        lane 3 (65 539 back)."""
        c.tags = {"kind": name}
        assert len(c.buf) == c.pos0
        c.bulk(256 * 20)
        P = len(c.buf)
        c.bulk(LINE)
        assert len(c.buf) == P + LINE and (P - c.pos0) % 256 == 0
        if any(c.slot_at[p] == c.slot_at[P] for p in range(P + 64, P + LINE, 64)):
            raise PlanError("the slot of P is posted again")
        if lane:
            c.lit(lane)
        c.not_found(9, P)
        c.bulk(2000 if c.composing else 80000 - len(c.buf) - TAIL)
        return c.finish(f"beyond/{name}", TAIL)
    cases.append(_build([seed, 10], lambda c: refused(c, 0, "stored_equals_pos0_low_bits_lane0_65536_back")))
    cases.append(_build([seed, 11], lambda c: refused(c, 3, "stored_equals_pos0_low_bits_lane3")))

    def alias(c, same):
        """An entry older than 64 KiB: P, a literal lane in front of a hit (posted), holds word W and its slot is
        not posted again; P + 65536 is a lane of a window without a hit that is not lane 0 (never posted) and holds
        W again (same) or another word of W's slot; W planted 100 bytes further on reads P's 16 bits as P + 65536:
        found there (same), or not at all."""
        c.tags = {"kind": "alias_same_word" if same else "alias_other_word", "alias_found": same}
        base = len(c.buf)
        assert base == c.pos0
        c.bulk(2048)
        c.lit(9)
        c.copy(RESET_LEN, base + 1024)
        P = base + 2048 + 5
        c.bulk(P + LINE - len(c.buf))
        where = len(c.buf)
        if same:
            c.not_found(9, P)                         # (65 536 back: refused)
        else:
            c.lit(6, share={0: ("slot", c.slot(P))})
        c.lit(where + 100 - len(c.buf))
        if same:
            c.copy(9, where)
        else:
            c.not_found(9, P)
        c.bulk(2000 if c.composing else 72000 - len(c.buf) - TAIL)
        return c.finish(f"beyond/{c.tags['kind']}", TAIL)
    cases.append(_build([seed, 20], lambda c: alias(c, True)))
    cases.append(_build([seed, 21], lambda c: alias(c, False)))
    return cases


# --------------------------------------------------------------------------------------------------- composed

COMPOSED_SIZES = (65536, 65536, 65536, 1 << 20)


def _join(c, rng, fresh):
    """Between two situations: a few literals and a reset, from the latest copy of the pool or -- when that is out
    of reach or its slot has been posted over (fresh) -- from a new pool at the next posted lane 0."""
    if fresh or c.reset_last is None or len(c.buf) - c.reset_last > 30000:
        c.lit(5)
        p = c.next_lane0()
        c.lit(p - len(c.buf) + POOL + 8)
        c.reset_last = p
    c.lit(int(rng.integers(1, 40)))
    c.reset()


def composed(seed=7):
    """Situations of all families one after the other in one chunk, with a reset between, in an order shuffled by
    the seed: each is planted into a hash map full of what the ones before left, and past several 64 KiB lines.
    Three chunks of 64 KiB (the situations of up to 3 KiB) and one of 1 MiB (all that can be relocated)."""
    global _collect
    recipes = []
    for fam in ("hit_lane_by_length", "trips", "shared_hashes", "matchless_windows", "chunk_ends", "beyond_64k"):
        _collect = []
        try:
            FAMILIES[fam](SEEDS[fam])
            recipes += [(fam, fn) for fn in _collect]
        finally:
            _collect = None

    def build(c, k, size):
        rng = np.random.default_rng([seed, k, 5])
        c.composing = True
        order = rng.permutation(len(recipes)).tolist()
        room = 3200 if size <= 65536 else 140000
        per_family, skipped = {}, 0
        for idx in order:
            if len(c.buf) > size - room - 400:
                break
            fam, fn = recipes[idx]
            for attempt in range(4):
                m = c.mark()
                try:
                    if len(c.buf):
                        _join(c, rng, attempt > 0)
                    fn(c)
                    if len(c.buf) - m[0] > room:
                        raise PlanError("too large for this chunk")
                    per_family[fam] = per_family.get(fam, 0) + 1
                    break
                except NotRelocatable:
                    c.rollback(m)
                    break
                except PlanError as e:
                    c.rollback(m)
                    if "too large" in str(e):
                        break
            else:
                skipped += 1
        c.composing = False
        _join(c, rng, False)
        srcs = _sources(c, 1)
        c.reset()
        c.lit(7)
        c.copy(11 + k, srcs[0])
        left = size - len(c.buf)
        if left > 300:
            c.bulk(left - 200)
            left = 200
        c.tags = {"size": size, "situations": list(c.sits), "per_family": per_family, "gave_up": skipped}
        return c.finish(f"composed/{size}_{k}", left)
    return [_build([seed, k], lambda c, k=k, size=size: build(c, k, size), tries=6)
            for k, size in enumerate(COMPOSED_SIZES)]


FAMILIES = {"hit_lane_by_length": hit_lane_by_length, "trips": trips, "shared_hashes": shared_hashes,
            "matchless_windows": matchless_windows, "chunk_ends": chunk_ends, "beyond_64k": beyond_64k,
            "composed": composed}
SEEDS = {"hit_lane_by_length": 1, "trips": 2, "shared_hashes": 3, "matchless_windows": 4, "chunk_ends": 5,
         "beyond_64k": 6, "composed": 7}
_cache = {}


def family(name, seed=None):
    seed = SEEDS[name] if seed is None else seed
    if (name, seed) not in _cache:
        _cache[(name, seed)] = FAMILIES[name](seed)
    return _cache[(name, seed)]


def parse_elements(stream: bytes):
    """-> (declared size, [("L", n) | ("C", length, distance)]) of a Snappy stream as this encoder writes them."""
    i = n = sh = 0
    while True:
        b = stream[i]
        i += 1
        n |= (b & 0x7F) << sh
        sh += 7
        if b < 0x80:
            break
    out = []
    while i < len(stream):
        t = stream[i]
        kind = t & 3
        if kind == 0:
            ln = t >> 2
            i += 1
            if ln >= 60:
                nb = ln - 59
                ln = int.from_bytes(stream[i:i + nb], "little")
                i += nb
            out.append(("L", ln + 1))
            i += ln + 1
        elif kind == 1:
            out.append(("C", ((t >> 2) & 7) + 4, ((t & 0xE0) << 3) | stream[i + 1]))
            i += 2
        elif kind == 2:
            out.append(("C", (t >> 2) + 1, stream[i + 1] | (stream[i + 2] << 8)))
            i += 3
        else:
            out.append(("C", (t >> 2) + 1, int.from_bytes(stream[i + 1:i + 5], "little")))
            i += 5
    return n, out
