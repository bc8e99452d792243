"""Guarded output slots and damaged streams for the decoder containment tests.

The C API promises that chunk i of a batched decode writes only inside out_ptrs[i][0, out_caps[i]).  The
batches of hipcomp-core_amd/batch.py cannot see a write outside that range: every chunk has the same capacity, the
slots are that capacity rounded up to 16 bytes and back to back, so a short overrun lands in padding nobody reads
and a long one in the next chunk's slot.  GuardedSlots gives every chunk its own capacity and its own slot, with
guard bytes around it that hold a seeded pseudo-random pattern: a decoder that honours ANY capacity of the batch
(the wrong chunk's included) writes only into memory the test owns, and every such write is seen.

damaged() makes the damaged copies of a stream that tests/test_decode_containment_gpu.py, tests/
test_cascaded_damage_cpu.py and scripts/fuzz_decoders.py decode.  Plain numpy, no GPU needed to import.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

LEAD = 64     # guard bytes before every slot (at least)
TAIL = 64     # a slot's guard runs to at least max(caps) + TAIL bytes from the slot's start


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def pattern(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


class GuardedSlots:
    """One device allocation of len(caps) slots.  Slot i starts at a 16-byte boundary + offsets[(i + turn) % len]
    with at least LEAD pattern bytes before it; `region` bytes of slot i are the caller's ([ptr_i, ptr_i +
    region[i]), by default caps[i]), everything else of the arena is guard.  `chunks` (optional) are written at the
    slot starts (an input batch: the guards then also check that nothing writes into or around the input)."""

    def __init__(self, torch, caps: Sequence[int], device, offsets=(0,), turn=0, seed=0,
                 chunks: Optional[Sequence[bytes]] = None, region: Optional[Sequence[int]] = None):
        self.n = len(caps)
        self.caps = [int(c) for c in caps]
        self.region = list(self.caps if region is None else [int(r) for r in region])
        room = max(self.region + [len(c) for c in (chunks or [])] + [0])
        self.stride = _round_up(LEAD + 16 + room + TAIL, 16)
        self.offs = np.array([offsets[(i + turn) % len(offsets)] for i in range(self.n)], dtype=np.int64)
        self.at = np.arange(self.n, dtype=np.int64) * self.stride + LEAD + self.offs   # slot starts in the arena
        self.host = pattern(seed, self.n * self.stride + LEAD)
        if chunks is not None:
            for i, c in enumerate(chunks):
                self.host[self.at[i]:self.at[i] + len(c)] = np.frombuffer(c, dtype=np.uint8)
        self.data = torch.from_numpy(self.host.copy()).to(device)
        base = self.data.data_ptr()
        assert base % 16 == 0
        self.ptrs = torch.from_numpy(self.at + base).to(device)
        self.sizes = torch.tensor([len(c) for c in chunks] if chunks is not None else [0] * self.n,
                                  dtype=torch.int64, device=device)
        self.caps_t = torch.tensor(self.caps, dtype=torch.int64, device=device)

    def batch(self, hc):
        return hc.batch.ChunkBatch(self.data, self.ptrs, self.sizes, self.stride)

    def after(self) -> np.ndarray:
        return self.data.cpu().numpy()

    def where(self, idx: int) -> str:
        """An arena byte as chunk index and signed offset from the start of that chunk's capacity."""
        i = min(int(idx // self.stride), self.n - 1)   # slot i's part of the arena: [i * stride, (i + 1) * stride)
        return f"chunk {i} offset {int(idx - self.at[i]):+d} (capacity {self.caps[i]}, region {self.region[i]})"

    def first_guard_change(self, got: Optional[np.ndarray] = None) -> Optional[str]:
        """None if every byte outside the slots' regions still holds the pattern, else where the first is."""
        got = (self.after() if got is None else got).copy()
        for a, r in zip(self.at.tolist(), self.region):   # (the regions are the caller's: take them out)
            got[a:a + r] = self.host[a:a + r]
        bad = np.flatnonzero(got != self.host)
        if bad.size == 0:
            return None
        return f"{bad.size} guard byte(s) changed, first at {self.where(int(bad[0]))}"

    def unchanged(self, got: Optional[np.ndarray] = None) -> Optional[str]:
        """None if no byte of the arena changed (an input batch), else where the first change is."""
        got = self.after() if got is None else got
        bad = np.flatnonzero(got != self.host)
        return None if bad.size == 0 else f"{bad.size} byte(s) changed, first at {self.where(int(bad[0]))}"

    def slot_bytes(self, got: np.ndarray, i: int, n: int) -> bytes:
        return got[self.at[i]:self.at[i] + n].tobytes()


# ---------------------------------------------------------------------------------------------- damaged streams

def _generic(rng, good: bytes, kind: int) -> bytes:
    """Today's damage of the LZ4 / Snappy tests: bytes changed, one removed, one inserted, the stream cut short;
    kind 4: an LZ4 offset byte pair somewhere set to a near / far / zero offset (scripts/fuzz_decoders.py)."""
    b = bytearray(good)
    if not b:
        return bytes([int(rng.integers(0, 256))])
    if kind == 0:
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif kind == 1:
        del b[int(rng.integers(0, len(b)))]
    elif kind == 2:
        b.insert(int(rng.integers(0, len(b) + 1)), int(rng.integers(0, 256)))
    elif kind == 3:
        b = b[: int(rng.integers(0, len(b)))]
    else:
        at = int(rng.integers(0, max(1, len(b) - 1)))
        v = int(rng.choice([0, 1, 2, 3, 4, 7, 63, 64, 65, 255, 256, 4000, 65535]))
        b[at] = v & 0xFF
        if at + 1 < len(b):
            b[at + 1] = v >> 8
    return bytes(b)


CASCADED_SIZE = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 8, 7: 8}
SUB_CHUNK = 4096


def cascaded_layout(good: bytes):
    """The sub-chunks of a well-formed Cascaded partition, as the decoder walks them (oracle/cascaded_oracle.c):
    -> (s, R, D, bp, metadata bytes, [(pos, meta words, array offsets relative to pos)])."""
    R, D, bp, t = good[0], good[1], good[2] & 0x0F, good[3]
    s = CASCADED_SIZE[t]
    msz = _round_up(4 + 4 * (R + 1), s) + _round_up(s * D, 4)
    subs = []
    if R == 0 and D == 0 and bp == 0:
        return s, R, D, bp, msz, subs
    pos = _round_up(8, s)
    while pos + msz <= len(good) // 4 * 4:
        meta = [int.from_bytes(good[pos + 4 * k: pos + 4 * k + 4], "little") for k in range(R + 2)]
        offs = [0]
        if R > 0:
            for i in range(R - 1):
                offs.append(_round_up(offs[i] + meta[i + 1], 4))
            offs.append(_round_up(offs[R - 1] + meta[R], max(s, 4)))
        subs.append((pos, meta, [pos + msz + o for o in offs]))
        if meta[0] < 4:
            break
        pos = _round_up(pos + meta[0] // 4 * 4, s)
    return s, R, D, bp, msz, subs


def _put32(b: bytearray, at: int, v: int):
    if 0 <= at and at + 4 <= len(b):
        b[at:at + 4] = (v & 0xFFFFFFFF).to_bytes(4, "little")


def cascaded_damage(good: bytes):
    """Damage at every place the Cascaded decoder trusts (deterministic): the header bytes (R, D, the bit-pack
    byte with its high nibble, the type), the uncompressed-bytes word, every sub-chunk's size word, the
    array-length words, the bit-pack headers of the arrays (frame of reference, count, bit widths up to and beyond
    the element's width), truncation at every sub-chunk boundary +-0/1/4, a sub-chunk duplicated or removed."""
    out = []

    def edit(fn):
        b = bytearray(good)
        fn(b)
        if bytes(b) != good:
            out.append(bytes(b))

    if len(good) < 8:
        return [good[:k] for k in range(len(good))]
    R, D, bp, t = good[0], good[1], good[2], good[3]
    s, R, D, bpl, msz, subs = cascaded_layout(good)
    ub = int.from_bytes(good[4:8], "little")

    def setbyte(at, v):
        return lambda b: b.__setitem__(at, v & 0xFF)
    for v in (R + 1, R - 1, 0, 7, 8, 255):
        edit(setbyte(0, v))
    for v in (D + 1, D - 1, 0, 255):
        edit(setbyte(1, v))
    for v in (bp ^ 1, bp | 0x10, 0xF0 | bp, 2):
        edit(setbyte(2, v))
    for v in (t ^ 1, t ^ 2, t ^ 4, t ^ 6, 8, 255):
        edit(setbyte(3, v))
    for v in (ub - s, ub + s, ub - SUB_CHUNK, ub + SUB_CHUNK, 0, 0xFFFFFFFF):
        if v >= 0:
            edit(lambda b, v=v: _put32(b, 4, v))
    ends = [len(good)]
    for k, (pos, meta, arrays) in enumerate(subs):
        left = len(good) - pos
        for v in (0, 1, 2, 3, left - 4, left - 1, left + 1, left + 4, meta[0] + 4, 0x80000000, 0xFFFFFFFF):
            edit(lambda b, v=v, pos=pos: _put32(b, pos, v))
        for j in range(1, R + 2):
            m = meta[j]
            for v in (m - 1, m + 1, m - 4, m + 4, 0, 2 * m + 8, 0xFFFF, 0xFFFFFFFF):
                edit(lambda b, v=v, at=pos + 4 * j: _put32(b, at, max(v, 0)))
        if bpl:   # the bit-pack header of every array: RLE counts (2-byte) and the values (s bytes)
            for a, es in [(arrays[l], 2) for l in range(R)] + [(arrays[R], s)]:
                w_off = _round_up(es, 4)
                if a + w_off + 4 > len(good):
                    continue
                word = int.from_bytes(good[a + w_off: a + w_off + 4], "little")
                cnt, bw = word & 0xFFFF, word >> 16
                for nbw in (0, 1, bw + 1, 8 * es - 1, 8 * es, 8 * es + 1, 33, 65, 0xFFFF):
                    edit(lambda b, at=a + w_off, v=(nbw << 16) | cnt: _put32(b, at, v))
                for ncnt in (cnt + 1, cnt - 1, 0, 0xFFFF):
                    edit(lambda b, at=a + w_off, v=(bw << 16) | (ncnt & 0xFFFF): _put32(b, at, v))
                edit(lambda b, at=a: b.__setitem__(at, b[at] ^ 0x01))                 # frame of reference + 1 bit
                edit(lambda b, at=a + es - 1: b.__setitem__(at, b[at] ^ 0x80))        # and its sign
        ends.append(pos)
    for e in sorted(set(ends + [_round_up(8, s)])):
        for d in (-4, -1, 0, 1, 4):
            if 0 <= e + d < len(good):
                out.append(good[: e + d])
    if subs:
        bounds = [p for p, _, _ in subs] + [len(good)]
        for k in range(len(subs)):
            one = good[bounds[k]:bounds[k + 1]]
            dup = good[:bounds[k + 1]] + one + good[bounds[k + 1]:]
            cut = good[:bounds[k]] + good[bounds[k + 1]:]
            out += [dup, cut]
            # the same with the uncompressed-bytes word made to fit what the sub-chunks now hold
            for b, delta in ((dup, 1), (cut, -1)):
                n_k = min(SUB_CHUNK, ub - (SUB_CHUNK * k)) if ub > SUB_CHUNK * k else 0
                bb = bytearray(b)
                _put32(bb, 4, max(ub + delta * n_k, 0))
                out.append(bytes(bb))
    return out


def damaged(codec: str, good: bytes, rng, n: int):
    """Damaged copies of a good stream of `codec` ("LZ4", "Snappy" or "Cascaded"), seeded by `rng`
    (np.random.Generator).  LZ4 / Snappy: n copies, the generic damage in turn (LZ4 with its offset pair edits).
    Cascaded: every edit of cascaded_damage() and n generic ones on top."""
    if codec == "Cascaded":
        return cascaded_damage(good) + [_generic(rng, good, k % 4) for k in range(n)]
    kinds = 5 if codec == "LZ4" else 4
    return [_generic(rng, good, k % kinds) for k in range(n)]


def capacity_kinds(true_size: int, es: int):
    """The capacities the containment tests give a chunk whose decoded size is `true_size`: exact, -1, +1,
    -one element, +15, +16, 1, 0, much larger than needed."""
    return [true_size, max(true_size - 1, 0), true_size + 1, max(true_size - es, 0), true_size + 15,
            true_size + 16, 1, 0, 3 * true_size + 100]


# ------------------------------------------------------------------------------------------- Cascaded corpus

CASCADED_OPTS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 1, 1), (3, 2, 1))   # (RLEs, deltas, bit-pack)
CASCADED_NP = {0: np.int8, 1: np.uint8, 2: np.int16, 3: np.uint16, 4: np.int32, 5: np.uint32, 6: np.int64,
               7: np.uint64}


def cascaded_sources(t: int, seed: int):
    """Sources of type tag t, 8 KiB at most: a sorted column over two sub-chunks and a bit (runs, deltas, narrow
    bit widths), short runs of small signed values, and full-width random values over one and a half sub-chunks."""
    dt = CASCADED_NP[t]
    s = CASCADED_SIZE[t]
    rng = np.random.default_rng(seed)
    sorted_col = np.cumsum(np.where(rng.integers(0, 4, 8000 // s) == 0, 0, rng.integers(1, 9, 8000 // s)))
    runs = np.repeat(rng.integers(-60, 60, 2000), rng.integers(1, 12, 2000))[: 3000 // s]
    wide = rng.integers(0, 256, 6000 // s * s, dtype=np.uint8).view(dt)
    return [sorted_col.astype(dt).tobytes(), runs.astype(dt).tobytes(), wide.tobytes()]


def cascaded_corpus(oracle, seed: int = 7, generic: int = 6):
    """Good Cascaded streams of all 8 types under every option set of CASCADED_OPTS, each followed by its damaged
    copies: -> [(stream, source bytes, type tag, good?)]."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(8):
        for k, (r, d, b) in enumerate(CASCADED_OPTS):
            for src in cascaded_sources(t, seed * 1000 + 10 * t + k):
                good = oracle.cascaded_compress(src, t, r, d, b)[0]
                out.append((good, src, t, True))
                out += [(s, src, t, False) for s in damaged("Cascaded", good, rng, generic)]
    return out
