"""The libzstd-made fixtures of the Zstandard tests: tests/golden/zstd/fixture.json (the index) and fixture.bin.

    python tests/zstd_fixtures.py        writes both again (needs libzstd.so.1)

* frames: libzstd's own frames at levels -5 to 19 of seeded inputs (empty, one byte, zeros, random, text, skewed
  bytes, periodic, integers; 300 KiB of content at most).  Only the frame is kept: the content comes back from
  inputs() by name, and its MD5 is in the index.
* damaged: seeded damaged copies of a few of those frames with libzstd's verdict and the MD5 of what it decoded.
  The damage kinds are the four generic ones of tests/decode_guard.py (_generic kinds 0-3), `cut` (the chunk cut
  at a section boundary: behind a frame, a frame header, a block header, a block, a literals section) and `bit`
  (one bit flipped in a frame header, a block header, a literals header or a sequences header).  make() asserts
  that within every kind libzstd accepts some cases and refuses some.  For the kinds in which that is rare there are
  sources made for it: a row of one-byte frames (a cut at a random byte that falls behind a frame), a row of empty
  skippable frames in front of a frame (a byte inserted into a length field or as a new frame header descriptor)
  and a skippable frame that holds a skippable frame and a frame (a byte removed from the outer header, after which
  the inner frames are read).  Only the sources' frames and the verdicts are kept: damaged_chunks() makes the chunks
  again from them and the seed.

About one random damage in 150 is accepted by libzstd 1.4.8 only through one of the documented differences of
include/hipcomp/zstd.h (a Huffman or sequence bitstream that is not exactly consumed).  Those differences have
named tests of their own (tests/test_zstd_framegen_cpu.py); the seed below was chosen so that the damaged set
holds none of them, and make() refuses to write a set on which the scalar decoder of tests/zstd_tables_driver.cpp
and libzstd disagree, printing the cases."""
from __future__ import annotations

import hashlib
import json
import os
import struct

import numpy as np

import zstd_framegen as G
from decode_guard import _generic

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "zstd")
SEED = 8878
DAMAGE_SEED = 8880   # chosen so that every assertion of make() holds
SLACK = 64   # capacity given to a damaged chunk beyond its source's size


def inputs():
    rng = np.random.default_rng(SEED)
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"1996-01-02", b"BUILDING", b"carefully",
             b"final", b"deposits", b"furiously", b"ironic", b"requests", b"TRUCK", b"0.04", b"N", b"O"]

    def text(n):
        return b" ".join(words[i] for i in rng.integers(0, len(words), n // 4 + 1))[:n]
    return {
        "empty": b"", "one_byte": b"a", "zeros": bytes(300 * 1024), "random": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
        "text_small": text(900), "text": text(65536), "text_large": text(300 * 1024),
        "skewed": rng.choice(np.array([65, 66, 67, 200, 201, 9], dtype=np.uint8), 40000, p=[.6, .2, .1, .05, .03, .02]).tobytes(),
        "periodic": b"abcdefghijk" * 9000, "skewed_small": bytes(rng.choice(np.array([65, 66, 67, 200], dtype=np.uint8), 3000, p=[.6, .2, .15, .05])),
        "integers_small": np.arange(500, dtype=np.int32).tobytes(), "integers": (1000 + rng.integers(0, 50, 8000).cumsum()).astype(np.int32).tobytes(),
    }


FRAMES = [("empty", 3), ("one_byte", 3), ("zeros", 1), ("zeros", 19), ("random", 3), ("text_small", -5), ("text_small", 3),
          ("text_small", 19), ("text", -5), ("text", 1), ("text", 3), ("text", 19), ("text_large", 3),
          ("skewed", -5), ("skewed", 3), ("skewed", 19), ("periodic", 1), ("periodic", 12), ("integers", 3),
          ("integers", 15)]
DAMAGE_SOURCES = [("text_small", 3), ("text_small", 19), ("skewed_small", 3), ("integers_small", 3), ("one_byte", 3)]
GENERIC_PER_KIND = 8
REMOVALS, INSERTIONS = 64, 640


def boundaries(chunk: bytes):
    """-> (section boundaries, [(header kind, byte offset)]) of a legal chunk."""
    cuts, heads, at = [], [], 0
    while at < len(chunk):
        fhd = chunk[at + 4]
        single, flag = fhd >> 5 & 1, fhd >> 6
        heads.append(("frame", at + 4))
        at += 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0) if flag == 0 else 1 << flag)
        cuts.append(at)
        while True:
            h = int.from_bytes(chunk[at:at + 3], "little")
            last, kind, size = h & 1, h >> 1 & 3, h >> 3
            heads.append(("block", at))
            at += 3
            cuts.append(at)
            if kind == 2:
                b = chunk[at:at + size]
                t, sf = b[0] & 3, b[0] >> 2 & 3
                heads.append(("literals", at))
                if t < 2:
                    hb = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                    lit_end = hb + ((b[0] >> 3 if hb == 1 else int.from_bytes(b[:hb], "little") >> 4) if t == 0 else 1)
                else:
                    hb = 3 if sf < 2 else sf + 2
                    lhc = int.from_bytes(b[:5], "little")
                    lit_end = hb + {3: lhc >> 14 & 0x3FF, 4: lhc >> 18 & 0x3FFF, 5: lhc >> 22 & 0x3FFFF}[hb]
                cuts.append(at + lit_end)
                heads.append(("sequences", at + lit_end))
                n = b[lit_end]
                if n:
                    heads.append(("sequences", at + lit_end + (1 if n < 128 else 2 if n < 255 else 3)))
            at += 1 if kind == 1 else size
            cuts.append(at)
            if last:
                break
        if fhd & 4:
            at += 4
            cuts.append(at)
    return sorted(set(cuts)), heads


def damaged_chunks(frames):
    """-> [(kind, chunk, capacity)] from the seed and the damage sources' frames alone"""
    rng = np.random.default_rng(DAMAGE_SEED)
    data = inputs()
    out = []
    one = frames[("one_byte", 3)]
    # twelve one-byte frames in a row: a cut at a random byte can fall behind a frame
    out += [("generic_3", _generic(rng, one * 12, 3), 12 + SLACK) for _ in range(3 * GENERIC_PER_KIND)]
    # a skippable frame that holds a zero byte, a skippable frame and a frame: without a byte of its header's end the
    # chunk reads as what it holds (about one removal in twenty)
    nested = G.skippable(b"\x00" + G.skippable(b"12345") + one) + one
    out += [("generic_1", _generic(rng, nested, 1), 2 + SLACK) for _ in range(REMOVALS)]
    # empty skippable frames in front of a frame: a byte inserted into a length field, or as a new frame header
    # descriptor, can leave a legal chunk (about one insertion in two hundred)
    row = G.skippable(b"") * 16 + one
    out += [("generic_2", _generic(rng, row, 2), 1 + SLACK) for _ in range(INSERTIONS)]
    for k, (name, level) in enumerate(DAMAGE_SOURCES):
        good = frames[(name, level)]
        cap = len(data[name]) + SLACK
        for kind in range(4):
            out += [(f"generic_{kind}", _generic(rng, good, kind), cap) for _ in range(GENERIC_PER_KIND)]
        # the same frame twice: a cut behind the first frame leaves a legal chunk
        two = good + good
        cuts, heads = boundaries(two)
        out += [("cut", two[:c], 2 * cap) for c in cuts[:-1]]
        for what, at in heads[:len(heads) // 2]:
            for bit in rng.choice(8, 3, replace=False):
                b = bytearray(good)
                b[at] ^= 1 << int(bit)
                out.append(("bit", bytes(b), cap))
    return out


def make():
    assert G.libzstd() is not None, "libzstd.so.1 does not load"
    data = inputs()
    frames = {(n, l): G.compress(data[n], l) for n, l in FRAMES + DAMAGE_SOURCES}
    blob, index = bytearray(), {"frames": [], "damaged": []}

    def put(b):
        at = len(blob)
        blob.extend(b)
        return [at, len(b)]
    for n, l in FRAMES:
        assert G.arbiter(frames[(n, l)], len(data[n])) == data[n]
        index["frames"].append({"input": n, "level": l, "at": put(frames[(n, l)]), "size": len(data[n]),
                                "md5": hashlib.md5(data[n]).hexdigest()})
    index["sources"] = [{"input": n, "level": l, "at": put(frames[(n, l)])} for n, l in DAMAGE_SOURCES]
    verdicts = {}
    for kind, chunk, cap in damaged_chunks(frames):   # (the chunks themselves come back from the sources and the seed)
        got = G.arbiter(chunk, cap)
        verdicts.setdefault(kind, set()).add(got is not None)
        index["damaged"].append([kind, hashlib.md5(chunk).hexdigest()[:12], cap, None if got is None else len(got),
                                 None if got is None else hashlib.md5(got).hexdigest()])
    for kind, seen in sorted(verdicts.items()):
        want = {True, False}
        assert seen == want, f"damage kind {kind}: libzstd's verdicts are {seen}"
    return index, bytes(blob)


def load():
    """-> (frames [(name, chunk, content)], damaged [(kind, chunk, capacity, size or None, md5 or None)])"""
    with open(os.path.join(DIR, "fixture.json")) as f:
        index = json.load(f)
    with open(os.path.join(DIR, "fixture.bin"), "rb") as f:
        blob = f.read()
    data = inputs()
    cut = lambda at: blob[at[0]:at[0] + at[1]]
    frames = []
    for e in index["frames"]:
        assert hashlib.md5(data[e["input"]]).hexdigest() == e["md5"], "inputs() no longer makes the fixture's content"
        frames.append((f"{e['input']}_level_{e['level']}", cut(e["at"]), data[e["input"]]))
    sources = {(e["input"], e["level"]): cut(e["at"]) for e in index["sources"]}
    chunks = damaged_chunks(sources)
    assert len(chunks) == len(index["damaged"])
    damaged = []
    for (kind, chunk, cap), e in zip(chunks, index["damaged"]):
        assert [kind, hashlib.md5(chunk).hexdigest()[:12], cap] == e[:3], "the damage is no longer the fixture's"
        damaged.append((kind, chunk, cap, e[3], e[4]))
    return frames, damaged


def driver_cases(cases) -> bytes:
    """The case file of tests/zstd_tables_driver.cpp: (chunk, capacity) records."""
    return b"".join(struct.pack("<IQ", len(c), cap) + c for c, cap in cases)


def driver_results(blob: bytes, n: int):
    """-> [content or None] from the driver's result file"""
    out, at = [], 0
    for _ in range(n):
        ok, size = struct.unpack_from("<IQ", blob, at)
        at += 12
        out.append(blob[at:at + size] if ok else None)
        at += size
    assert at == len(blob)
    return out


if __name__ == "__main__":
    import subprocess
    import tempfile
    index, blob = make()
    # the set must hold no case of the documented differences (see above)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "driver")
        root = os.path.dirname(HERE)
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"), "-I",
                        os.path.join(root, "hipcomp-core_amd", "csrc"), os.path.join(HERE, "zstd_tables_driver.cpp"), "-o", exe], check=True)
        sources = {(e["input"], e["level"]): blob[e["at"][0]:e["at"][0] + e["at"][1]] for e in index["sources"]}
        cases = [(c, cap) for _, c, cap in damaged_chunks(sources)]
        with open(os.path.join(tmp, "cases"), "wb") as f:
            f.write(driver_cases(cases))
        subprocess.run([exe, "decode", os.path.join(tmp, "cases"), os.path.join(tmp, "res")], check=True)
        with open(os.path.join(tmp, "res"), "rb") as f:
            got = driver_results(f.read(), len(cases))
        differ = [(i, e[0]) for i, (e, g) in enumerate(zip(index["damaged"], got)) if (g is None) != (e[3] is None)]
        assert not differ, f"cases under a documented difference (choose another SEED): {differ}"
    os.makedirs(DIR, exist_ok=True)
    with open(os.path.join(DIR, "fixture.json"), "w") as f:
        json.dump(index, f, separators=(",", ":"))
    with open(os.path.join(DIR, "fixture.bin"), "wb") as f:
        f.write(blob)
    acc = sum(e[3] is not None for e in index["damaged"])
    print(f"{len(index['frames'])} frames, {len(index['damaged'])} damaged ({acc} accepted by libzstd), {len(blob)} bytes")
