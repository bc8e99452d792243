"""The libzstd-made fixtures of the Zstandard dictionary tests: tests/golden/zstd_dict/fixture.json (the index) and
fixture.bin.

    python tests/zstd_dict_fixtures.py        writes both again (needs libzstd.so.1 and g++)

* dictionaries: "a" and "b", trained by ZDICT_trainFromBuffer from seeded records of two vocabularies (so their IDs
  differ), and "raw", raw content.
* frames: ZSTD_compress_usingDict at levels -5, 1, 3 and 19 of seeded records of 0, 1, about 60, 300 and 5000 bytes, of
  70 000 bytes and of 300 KiB (several blocks follow the first), one chunk of two frames, one record made to continue
  the dictionary's end, one frame compressed without a dictionary and decoded with one, and frames against "b" and "raw".  Only the frame is kept: the content comes back
  from inputs() by name, and its MD5 is in the index.
* damaged: seeded damaged copies of frames (decoded with the dictionary they were made with) and of dictionary "a"
  (a good frame decoded with the damaged dictionary), with libzstd's verdict, the MD5 of what it decoded and whether it loads the dictionary.  The
  damage kinds are the four generic ones of tests/decode_guard.py; as in tests/zstd_fixtures.py there are sources made
  so that every kind is accepted sometimes: a row of small frames, nested skippable frames, a row of empty ones.

make() asserts that the set holds a frame whose first block has Treeless literals, one with a Repeat_Mode table in its
first block, one with a match that begins in the dictionary and one whose match continues into the output (counted by
tests/zstd_dict_driver.cpp), that within every damage kind libzstd accepts some cases and refuses some, and that the
driver and libzstd agree on every case; otherwise nothing is written."""
from __future__ import annotations

import hashlib
import json
import os
import struct
import subprocess
import tempfile

import numpy as np

import zstd_dictgen as D
import zstd_framegen as G
from decode_guard import _generic

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIR = os.path.join(HERE, "golden", "zstd_dict")
SEED = 8878
DAMAGE_SEED = 2     # chosen so that every assertion of make() holds
SLACK = 64
DICT_BYTES = 16 * 1024
LEVELS = (-5, 1, 3, 19)
SIZES = (("empty", 0), ("one_byte", 1), ("r60", 60), ("r300", 300), ("r5000", 5000), ("r70000", 70000), ("r300k", 300 * 1024))
GENERIC_PER_KIND = 10
REMOVALS, INSERTIONS = 128, 640
NO_DICT = 0xFFFFFFFF


def records(seed, vocabulary, count):
    rng = np.random.default_rng(seed)
    keys = [b"id", b"user", b"status", b"region", b"amount", b"comment", b"timestamp", b"tags"]
    out = []
    for _ in range(count):
        fields = []
        for k in keys[:int(rng.integers(3, len(keys) + 1))]:
            words = b" ".join(vocabulary[i] for i in rng.integers(0, len(vocabulary), int(rng.integers(1, 6))))
            fields.append(b'"' + k + b'": "' + words + b'"' if rng.integers(0, 2) else b'"' + k + b'": ' + str(int(rng.integers(0, 100000))).encode())
        out.append(b"{" + b", ".join(fields) + b"}")
    return out


VOCAB_A = [b"pending", b"shipped", b"returned", b"eu-west", b"us-east", b"ap-south", b"carefully", b"final", b"deposits", b"express",
           b"furiously", b"ironic", b"requests", b"TRUCK", b"AIR", b"RAIL", b"2024-01-02T03:04:05Z", b"gold", b"silver", b"none"]
VOCAB_B = [b"GET", b"POST", b"/api/v1/items", b"/api/v1/users", b"200", b"404", b"500", b"Mozilla/5.0", b"curl/8.1", b"keep-alive",
           b"gzip", b"text/html", b"application/json", b"cache-miss", b"cache-hit", b"edge-7", b"edge-12", b"ms", b"bytes", b"-"]


def inputs(dicts):
    """-> {name: content} of the frames, from the seed; "cross" is the end of dictionary "a" and a bit of it again, so
    that a match that begins in the dictionary goes on into the output"""
    out = {"cross": dicts["a"][-40:] + dicts["a"][-40:-15]}
    for k, (name, n) in enumerate(SIZES):
        out[name] = b"\n".join(records(SEED + 10 + k, VOCAB_A, max(1, n // 60)))[:n]
    out["b60"] = records(SEED + 30, VOCAB_B, 1)[0]
    out["b5000"] = b"\n".join(records(SEED + 31, VOCAB_B, 90))[:5000]
    return out


def dictionaries():
    a = D.train(records(SEED, VOCAB_A, 4000), DICT_BYTES)
    b = D.train(records(SEED + 1, VOCAB_B, 4000), DICT_BYTES)
    return {"a": a, "b": b, "raw": b"\n".join(records(SEED + 2, VOCAB_A, 30))[:2000]}


def frame_plans():
    """-> [(name, [(input, level, dictionary to compress with or None)], dictionary to decode with)]"""
    out = [(f"{name}_level_{level}", [(name, level, "a")], "a") for name, _ in SIZES for level in LEVELS]
    out += [("two_frames", [("r300", 3, "a"), ("r60", 1, "a")], "a"), ("made_without_dictionary", [("r300", 3, None)], "a"),
            ("cross_level_3", [("cross", 3, "a")], "a"), ("cross_level_19", [("cross", 19, "a")], "a"),
            ("b60_level_3", [("b60", 3, "b")], "b"), ("b5000_level_19", [("b5000", 19, "b")], "b"),
            ("r300_raw_level_3", [("r300", 3, "raw")], "raw"), ("r5000_raw_level_1", [("r5000", 1, "raw")], "raw")]
    return out


DAMAGE_SOURCES = ("r60_level_3", "r300_level_3", "r300_level_19", "r5000_level_1", "one_byte_level_3")


def damaged_chunks(frames, dicts):
    """frames: {name: (chunk, content size)} of the damage sources -> [(kind, chunk, capacity, dictionary bytes)] from the
    seed alone.  Kinds frame_0..3: a damaged frame with dictionary "a"; dict_0..3: a good frame with a damaged "a"."""
    rng = np.random.default_rng(DAMAGE_SEED)
    a = dicts["a"]
    one = frames["one_byte_level_3"][0]
    out = [("frame_3", _generic(rng, one * 12, 3), 12 + SLACK, a) for _ in range(4 * GENERIC_PER_KIND)]
    nested = G.skippable(b"\x00" + G.skippable(b"12345") + one) + one
    out += [("frame_1", _generic(rng, nested, 1), 2 + SLACK, a) for _ in range(REMOVALS)]
    row = G.skippable(b"") * 16 + one
    out += [("frame_2", _generic(rng, row, 2), 1 + SLACK, a) for _ in range(INSERTIONS)]
    for name in DAMAGE_SOURCES:
        good, size = frames[name]
        for kind in range(4):
            out += [(f"frame_{kind}", _generic(rng, good, kind), size + SLACK, a) for _ in range(GENERIC_PER_KIND)]
    good, size = frames["r300_level_3"]
    head = a[:400]      # the dictionary's entropy tables lie in its first few hundred bytes
    for kind in range(4):
        out += [(f"dict_{kind}", good, size + SLACK, _generic(rng, a, kind)) for _ in range(GENERIC_PER_KIND)]
        out += [(f"dict_{kind}", good, size + SLACK, _generic(rng, head, kind) + a[400:]) for _ in range(GENERIC_PER_KIND)]
    return out


def driver_cases(cases) -> bytes:
    """The decode / sizes case file of tests/zstd_dict_driver.cpp: (chunk, capacity, dictionary or None) records."""
    return b"".join(struct.pack("<IQI", len(c), cap, NO_DICT if d is None else len(d)) + c + (d or b"") for c, cap, d in cases)


def driver_results(blob: bytes, n: int):
    """-> [(content or None, matches that begin in the dictionary, of those crossing into the output, first-block forms)]"""
    out, at = [], 0
    for _ in range(n):
        ok, size, in_dict, crossing, forms = struct.unpack_from("<IQIII", blob, at)
        at += 24
        out.append((blob[at:at + size] if ok else None, in_dict, crossing, forms))
        at += size
    assert at == len(blob)
    return out


def prepare_cases(dicts) -> bytes:
    return b"".join(struct.pack("<I", len(d)) + d for d in dicts)


def prepare_results(blob: bytes, n: int):
    """-> [prepared blob or None]"""
    out, at = [], 0
    for _ in range(n):
        status, size = struct.unpack_from("<IQ", blob, at)
        at += 12
        out.append(blob[at:at + size] if status == 0 else None)
        at += size
    assert at == len(blob)
    return out


def build_driver(directory, sanitize=True) -> str:
    exe = os.path.join(directory, "zstd_dict_driver")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hipcomp-core_amd", "csrc")]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(cmd + [os.path.join(HERE, "zstd_dict_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_driver(exe, directory, mode, payload: bytes) -> bytes:
    cases, res = os.path.join(directory, "cases"), os.path.join(directory, "res")
    with open(cases, "wb") as f:
        f.write(payload)
    r = subprocess.run([exe, mode, cases, res], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(res, "rb") as f:
        return f.read()


def make():
    assert D.libzstd() is not None, "libzstd.so.1 does not load"
    dicts = dictionaries()
    data = inputs(dicts)
    assert D.libzstd().ZDICT_getDictID(dicts["a"], len(dicts["a"])) != D.libzstd().ZDICT_getDictID(dicts["b"], len(dicts["b"]))
    blob, index = bytearray(), {"dictionaries": {}, "frames": [], "damaged": []}

    def put(b):
        at = len(blob)
        blob.extend(b)
        return [at, len(b)]
    for name, d in dicts.items():
        index["dictionaries"][name] = put(d)
    frames = {}
    for name, parts, dec in frame_plans():
        chunk = b"".join(D.compress(data[i], level, dicts[c] if c else b"") for i, level, c in parts)
        content = b"".join(data[i] for i, _, _ in parts)
        assert D.arbiter(chunk, len(content), dicts[dec]) == content, name
        frames[name] = (chunk, len(content))
        index["frames"].append({"name": name, "inputs": [i for i, _, _ in parts], "dictionary": dec, "at": put(chunk),
                                "size": len(content), "md5": hashlib.md5(content).hexdigest()})
    verdicts, cases = {}, []
    for kind, chunk, cap, d in damaged_chunks(frames, dicts):   # (the chunks come back from the frames and the seed)
        got = D.arbiter(chunk, cap, d)
        verdicts.setdefault(kind, set()).add(got is not None)
        cases.append((chunk, cap, d))
        index["damaged"].append([kind, hashlib.md5(chunk + d).hexdigest()[:12], cap, None if got is None else len(got),
                                 None if got is None else hashlib.md5(got).hexdigest(), D.dictionary_verdict(d)])
    for kind, seen in sorted(verdicts.items()):
        assert seen == {True, False}, f"damage kind {kind}: libzstd's verdicts are {seen}"
    # the driver: the forms the set must hold, and its agreement with libzstd on every case
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp, sanitize=False)
        legal = [(frames[n][0], frames[n][1], dicts[dec]) for n, _, dec in frame_plans()]
        got = driver_results(run_driver(exe, tmp, "decode", driver_cases(legal)), len(legal))
        for (name, parts, dec), g in zip(frame_plans(), got):
            assert g[0] == b"".join(data[i] for i, _, _ in parts), f"the driver does not decode {name}"
        assert any(g[3] & 1 for g in got), "no frame whose first block has Treeless literals"
        assert any(g[3] & 14 for g in got), "no frame with a Repeat_Mode table in its first block"
        assert any(g[1] for g in got) and any(g[2] for g in got), "no match that begins in the dictionary / crosses into the output"
        got = driver_results(run_driver(exe, tmp, "decode", driver_cases(cases)), len(cases))
        differ = [(i, e[0]) for i, (e, g) in enumerate(zip(index["damaged"], got))
                  if (None if g[0] is None else hashlib.md5(g[0]).hexdigest()) != e[4]]
        assert not differ, f"cases on which the driver and libzstd differ (choose another DAMAGE_SEED): {differ}"
    return index, bytes(blob)


def load():
    """-> (dictionaries {name: bytes}, frames [(name, chunk, content, dictionary name)],
    damaged [(kind, chunk, capacity, dictionary bytes, size or None, md5 or None, libzstd loads the dictionary?)])"""
    with open(os.path.join(DIR, "fixture.json")) as f:
        index = json.load(f)
    with open(os.path.join(DIR, "fixture.bin"), "rb") as f:
        blob = f.read()
    cut = lambda at: blob[at[0]:at[0] + at[1]]
    dicts = {name: cut(at) for name, at in index["dictionaries"].items()}
    data = inputs(dicts)
    frames = []
    for e in index["frames"]:
        content = b"".join(data[i] for i in e["inputs"])
        assert hashlib.md5(content).hexdigest() == e["md5"], "inputs() no longer makes the fixture's content"
        frames.append((e["name"], cut(e["at"]), content, e["dictionary"]))
    sources = {n: (c, len(d)) for n, c, d, _ in frames}
    chunks = damaged_chunks(sources, dicts)
    assert len(chunks) == len(index["damaged"])
    damaged = []
    for (kind, chunk, cap, d), e in zip(chunks, index["damaged"]):
        assert [kind, hashlib.md5(chunk + d).hexdigest()[:12], cap] == e[:3], "the damage is no longer the fixture's"
        damaged.append((kind, chunk, cap, d, e[3], e[4], e[5]))
    return dicts, frames, damaged


if __name__ == "__main__":
    index, blob = make()
    os.makedirs(DIR, exist_ok=True)
    with open(os.path.join(DIR, "fixture.json"), "w") as f:
        json.dump(index, f, separators=(",", ":"))
    with open(os.path.join(DIR, "fixture.bin"), "wb") as f:
        f.write(blob)
    acc = sum(e[3] is not None for e in index["damaged"])
    print(f"{len(index['frames'])} frames, {len(index['damaged'])} damaged ({acc} accepted by libzstd), {len(blob)} bytes")
