"""What the tests of the Zstandard encoder with dictionaries (include/hipcomp/zstd_dict_compress.h) share: the CPU
driver of csrc/zstd_dict_compress/zstd_dict_codes.hpp (tests/zstd_dict_codes_driver.cpp, a stand-alone program built
with the sanitizers), a reader of the frames the encoder writes -- tests/zstd_seqscan.py's with the Dictionary_ID
field, Treeless literals and Repeat_Mode -- the restated definitions of the blob, and the planned cases.

Plain Python; importing it needs neither a GPU nor libzstd."""
from __future__ import annotations

import os
import random
import struct
import subprocess

import zstd_dict_fixtures as F
import zstd_dictgen as D
import zstd_framegen as G
import zstd_seqscan as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAX_CHUNK = 32768
MAX_TAIL = 32768
BASE = 14080            # HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES
TABLE_AT, TABLES_AT = 64, 64 + 8192
TREELESS, REPEAT = 3, 3


# ---------------------------------------------------------------------------------------------- restated definitions
def prepared_size(dict_bytes: int) -> int:
    return BASE + (min(dict_bytes, MAX_TAIL) + 15) // 16 * 16


def tail_len(content_size: int) -> int:
    return 0 if content_size < 8 else min(content_size, MAX_TAIL)


def hash_of(v: int) -> int:
    return ((v * 0x9E3779B1) & 0xFFFFFFFF) >> 20


def prime_table(tail: bytes):
    """slot h: the greatest v in [0, T - 4] whose 4 bytes hash to h, 0 where there is none"""
    table = [0] * 4096
    for v in range(len(tail) - 3):
        h = hash_of(int.from_bytes(tail[v:v + 4], "little"))
        table[h] = max(table[h], v)
    return table


def dict_model(d: bytes):
    """-> what a frame reader needs of a dictionary the encoder accepted: id, rep, content, and for a formatted one
    norms = {"ll" / "of" / "ml": (norm, log)}"""
    if len(d) < 8 or struct.unpack_from("<I", d)[0] != D.DICT_MAGIC:
        return {"id": 0, "rep": (1, 4, 8), "content": d, "norms": None}
    at = 8
    hb = d[at]
    at += 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
    norms = {}
    for key, max_sym in (("of", 31), ("ml", 52), ("ll", 35)):
        norm, log, used = S.read_ncount(d[at:at + 200], max_sym)
        norms[key] = (norm, log)
        at += used
    return {"id": struct.unpack_from("<I", d, 4)[0], "rep": struct.unpack_from("<III", d, at), "content": d[at + 12:], "norms": norms}


# --------------------------------------------------------------------------------------------------- the driver
def build_driver(directory) -> str:
    exe = os.path.join(directory, "zstd_dict_codes_driver")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include")]
    csrc = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
    for sub in ("", "zstd", "zstd_compress", "zstd_dict", "deflate_compress", "deflate"):
        cmd += ["-I", os.path.join(csrc, sub)]
    r = subprocess.run(cmd + [os.path.join(HERE, "zstd_dict_codes_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_driver(exe, directory, mode, payload: bytes) -> bytes:
    return F.run_driver(exe, directory, mode, payload)


def prepare(exe, directory, dicts):
    """-> [(status, blob)]: status 0 and the whole blob, or 1 and the 64-byte header"""
    blob = run_driver(exe, directory, "prepare", F.prepare_cases(dicts))
    out, at = [], 0
    for _ in dicts:
        status, size = struct.unpack_from("<IQ", blob, at)
        out.append((status, blob[at + 12:at + 12 + size]))
        at += 12 + size
    assert at == len(blob)
    return out


def encode(exe, directory, cases):
    """cases: [(content, tokens [(ll, ml, offset)], dictionary bytes or None, checksum)] -> [frame or None (refused)]"""
    payload = b""
    for content, tokens, d, checksum in cases:
        payload += struct.pack("<IIII", (1 if checksum else 0) | (2 if d is not None else 0), len(d or b""), len(content), len(tokens))
        payload += (d or b"") + content + b"".join(struct.pack("<III", *t) for t in tokens)
    blob = run_driver(exe, directory, "encode", payload)
    out, at = [], 0
    for _ in cases:
        size, = struct.unpack_from("<I", blob, at)
        out.append(blob[at + 4:at + 4 + size] if size else None)
        at += 4 + size
    assert at == len(blob)
    return out


# ------------------------------------------------------------------------------------------------- the frame reader
def frame_info(frame: bytes, model=None):
    """One single-segment frame of one block -> {"id_bytes", "dict_id", "checksum", "block" (0 raw, 1 RLE, 2 compressed),
    and for a compressed block "lit_type", "lit_streams", "modes" (LL, OF, ML; () without sequences), "seqs" [(ll, ml, Offset_Value)]}.
    model: dict_model of the dictionary, for Repeat_Mode tables."""
    assert frame[:4] == struct.pack("<I", 0xFD2FB528)
    fhd = frame[4]
    assert fhd >> 5 & 1 and not fhd & 0x18
    idb = (0, 1, 2, 4)[fhd & 3]
    fcs = 1 if fhd >> 6 == 0 else 1 << (fhd >> 6)
    out = {"id_bytes": idb, "dict_id": int.from_bytes(frame[5:5 + idb], "little"), "checksum": bool(fhd & 4)}
    at = 5 + idb + fcs
    h = int.from_bytes(frame[at:at + 3], "little")
    assert h & 1
    out["block"] = kind = h >> 1 & 3
    size = 1 if kind == 1 else h >> 3
    assert len(frame) == at + 3 + size + (4 if out["checksum"] else 0)
    if kind != 2:
        return out
    b = frame[at + 3:at + 3 + size]
    t, sf = b[0] & 3, b[0] >> 2 & 3
    out["lit_type"] = t
    if t < 2:
        hb = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = b[0] >> 3 if hb == 1 else int.from_bytes(b[:hb], "little") >> 4
        lit_end = hb + (regen if t == 0 else 1)
        out["lit_streams"] = 1
    else:
        hb = 3 if sf < 2 else sf + 2
        lhc = int.from_bytes(b[:5], "little")
        lit_end = hb + {3: lhc >> 14 & 0x3FF, 4: lhc >> 18 & 0x3FFF, 5: lhc >> 22 & 0x3FFFF}[hb]
        out["lit_streams"] = 1 if sf == 0 else 4
    s = b[lit_end:]
    n, p = s[0], 1
    if n == 0:
        assert len(s) == 1
        out["modes"], out["seqs"] = (), []
        return out
    if n >= 128:
        assert n < 255
        n, p = ((n - 128) << 8) + s[1], 2
    modes = s[p]
    p += 1
    out["modes"] = (modes >> 6, modes >> 4 & 3, modes >> 2 & 3)
    tables = []
    for mode, key, (dnorm, dlog), max_sym in zip(out["modes"], ("ll", "of", "ml"), (G.LL_DEFAULT, G.OF_DEFAULT, G.ML_DEFAULT), (35, 31, 52)):
        if mode == G.PREDEFINED:
            tables.append((G.fse_table(dnorm, dlog), dlog))
        elif mode == G.RLE:
            tables.append(([(s[p], 0, 0)], 0))
            p += 1
        elif mode == G.REPEAT:
            norm, log = model["norms"][key]
            tables.append((G.fse_table(norm, log), log))
        else:
            norm, log, used = S.read_ncount(s[p:], max_sym)
            tables.append((G.fse_table(norm, log), log))
            p += used
    (tll, lll), (tof, lof), (tml, lml) = tables
    r = S.BackReader(s[p:])
    sll, sof, sml = r.read(lll), r.read(lof), r.read(lml)
    seqs = []
    for k in range(n):
        lc, oc, mc = tll[sll][0], tof[sof][0], tml[sml][0]
        ov = (1 << oc) + r.read(oc)
        ml = G.ML_BASE[mc] + r.read(G.ML_BITS[mc])
        ll = G.LL_BASE[lc] + r.read(G.LL_BITS[lc])
        seqs.append((ll, ml, ov))
        if k + 1 < n:
            sll = tll[sll][2] + r.read(tll[sll][1])
            sml = tml[sml][2] + r.read(tml[sml][1])
            sof = tof[sof][2] + r.read(tof[sof][1])
    assert r.left == 0
    out["seqs"] = seqs
    return out


def tokens_of(info, rep0: int):
    """[(ll, ml, Offset_Value)] -> [(ll, ml, offset)] as this encoder codes offsets: value 1 is the offset before (rep0 in
    front of the first sequence) and stands only behind literals; 2 and 3 are never written.  None: no compressed block."""
    if info["block"] != 2:
        return None
    out, prev = [], rep0
    for ll, ml, ov in info["seqs"]:
        assert ov == 1 or ov > 3, "repeat offsets 2 and 3 are not used"
        assert not (ov == 1 and ll == 0)
        off = prev if ov == 1 else ov - 3
        out.append((ll, ml, off))
        prev = off
    return out


# ---------------------------------------------------------------------------------------------------- dictionaries
def skewed_text(n: int, seed: int) -> bytes:
    """letters of D.TEXT drawn at random: literals that the dictionary's Huffman code covers, with no structure to match"""
    rnd = random.Random(seed)
    return bytes(rnd.choice(D.TEXT) for _ in range(n))


def planned_dictionaries():
    """-> {name: bytes}, every one accepted: formatted ones at the tables' limits, with probabilities of -1, with repeat
    offsets at the edges, IDs of every field size, contents around the 8-byte and the 32 KiB edges"""
    rnd = random.Random(19)
    big = bytes(rnd.randrange(256) for _ in range(40000))
    minus = ([20] + [2] * 4 + [-1] * 30 + [6], 6)       # LL: 20 + 8 + 30 + 6 = 64, codes with probability -1
    assert sum(abs(c) for c in minus[0]) == 64 and len(minus[0]) == 36
    few_of = ([16] * 4, 6)                               # offset codes 0 .. 3 only: larger ones have probability 0

    def limits(nsym, lg):
        norm = [1] * nsym
        norm[0] = (1 << lg) - (nsym - 1)
        return (norm, lg)
    return {
        "formatted": D.formatted().bytes,
        "id_1_byte": D.formatted(dict_id=77, weights="direct").bytes,
        "id_2_bytes": D.formatted(dict_id=0x1234, rep=(1, 4, 8)).bytes,
        "id_zero": D.formatted(dict_id=0).bytes,
        "minus_one": D.formatted(dict_id=300, ll=minus).bytes,
        "few_offset_codes": D.formatted(dict_id=301, of=few_of).bytes,
        "limits": D.formatted(dict_id=302, of=limits(32, 8), ml=limits(53, 9), ll=limits(36, 9)).bytes,
        "rep_is_content_size": D.formatted(dict_id=303, rep=(600, 17, 1)).bytes,
        "content_7": D.formatted(dict_id=304, content=D.TEXT[:7], rep=(7, 1, 2)).bytes,
        "content_8": D.formatted(dict_id=305, content=D.TEXT[:8], rep=(8, 1, 2)).bytes,
        "content_32768": D.formatted(dict_id=306, content=big[:32768], rep=(5, 17, 300)).bytes,
        "content_40000": D.formatted(dict_id=307, content=big, rep=(5, 17, 300)).bytes,
        "raw_text": D.TEXT[:300],
        "raw_7": D.TEXT[:7],
        "raw_big": big,
        "raw_empty": b"",
    }
