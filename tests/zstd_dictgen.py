"""Planned dictionaries and planned frames that use them, for the Zstandard decoder with dictionaries
(include/hipcomp/zstd_dict.h).  The sibling of tests/zstd_framegen.py, whose writers it uses: a dictionary is written
from chosen tables, repeat offsets and content, a frame from a plan against a dictionary, so the expected bytes are
known by construction.  libzstd (libzstd.so.1 through ctypes) is the arbiter: arbiter(chunk, capacity, dictionary)
is ZSTD_decompress_usingDict, dictionary_verdict(dictionary) what it says of a dictionary alone.

Plain Python; importing it needs neither a GPU nor libzstd."""
from __future__ import annotations

import ctypes
import struct

import zstd_framegen as G
from zstd_framegen import FSE, PREDEFINED, REPEAT

DICT_MAGIC = 0xEC30A437
NO_DICT = None          # a chunk without a dictionary (a null blob)


# ------------------------------------------------------------------------------------------------------ libzstd
_bound = False


def libzstd():
    global _bound
    z = G.libzstd()
    if z is not None and not _bound:
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        z.ZSTD_createDCtx.restype = z.ZSTD_createCCtx.restype = vp
        z.ZSTD_freeDCtx.argtypes = z.ZSTD_freeCCtx.argtypes = [vp]
        z.ZSTD_decompress_usingDict.restype = z.ZSTD_compress_usingDict.restype = sz
        z.ZSTD_decompress_usingDict.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, sz, ctypes.c_char_p, sz]
        z.ZSTD_compress_usingDict.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, sz, ctypes.c_char_p, sz, ctypes.c_int]
        z.ZDICT_trainFromBuffer.restype = sz
        z.ZDICT_trainFromBuffer.argtypes = [ctypes.c_char_p, sz, ctypes.c_char_p, ctypes.POINTER(sz), ctypes.c_uint]
        z.ZDICT_isError.restype = ctypes.c_uint
        z.ZDICT_isError.argtypes = [sz]
        z.ZDICT_getDictID.restype = ctypes.c_uint
        z.ZDICT_getDictID.argtypes = [ctypes.c_char_p, sz]
        _bound = True
    return z


def arbiter(chunk: bytes, capacity: int, dictionary):
    """ZSTD_decompress_usingDict of the chunk into `capacity` bytes: the content, or None where libzstd refuses.
    dictionary None: no dictionary."""
    z = libzstd()
    ctx = z.ZSTD_createDCtx()
    buf = ctypes.create_string_buffer(max(capacity, 1))
    d = dictionary or b""
    n = z.ZSTD_decompress_usingDict(ctx, buf, capacity, chunk, len(chunk), d if d else None, len(d))
    z.ZSTD_freeDCtx(ctx)
    return None if z.ZSTD_isError(n) else buf.raw[:n]


def compress(data: bytes, level: int, dictionary: bytes) -> bytes:
    z = libzstd()
    ctx = z.ZSTD_createCCtx()
    buf = ctypes.create_string_buffer(z.ZSTD_compressBound(len(data)))
    n = z.ZSTD_compress_usingDict(ctx, buf, len(buf), data, len(data), dictionary if dictionary else None, len(dictionary), level)
    z.ZSTD_freeCCtx(ctx)
    assert not z.ZSTD_isError(n)
    return buf.raw[:n]


def train(samples, dict_bytes: int) -> bytes:
    z = libzstd()
    sizes = (ctypes.c_size_t * len(samples))(*[len(s) for s in samples])
    buf = ctypes.create_string_buffer(dict_bytes)
    n = z.ZDICT_trainFromBuffer(buf, dict_bytes, b"".join(samples), sizes, len(samples))
    assert not z.ZDICT_isError(n), "ZDICT_trainFromBuffer failed"
    return buf.raw[:n]


PROBE = G.frame([("raw", b"probe")])[0]


def dictionary_verdict(dictionary: bytes) -> bool:
    """True where libzstd loads the dictionary: a frame that needs nothing from it decodes with it."""
    return arbiter(PROBE, 16, dictionary) == b"probe"


# ------------------------------------------------------------------------------------------------- dictionaries
TEXT = b"It was the best of times, it was the worst of times, it was the age of wisdom, it was the age of foolishness. " * 12
OF_NORM = ([4] * 16, 6)                                     # offset codes 0 .. 15
ML_NORM = ([24] + [2] * 52, 7)                              # every match length code
LL_NORM = ([29] + [1] * 35, 6)                              # every literal length code


class Dict:
    """A dictionary and what a frame writer needs of it.  formatted() / raw() make one."""

    def __init__(self, data, content, dict_id=0, rep=(1, 4, 8), tables=None, codes=None, sections=None):
        self.bytes, self.content, self.dict_id, self.rep = bytes(data), bytes(content), dict_id, tuple(rep)
        self.tables, self.codes = tables, codes       # SeqCoder tables, Huffman codes: None for raw content
        self.sections = sections or []                # the byte offsets at which its sections start and end

    @property
    def is_formatted(self):
        return self.tables is not None


def raw(content: bytes) -> Dict:
    return Dict(content, content)


def formatted(content=TEXT[:600], dict_id=0x1234ABCD, rep=(5, 17, 300), huffman_text=TEXT, weights="fse", of=OF_NORM, ml=ML_NORM,
              ll=LL_NORM, weights_override=None) -> Dict:
    w, log = G.huf_weights(G.huf_lengths(huffman_text))
    if weights_override is not None:
        w, log = weights_override
    desc = G.weights_direct(w) if weights == "direct" else G.weights_fse(w, 6)
    parts = [struct.pack("<II", DICT_MAGIC, dict_id), desc, G.write_ncount(*of), G.write_ncount(*ml), G.write_ncount(*ll),
             struct.pack("<III", *rep), content]
    sections, at = [], 0
    for part in parts:
        at += len(part)
        sections.append(at)
    tables = {"of": (G.fse_table(*of), of[1]), "ml": (G.fse_table(*ml), ml[1]), "ll": (G.fse_table(*ll), ll[1])} \
        if all(sum(abs(c) for c in t[0]) == 1 << t[1] for t in (of, ml, ll)) else {}
    codes = G.huf_codes(w, log) if log <= 11 else {}
    return Dict(b"".join(parts), content, dict_id, rep, tables, codes, sections)


def execute(history: bytearray, literals: bytes, sequences, rep):
    """zstd_framegen.execute with the dictionary as history (frame_start 0) and libzstd's rule that a repeat offset of
    rep[0] - 1 == 0 means 1; appends to history, updates rep."""
    lit = 0
    for ll, ml, ov in sequences:
        history += literals[lit:lit + ll]
        lit += ll
        if ov > 3:
            off = ov - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ov - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = (rep[0] - 1 if idx == 3 else rep[idx]) or 1
                rep[:] = [off, rep[0], rep[1]] if idx >= 2 else [off, rep[0], rep[2]]
        assert 0 < off <= len(history), "an offset before the dictionary's start"
        for _ in range(ml):
            history.append(history[-off])
    history += literals[lit:]


def frame(d, blocks, dict_id=None, declare=True, checksum=False, check=True):
    """A frame against dictionary d (a Dict, or None).  blocks as for zstd_framegen.frame; a "seq" block's literals part
    may be the string "treeless" (the literals coded with the dictionary's Huffman codes, 4 streams) or "treeless1".
    check False: the plan is illegal, its content is not computed.  -> (frame, content)"""
    content = d.content if d else b""
    history, rep, coder, body = bytearray(content), list(d.rep if d else (1, 4, 8)), G.SeqCoder(), b""
    if d and d.is_formatted:
        coder.tables = dict(d.tables)
    for i, b in enumerate(blocks):
        last = i + 1 == len(blocks)
        if b[0] == "raw":
            history += b[1]
            body += G.block(0, b[1], last)
        elif b[0] == "rle":
            history += bytes([b[1]]) * b[2]
            body += G.block(1, bytes([b[1]]), last, b[2])
        else:
            _, lit_section, lits, seqs, kw = b
            if lit_section in ("treeless", "treeless1"):
                lit_section = G.literals_huffman(lits, 1 if lit_section == "treeless1" else 4, None, b"", d.codes, treeless=True)
            if check:
                execute(history, lits, seqs, rep)
            body += G.block(2, lit_section + coder.section(seqs, **kw), last)
    out = bytes(history[len(content):])
    head = G.frame_header(len(out) if declare and check else None, checksum=checksum, dict_id=dict_id)
    tail = struct.pack("<I", G.xxh64(out) & 0xFFFFFFFF) if checksum else b""
    return head + body + tail, out


def second_formatted() -> Dict:
    return formatted(dict_id=99, content=TEXT[100:500], rep=(7, 2, 1))


def offset_one_formatted() -> Dict:
    """its first repeat offset is 1: rep[0] - 1 is the zero case"""
    return formatted(rep=(1, 4, 8), dict_id=5)


def planned_dictionaries():
    """-> [(name, dictionary bytes, legal?)]: legal is what the rules of include/hipcomp/zstd_dict.h say; the CPU test holds
    every one of them to libzstd."""
    good = formatted()
    out = [("formatted", good.bytes, True), ("formatted_direct_weights", formatted(weights="direct", dict_id=77).bytes, True),
           ("raw_content", TEXT[:300], True), ("empty", b"", True), ("magic_and_id_only", good.bytes[:8], False),
           ("raw_with_magic_elsewhere", b"x" + good.bytes, True), ("second_formatted", second_formatted().bytes, True),
           ("repeat_offsets_1_4_8", offset_one_formatted().bytes, True)]
    out += [(f"raw_{n}_bytes", good.bytes[:n], True) for n in range(1, 8)]
    names = ("id", "huffman", "of", "ml", "ll", "repeat_offsets")
    for name, at in zip(names, good.sections):
        for cut in (at - 1, at, at + 1):
            if cut > 8:
                out.append((f"cut_{name}{cut - at:+d}", good.bytes[:cut], False))
    n = len(TEXT[:600])
    for name, rep, legal in (("rep_zero", (5, 0, 300), False), ("rep_is_content_size", (n, 17, 1), True),
                             ("rep_past_content", (5, 17, n + 1), False), ("rep_first_zero", (0, 1, 1), False)):
        out.append((name, formatted(rep=rep).bytes, legal))
    out.append(("content_of_one_byte", formatted(content=b"z", rep=(1, 1, 1)).bytes, True))
    out.append(("no_content", formatted(content=b"", rep=(1, 1, 1)).bytes, False))
    # each table's largest symbol and accuracy log, at the limit and one above
    for name, key, syms, log in (("of", "of", 32, 8), ("ml", "ml", 53, 9), ("ll", "ll", 36, 9)):
        def table(nsym, lg):
            norm = [1] * nsym
            norm[0] = (1 << lg) - (nsym - 1)
            return (norm, lg)
        out.append((f"{name}_at_the_limits", formatted(**{key: table(syms, log)}).bytes, True))
        out.append((f"{name}_symbol_too_large", formatted(**{key: table(syms + 1, log)}).bytes, False))
        out.append((f"{name}_log_too_large", formatted(**{key: table(syms, log + 1)}).bytes, False))
    # weights 2 and 3 and the implied 2: no symbol of weight 1
    out.append(("huffman_weights_sum", good.bytes[:8] + bytes([128 + 1, 0x23]) + good.bytes[good.sections[1]:], False))
    # code lengths 1, 2, .. 11, 12, 12: a tree of depth 12 is refused in a dictionary as it is in a block
    lengths = {s: min(s + 1, 12) for s in range(13)}
    out.append(("huffman_depth_12", formatted(weights="direct", weights_override=G.huf_weights(lengths)).bytes, False))
    return out


# ------------------------------------------------------------------------------------------------------- frames
def small_formatted() -> bytes:
    """a small legal formatted dictionary: every prefix of it is a case"""
    return formatted(content=TEXT[:40], rep=(3, 9, 40), huffman_text=b"abcabcaabdd", weights="direct").bytes


def planned_frames():
    """-> [(name, chunk, dictionary bytes or None, content or None)]: content None means the plan is illegal.  The CPU
    test asserts libzstd's verdict and bytes on every one."""
    fd, fd2, rd = formatted(), second_formatted(), raw(TEXT[:300])
    n = len(fd.content)
    lits = TEXT[700:900]
    out = []

    def add(name, d, blocks, **kw):
        legal = kw.pop("legal", True)
        given = kw.pop("given", d)
        chunk, content = frame(d, blocks, check=legal, **kw)
        out.append((name, chunk, None if given is None else given.bytes, content if legal else None))
    seq = [(5, 10, 3 + 40), (3, 6, 3 + 9)]
    add("treeless_first_block", fd, [("seq", "treeless", lits, seq, {})], dict_id=fd.dict_id)
    add("treeless_one_stream", fd, [("seq", "treeless1", lits[:90], seq, {})])
    for name, modes in (("ll", (REPEAT, PREDEFINED, PREDEFINED)), ("of", (PREDEFINED, REPEAT, PREDEFINED)),
                        ("ml", (PREDEFINED, PREDEFINED, REPEAT)), ("all", (REPEAT, REPEAT, REPEAT))):
        add(f"repeat_mode_{name}", fd, [("seq", G.literals_raw(lits), lits, seq * 3, dict(modes=modes))], dict_id=fd.dict_id)
    add("repeat_then_describe_then_repeat", fd, [("seq", "treeless", lits, seq, dict(modes=(REPEAT, REPEAT, REPEAT))),
                                                 ("seq", G.literals_raw(lits), lits, seq * 9, dict(modes=(FSE, REPEAT, FSE), logs=(6, 6, 6))),
                                                 ("seq", "treeless", lits, seq, dict(modes=(REPEAT, REPEAT, REPEAT)))], declare=False)
    # the first sequence coded as a repeat offset, with and without literals; rep[0] - 1 and its zero case
    one = offset_one_formatted()
    for ov in (1, 2, 3):
        for ll in (0, 5):
            add(f"first_sequence_repeat_{ov}_ll_{ll}", fd, [("seq", G.literals_raw(lits), lits, [(ll, 8, ov), (2, 5, 1)], {})])
            add(f"first_sequence_repeat_{ov}_ll_{ll}_raw_dictionary", rd, [("seq", G.literals_raw(lits), lits, [(ll, 8, ov), (2, 5, 1)], {})])
    add("first_sequence_repeat_3_ll_0_of_offset_one", one, [("seq", G.literals_raw(lits), lits, [(0, 8, 3), (2, 5, 1)], {})])
    # where a match lies
    for d, tag in ((fd, "formatted"), (rd, "raw")):
        m = len(d.content)
        add(f"match_wholly_in_dictionary_{tag}", d, [("seq", G.literals_raw(lits), lits, [(5, 10, 3 + 5 + 100)], {})])
        add(f"match_ends_at_dictionary_end_{tag}", d, [("seq", G.literals_raw(lits), lits, [(5, 10, 3 + 5 + 10)], {})])
        add(f"match_crosses_into_output_{tag}", d, [("seq", G.literals_raw(lits), lits, [(20, 10, 3 + 20 + 4)], {})])
        add(f"match_crosses_and_overruns_itself_{tag}", d, [("seq", G.literals_raw(lits), lits, [(2, 200, 3 + 2 + 3)], {})])
        add(f"match_of_the_whole_dictionary_and_more_{tag}", d, [("seq", G.literals_raw(lits), lits, [(7, m + 90, 3 + 7 + m)], {})])
        add(f"farthest_offset_{tag}", d, [("seq", G.literals_raw(lits), lits, [(9, 12, 3 + 9 + m)], {})])
        add(f"offset_one_beyond_{tag}", d, [("seq", G.literals_raw(lits), lits, [(9, 12, 3 + 9 + m + 1)], {})], legal=False)
        add(f"second_block_reaches_the_dictionary_{tag}", d, [("raw", TEXT[:70]), ("seq", G.literals_raw(lits), lits, [(4, 30, 3 + 70 + 4 + 50)], {})])
        add(f"second_block_one_beyond_{tag}", d, [("raw", TEXT[:70]), ("seq", G.literals_raw(lits), lits, [(4, 30, 3 + 70 + 4 + m + 1)], {})], legal=False)
        for c in (0, 1, 7, 15):        # matches that begin at content[16 k + c]
            add(f"match_begins_at_content_{c}_mod_16_{tag}", d, [("seq", G.literals_raw(lits), lits, [(3, 70, 3 + 3 + m - (64 + c))], {})])
    add("many_matches_in_the_dictionary", fd, [("seq", G.literals_raw(lits), lits, [(1, 3 + k % 30, 3 + 1 + 7 * k % 500) for k in range(150)],
                                                dict(modes=(REPEAT, REPEAT, REPEAT)))], checksum=True, dict_id=fd.dict_id)
    # two frames in a chunk: each starts again from the dictionary
    a = frame(fd, [("seq", "treeless", lits, [(5, 10, 3 + 5 + 100)], dict(modes=(REPEAT, REPEAT, REPEAT)))], dict_id=fd.dict_id)
    b = frame(fd, [("seq", "treeless", lits[:60], [(6, 20, 3 + 6 + n)], dict(modes=(REPEAT, REPEAT, REPEAT)))], checksum=True)
    out.append(("two_frames_both_reach_the_dictionary", a[0] + G.skippable(b"between") + b[0], fd.bytes, a[1] + b[1]))
    bad = frame(fd, [("seq", G.literals_raw(lits), lits, [(6, 20, 3 + 6 + n + 1)], {})], check=False)
    out.append(("second_frame_reaches_the_first_frames_output", a[0] + bad[0], fd.bytes, None))
    # the dictionary's tables with a dictionary that has none
    for name, d in (("raw_dictionary", rd), ("no_dictionary", None), ("empty_dictionary", raw(b""))):
        c1 = frame(fd, [("seq", "treeless", lits, [], {})])[0]
        c2 = frame(fd, [("seq", G.literals_raw(lits), lits, seq, dict(modes=(REPEAT, PREDEFINED, PREDEFINED)))])[0]
        out += [(f"treeless_with_{name}", c1, None if d is None else d.bytes, None),
                (f"repeat_mode_with_{name}", c2, None if d is None else d.bytes, None)]
    # Dictionary_ID
    plain = [("raw", TEXT[:50]), ("seq", G.literals_raw(lits), lits, [(5, 10, 3 + 5)], {})]
    add("dictionary_id_equal", fd, plain, dict_id=fd.dict_id)
    add("dictionary_id_different", fd, plain, dict_id=fd.dict_id + 1, legal=False)
    add("dictionary_id_zero", fd, plain, dict_id=0)
    add("dictionary_id_absent", fd, plain)
    add("dictionary_id_of_another_dictionary", fd2, plain, dict_id=fd2.dict_id, given=fd, legal=False)
    add("dictionary_id_against_raw_content", rd, plain, dict_id=7, legal=False)
    add("dictionary_id_without_a_dictionary", None, plain, dict_id=7, legal=False)
    add("dictionary_id_zero_against_raw_content", rd, plain, dict_id=0)
    add("no_dictionary_needed_formatted_given", None, plain, given=fd)
    add("tables_first_used_in_the_second_block", fd, [("seq", G.literals_raw(lits), lits, [], {}),
                                                      ("seq", "treeless", lits, seq, dict(modes=(REPEAT, REPEAT, REPEAT)))])
    add("undeclared_size_with_dictionary", fd, [("seq", "treeless", lits, [(5, 10, 3 + 5 + 100)], {})], declare=False)
    add("undeclared_size_offset_beyond", fd, [("seq", G.literals_raw(lits), lits, [(9, 12, 3 + 9 + n + 1)], {})], declare=False, legal=False)
    # a frame against a dictionary that is refused
    out.append(("dictionary_refused", frame(None, plain)[0], formatted(rep=(5, 0, 300)).bytes, None))
    return out
