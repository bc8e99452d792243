"""Plans that ask whether a decoder carries state from one chunk, frame or block into the next.

The four companion decoders (Deflate, gzip on top of it, Zstandard, Zstandard with dictionaries) keep their tables in
a wave's slice of LDS and walk a batch grid-stride: from its second trip on a wave decodes with the previous chunk's
tables, lengths, queue and literals still lying where it left them.  Both formats have streams that are illegal only
because a table is missing, and legal streams whose bytes change if an offset or a table leaks.  Here are

  * primers: small legal streams that leave as much behind as the format allows (and one each that fails late),
  * victims: every planned stream of tests/zstd_framegen.py, tests/deflate_streamgen.py and tests/zstd_dictgen.py of
    4 KiB or less, legal and illegal,
  * layout(): a batch of 3 W chunks, W the decoder's grid in waves, in which every wave decodes a primer, then a
    victim, then a legal victim, and every victim follows every primer on some wave,
  * the same question inside one chunk: a primer frame and a victim frame, a primer block and a victim block.

What is expected never comes from the library: a legal stream's bytes are planned, and tests/test_decoder_state_cpu.py
holds every expectation to libzstd and zlib.  Plain Python and numpy; importing it needs neither a GPU nor libzstd
(the dictionary victims ask libzstd for their bytes when they are built)."""
from __future__ import annotations

import functools
from collections import namedtuple

import deflate_streamgen as DG
import gzip_membergen as M
import zstd_dictgen as D
import zstd_framegen as G

# The decoders' grids in waves: a batch of more chunks is walked grid-stride.
DEFLATE_WAVES = 8192   # hipcomp-core_amd/csrc/deflate/deflate_kernels.hip: kMaxBlocks (256 * 32 / kWavesPerBlock) x kWavesPerBlock (4);
#                        gzip's verify kernel, csrc/gzip/gzip_kernels.hip: kMaxBlocks (256 * 8) x kWavesPerBlock (kBlock 256 / 64)
ZSTD_WAVES = 3072      # hipcomp-core_amd/csrc/zstd/zstd_sizing.hpp: kMaxWaves = 256 * groups_by_lds(4 * 12 KiB) * 4, both Zstandard decoders

PRIMER_CONTENT_MAX = 16 * 1024
VICTIM_MAX = 4 * 1024
REFUSED_ROOM = 64      # the capacity of a refused chunk where nothing says what it would have decoded to

# name; the chunk; its content, None for a chunk that is refused; room: the capacity it is given (the content's length,
# for a refused chunk what it would decode to were the missing piece there); dictionary: None, "A" or "B"
Stream = namedtuple("Stream", "name chunk content room dictionary")


def stream(name, chunk, content, room=None, dictionary=None):
    return Stream(name, bytes(chunk), None if content is None else bytes(content),
                  (REFUSED_ROOM if content is None else len(content)) if room is None else room, dictionary)


def is_legal(s):
    return s.content is not None


# ---------------------------------------------------------------------------------------------------- Zstandard
TEXT = b"It was the best of times, it was the worst of times, it was the age of wisdom. " * 220
ZSTD_STATE_SENSITIVE = ("repeat_mode_without_tables", "treeless_without_a_tree", "three_blocks_repeat_mode", "treeless_1_and_4_streams",
                        "repeat_code_1_ll_0", "repeat_code_1_ll_5", "repeat_code_2_ll_0", "repeat_code_2_ll_5", "repeat_code_3_ll_0",
                        "repeat_code_3_ll_5")
# what an illegal plan would decode to if the table it lacks were there: 200 literals and matches of 10 and 4; 20 literals
ZSTD_WOULD_BE = {"repeat_mode_without_tables": 214, "treeless_without_a_tree": 20}


def complete_lengths(nsym, maxbits):
    """nsym code lengths of a complete prefix code that reaches maxbits: the chain 1, 2, .. maxbits, maxbits, then the
    shortest code that can still be split is split until there are nsym"""
    lens = list(range(1, maxbits)) + [maxbits, maxbits]
    while len(lens) < nsym:
        lens.sort()
        v = lens.pop(next(i for i, x in enumerate(lens) if x < maxbits))
        lens += [v + 1, v + 1]
    assert len(lens) == nsym and sum(1 << (maxbits - v) for v in lens) == 1 << maxbits and max(lens) == maxbits
    return lens


def _spread(data):
    """the bytes of `data` in a fixed scattered order"""
    return bytes(b for _, b in sorted(enumerate(data), key=lambda p: (p[0] * 2654435761) & 0xFFFF))


def _huffman_section(data, streams=4, mode="fse"):
    w, log = G.huf_weights(G.huf_lengths(data))
    desc = G.weights_direct(w) if mode == "direct" else G.weights_fse(w, 6)
    return G.literals_huffman(data, streams, None, desc, G.huf_codes(w, log))


MANY = [(3, 4 + k % 9, 3 + 1 + k % 40) for k in range(100)]
MAX_LOGS = [(k % 17, 3 + k % 40, 3 + 1 + (k % 3 if k > 3 else 0)) for k in range(1, 121)]
MOVE_OFFSETS = [(10, 5, 3 + 7), (4, 6, 3 + 15), (3, 4, 3 + 9)]      # leaves the repeat offsets 9, 15, 7
FIRST_BLOCK = MANY + MOVE_OFFSETS + [(2, 5, 2)]                     # ... then 15, 9, 7; offset code 1 is in its table


@functools.lru_cache(maxsize=None)
def zstd_primer_plans():
    """-> [(name, the blocks of the primer's frame for zstd_framegen.frame, the Huffman codes it leaves or None)]"""
    lits = TEXT[:400]
    # a Huffman tree of depth 11 over 120 symbols, four streams; the weights are stored directly (120 of them: an
    # FSE-compressed description of so many weights does not fit its 127 bytes)
    lens = complete_lengths(120, 11)
    length = {s: lens[(s * 7) % 120] for s in range(120)}
    data = _spread(bytes(s for s in range(120) for _ in range(1 + (512 >> length[s]))))
    w, log = G.huf_weights(length)
    assert log == 11
    deep = G.huf_codes(w, log)
    out = [("huffman_depth_11_over_120_symbols", [("seq", G.literals_huffman(data, 4, None, G.weights_direct(w), deep), data, [(10, 5, 3 + 7)], {},
                                                   {"huffman_depth_11"})], deep),
           ("fse_tables_at_the_maximum_logs", [("seq", G.literals_raw(lits * 3), lits * 3, MAX_LOGS, dict(modes=(G.FSE, G.FSE, G.FSE), logs=(9, 8, 9)))], None),
           ("rle_modes", [("seq", G.literals_raw(lits), lits, [(2, 7, 3 + 2)] * 50, dict(modes=(G.RLE, G.RLE, G.RLE)))], None),
           ("repeat_offsets_9_15_7", [("seq", G.literals_raw(lits), lits, MOVE_OFFSETS, {})], None)]
    # literals that fill the wave's literal buffer: the tests size it for the largest chunk of the batch, these 16 KiB
    n = PRIMER_CONTENT_MAX
    w, log = G.huf_weights(G.huf_lengths(TEXT[:n]))
    codes = G.huf_codes(w, log)
    out += [("rle_literals_of_16k", [("seq", G.literals_rle(0x61, n, 3), b"a" * n, [], {})], None),
            ("huffman_literals_of_16k", [("seq", G.literals_huffman(TEXT[:n], 4, None, G.weights_fse(w, 6), codes), TEXT[:n], [], {})], codes)]
    # all of it in one frame: a tree, three described tables, moved offsets, and a second block that reuses them
    first, second = TEXT[:900], TEXT[900:1300]
    w, log = G.huf_weights(G.huf_lengths(first))
    codes = G.huf_codes(w, log)
    assert set(second) <= set(codes)
    fse = dict(modes=(G.FSE, G.FSE, G.FSE), logs=(6, 6, 7))
    out.append(("tree_tables_and_offsets_reused",
                [("seq", G.literals_huffman(first, 4, None, G.weights_fse(w, 6), codes), first, FIRST_BLOCK, fse),
                 ("seq", G.literals_huffman(second, 4, None, b"", codes, treeless=True), second, [(3, 12, 2)] + MANY, dict(modes=(G.REPEAT,) * 3))], codes))
    return out


@functools.lru_cache(maxsize=None)
def zstd_primers():
    """-> [Stream]: legal frames that leave tables, offsets and literals behind, and one that fails late"""
    out = []
    for name, blocks, _ in zstd_primer_plans():
        fr = G.frame(blocks)
        assert len(fr[1]) <= PRIMER_CONTENT_MAX, name
        out.append(stream(name, fr[0], fr[1]))
    # fails late: the first block of the last primer, which builds a tree and three tables, then its second block cut short
    (_, lit1, first, seq1, fse), (_, lit2, second, _, repeat) = zstd_primer_plans()[-1][1]
    coder = G.SeqCoder()
    body = G.block(2, lit1 + coder.section(seq1, **fse), False)
    cut = G.block(2, lit2 + coder.section(MANY, **repeat), True)
    history = bytearray()
    G.execute(history, 0, first, seq1, [1, 4, 8])
    out.append(stream("fails_in_the_second_block", G.frame_header(None, window_log=17) + body + cut[:len(cut) // 2], None, room=len(history)))
    return out


def _one_block(payload: bytes) -> bytes:
    """a frame without a declared size whose one block is a compressed block"""
    return G.frame_header(None, window_log=17) + G.block(2, payload, True)


@functools.lru_cache(maxsize=None)
def zstd_leak_plans():
    """Chunks written so that what one primer leaves behind would show.  -> [(Stream, primer name or None, the block for
    zstd_framegen.frame or None)].  Legal: a frame whose first sequence is a repeat code, which must see the offsets 1, 4
    and 8 (its bytes change with any others).  Illegal: a block that is legal as the NEXT block of a primer's frame and
    nowhere else -- treeless literals coded with the primer's tree, sequences in Repeat_Mode coded with the primer's three
    tables -- alone in a frame of its own.  A decoder that finds the primer's tree or tables in LDS decodes it without
    complaint, to `room` bytes (the planned illegal frames of tests/zstd_framegen.py lack a table too, but their
    bitstreams fit no table that a primer leaves: they are refused either way)."""
    out = []
    text, lits = TEXT[:50], TEXT[100:300]
    for ov in (1, 2, 3):
        for ll in (0, 5):
            if (ov, ll) != (3, 0):      # (repeat code 3 without literals is the first offset - 1: no offset at all)
                fr = G.frame([("raw", text), ("seq", G.literals_raw(lits), lits, [(ll, 8, ov), (2, 5, 1)], {})])
                out.append((stream(f"first_sequence_is_repeat_code_{ov}_ll_{ll}", fr[0], fr[1]), None, None))
    for name, blocks, codes in zstd_primer_plans():
        if codes:
            data = bytes(sorted(codes)[(7 * i) % len(codes)] for i in range(150))
            section = G.literals_huffman(data, 4, None, b"", codes, treeless=True)
            out.append((stream(f"treeless_with_the_tree_of_{name}", _one_block(section + b"\x00"), None, room=len(data)), name, ("seq", section, data, [], {})))
        coder, described = G.SeqCoder(), None
        for b in blocks:
            if b[3]:
                coder.section(b[3], **b[4])
                if b[4].get("modes", (G.PREDEFINED,))[0] != G.REPEAT:
                    described = b
        if described:       # the first sequences of the block that set the tables up, in Repeat_Mode: the same codes, explicit offsets
            seqs = described[3][:20]
            own = described[2][:sum(q[0] for q in seqs) + 7]
            would_be = bytearray()
            G.execute(would_be, 0, own, seqs, [1, 4, 8])
            payload = G.literals_raw(own) + coder.section(seqs, modes=(G.REPEAT,) * 3)
            out.append((stream(f"repeat_mode_with_the_tables_of_{name}", _one_block(payload), None, room=len(would_be)), name,
                        ("seq", G.literals_raw(own), own, seqs, dict(modes=(G.REPEAT,) * 3))))
    return out


def zstd_sensitive_names():
    return ZSTD_STATE_SENSITIVE + tuple(v.name for v, _, _ in zstd_leak_plans())


@functools.lru_cache(maxsize=None)
def zstd_victims():
    """-> ([Stream], names left out): every legal and illegal plan and the documented differences, of 4 KiB or less,
    then the chunks of zstd_leak_plans()"""
    out, left_out = [], []
    for name, chunk, content, _ in G.legal_plans():
        if len(chunk) <= VICTIM_MAX and len(content) <= VICTIM_MAX:
            out.append(stream(name, chunk, content))
        else:
            left_out.append(name)
    for name, chunk in G.illegal_plans() + G.documented_differences():
        if len(chunk) <= VICTIM_MAX:
            out.append(stream(name, chunk, None, room=ZSTD_WOULD_BE.get(name)))
        else:
            left_out.append(name)
    return out + [v for v, _, _ in zstd_leak_plans()], left_out


@functools.lru_cache(maxsize=None)
def zstd_within_chunk():
    """-> [Stream]: a primer frame, then a state-sensitive victim frame, in one chunk; the same with a skippable frame
    between the two.  Refused where either frame is."""
    victims = {v.name: v for v in zstd_victims()[0]}
    out = []
    for p in zstd_primers():
        for name in zstd_sensitive_names():
            v = victims[name]
            for tag, between in (("", b""), ("_skippable_between", G.skippable(b"between the two"))):
                legal = is_legal(p) and is_legal(v)
                out.append(stream(f"{p.name}+{name}{tag}", p.chunk + between + v.chunk, p.content + v.content if legal else None,
                                  room=p.room + v.room))
    return out


# ------------------------------------------------------------------------------------------------ dictionaries
def dictionary_a() -> D.Dict:
    """the dictionary the planned frames of tests/zstd_dictgen.py are written against"""
    return D.formatted()


def dictionary_b() -> D.Dict:
    """other tables (all four), other repeat offsets, another ID and other content"""
    return D.formatted(content=D.TEXT[50:450], dict_id=0x0B0B0B, rep=(9, 33, 2), huffman_text=b"the quick brown fox jumps over the lazy dog " * 9 + D.TEXT[:300],
                       of=([8] * 4 + [2] * 16, 6), ml=([76] + [1] * 52, 7), ll=([15, 15] + [1] * 34, 6))


@functools.lru_cache(maxsize=None)
def dictionaries():
    return {"A": dictionary_a(), "B": dictionary_b()}


DICT_SEQ = [(5, 10, 3 + 40), (3, 6, 3 + 9), (0, 7, 2), (4, 9, 3 + 33)]
REPEAT_ALL = dict(modes=(G.REPEAT, G.REPEAT, G.REPEAT))


@functools.lru_cache(maxsize=None)
def dict_primers():
    """-> [Stream]: for each dictionary a frame that repeats all four of its tables and moves its repeat offsets, then
    the plain Zstandard primers, which need no dictionary and are given A"""
    out = []
    for key, d in dictionaries().items():
        lits = bytes(b for b in D.TEXT[700:1000] if b in d.codes)[:200]
        chunk, content = D.frame(d, [("seq", "treeless", lits, DICT_SEQ * 3, REPEAT_ALL)], dict_id=d.dict_id)
        out.append(stream(f"repeats_the_four_tables_of_{key}", chunk, content, dictionary=key))
    return out + [p._replace(dictionary="A") for p in zstd_primers()]


@functools.lru_cache(maxsize=None)
def dict_plans():
    """-> [(name, chunk)]: the planned frames of tests/zstd_dictgen.py and the state-sensitive plain plans"""
    plain = {v.name: v for v in zstd_victims()[0]}
    return [(n, c) for n, c, _, _ in D.planned_frames()] + [(n, plain[n].chunk) for n in ZSTD_STATE_SENSITIVE]


# Chunks that libzstd 1.4.8 accepts with that dictionary and this decoder refuses, under documented difference 1 of
# include/hipcomp/zstd.h.  The plan names one sequence in Repeat_Mode over a bitstream written for two sequences and the
# predefined tables: with A's tables the one sequence does not end the bitstream exactly (tests/test_decoder_state_cpu.py
# counts the bits), libzstd goes on with what its register holds.
DICT_DOCUMENTED_DIFFERENCES = {"repeat_mode_without_tables_with_A"}


@functools.lru_cache(maxsize=None)
def dict_victims():
    """-> [Stream]: every plan of dict_plans() with A, with B and with no dictionary in turn.  What is expected is the
    arbiter's verdict and bytes with that dictionary (without one, libzstd's plain verdict): libzstd is needed.  Then
    the chunks of zstd_leak_plans() without a dictionary."""
    ds = dictionaries()
    out = []
    for name, chunk in dict_plans():
        assert len(chunk) <= VICTIM_MAX
        for key in ("A", "B", None):
            content = D.arbiter(chunk, VICTIM_MAX, ds[key].bytes if key else None)
            if f"{name}_with_{key}" in DICT_DOCUMENTED_DIFFERENCES:
                assert content is not None
                content = None
            out.append(stream(f"{name}_with_{key or 'no_dictionary'}", chunk, content, room=None if content is not None else 512, dictionary=key))
    return out + [v._replace(name=v.name + "_with_no_dictionary") for v, _, _ in zstd_leak_plans()]


@functools.lru_cache(maxsize=None)
def dict_within_chunk():
    """-> [Stream], all legal, all with dictionary A: frame 1 describes its own tree and tables, frame 2 repeats the
    dictionary's; frame 1 moves A's repeat offsets, frame 2 begins with each repeat code."""
    a = dictionary_a()
    lits = D.TEXT[700:900]
    own = bytes(range(32, 127)) * 3 + lits           # another tree than the dictionary's
    fse = dict(modes=(G.FSE, G.FSE, G.FSE), logs=(6, 6, 7))
    one = D.frame(a, [("seq", _huffman_section(own, 4, "direct"), own, MANY, fse)])
    two = D.frame(a, [("seq", "treeless", lits, DICT_SEQ * 3, REPEAT_ALL)], dict_id=a.dict_id)
    out = [stream("own_tables_then_the_dictionarys", one[0] + two[0], one[1] + two[1], dictionary="A"),
           stream("own_tables_then_the_dictionarys_skippable_between", one[0] + G.skippable(b"x" * 9) + two[0], one[1] + two[1], dictionary="A")]
    moved = D.frame(a, [("seq", G.literals_raw(lits), lits, MOVE_OFFSETS + [(2, 5, 1)], {})])
    for ov in (1, 2, 3):
        for ll in (0, 5):
            rep = D.frame(a, [("seq", G.literals_raw(lits), lits, [(ll, 8, ov), (2, 5, 1)], {})])
            out.append(stream(f"moved_offsets_then_repeat_code_{ov}_ll_{ll}", moved[0] + rep[0], moved[1] + rep[1], dictionary="A"))
    return out


def zstd_size_query_model(s: Stream, given_dict_id=None):
    """What include/hipcomp/zstd.h and zstd_dict.h promise of the size query.  Where every frame declares its size: the sum of
    the declared sizes, or 0 where a frame or block header is refused or the chunk ends early; nothing is decoded.
    Otherwise the decoded size, 0 for a refused chunk.  given_dict_id: None for the plain decoder (a Dictionary_ID other
    than 0 is refused), else the ID of the chunk's dictionary (0: none, or raw content)."""
    c, at, total = s.chunk, 0, 0
    while at < len(c):
        n = len(c) - at
        if n < 5:
            return 0
        magic = int.from_bytes(c[at:at + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if n < 8 or 8 + int.from_bytes(c[at + 4:at + 8], "little") > n:
                return 0
            at += 8 + int.from_bytes(c[at + 4:at + 8], "little")
            continue
        fhd = c[at + 4]
        if magic != G.MAGIC or fhd & 8:
            return 0
        single, did_bytes = fhd >> 5 & 1, (0, 1, 2, 4)[fhd & 3]
        fcs_bytes = single if fhd >> 6 == 0 else 1 << (fhd >> 6)
        hb = 5 + (0 if single else 1) + did_bytes + fcs_bytes
        if n < hb or (not single and 10 + (c[at + 5] >> 3) > 31):
            return 0
        did = int.from_bytes(c[at + hb - fcs_bytes - did_bytes:at + hb - fcs_bytes], "little")
        if did != 0 and did != given_dict_id:
            return 0
        if not fcs_bytes:
            return len(s.content) if is_legal(s) else 0
        total += int.from_bytes(c[at + hb - fcs_bytes:at + hb], "little") + (256 if fcs_bytes == 2 else 0)
        at += hb
        while True:
            if len(c) - at < 3:
                return 0
            h = int.from_bytes(c[at:at + 3], "little")
            kind, follows = h >> 1 & 3, 1 if h >> 1 & 3 == 1 else h >> 3
            if kind == 3 or follows > len(c) - at - 3:
                return 0
            at += 3 + follows
            if h & 1:
                break
        if fhd & 4:
            if len(c) - at < 4:
                return 0
            at += 4
    return total


# ------------------------------------------------------------------------------------------------------ Deflate
DEFLATE_REQUIRED = ("unused_pattern_of_single_litlen_code", "unused_pattern_of_single_distance_code", "fixed_litlen_symbol_286",
                    "fixed_litlen_symbol_287", "fixed_distance_symbol_30", "fixed_distance_symbol_31", "repeat_16_first", "litlen_incomplete",
                    "dist_incomplete_two_codes", "match_without_distance_code")
ZSTD_REQUIRED = ZSTD_STATE_SENSITIVE


@functools.lru_cache(maxsize=None)
def _full_dynamic_tokens():
    """tokens for the largest alphabets: every literal, every length symbol, and every distance symbol that 16 KiB of
    content can reach (symbols 28 and 29 begin at distances 16 385 and 24 577: the table holds their codes, no
    match of a primer can use them)"""
    toks = list(range(256)) * 49
    toks += [("m", DG.LENGTH_BASE[i], 1 + i, 257 + i) for i in range(29)]
    toks += [("m", 3, DG.DIST_BASE[s]) for s in range(28)]
    return toks


def full_dynamic_block(w, final):
    """all 286 literal/length and all 30 distance lengths, codes of 15 bits in both"""
    DG.dynamic_block(w, _full_dynamic_tokens(), final, DG.max_alphabet_litlen(), DG.max_alphabet_dist())
    return DG.expand(_full_dynamic_tokens())


@functools.lru_cache(maxsize=None)
def deflate_primers():
    """-> [Stream]"""
    out = []

    def add(name, w, content):
        assert len(content) <= PRIMER_CONTENT_MAX, (name, len(content))
        out.append(stream(name, w.done(), content))
    w = DG.BitWriter()
    add("dynamic_286_and_30_symbols_15_bits", w, full_dynamic_block(w, True))
    text = DG._text(3000, 41)
    toks = list(text[:1500]) + [("m", 258, 700), ("m", 3, 1)] + list(text[1500:])
    w = DG.BitWriter()
    DG.fixed_block(w, toks, True)
    add("fixed_block", w, DG.expand(toks))
    w = DG.BitWriter()
    DG.dynamic_block(w, list(text[:900]), True, None, [0])       # HLIT = 257, HDIST = 1: no length and no distance code
    add("dynamic_hlit_257_hdist_1", w, text[:900])
    # the last block ends with 1, 37 and 63 literals behind its last match: they lie in the 64-byte literal queue
    for left, blk in ((1, DG.fixed_block), (37, DG.dynamic_block), (63, DG.fixed_block)):
        toks = list(text[:200]) + [("m", 40, 100)] + list(text[200:200 + 128 + left])
        w = DG.BitWriter()
        blk(w, toks, True)
        add(f"{left}_bytes_left_in_the_literal_queue", w, DG.expand(toks))
    # a stored block behind the full tables, then a fixed block: all three kinds in one stream
    w = DG.BitWriter()
    a = full_dynamic_block(w, False)
    DG.stored_block(w, text[:333], False)
    tail = [("m", 100, 5000), 33, ("m", 7, 1)]
    DG.fixed_block(w, tail, True)
    add("dynamic_stored_fixed", w, a + text[:333] + DG.expand(tail, a + text[:333]))
    # fails late: the full dynamic block, then a dynamic block cut 12 bytes in, inside its header
    w = DG.BitWriter()
    a = full_dynamic_block(w, False)
    whole_bytes = len(w.out)
    DG.dynamic_block(w, list(text[:400]), True)
    out.append(stream("fails_in_the_second_block", w.done()[:whole_bytes + 12], None, room=len(a) + 400))
    return out


TRUNCATED_WHOLE = 60 + 40 + 11 + 50 + 100      # what the stream that illegal_plans() truncates decodes to when whole


@functools.lru_cache(maxsize=None)
def deflate_victims():
    """-> ([Stream], names left out)"""
    out, left_out = [], []
    for name, s, content in DG.legal_plans():
        if len(s) <= VICTIM_MAX and len(content) <= VICTIM_MAX:
            out.append(stream(name, s, content))
        else:
            left_out.append(name)
    for name, s in DG.illegal_plans():
        if len(s) <= VICTIM_MAX:
            out.append(stream(name, s, None, room=TRUNCATED_WHOLE if name.startswith("truncated_at_") else None))
        else:
            left_out.append(name)
    return out, left_out


@functools.lru_cache(maxsize=None)
def deflate_within_stream():
    """-> [Stream]: one stream of primer block(s) and a victim block behind them"""
    out = []
    text = DG._text(600, 43)

    def behind_full(name, victim, content_of=None):
        """victim(w) writes the final block; content_of(history) -> what it adds, None: the stream is refused"""
        w = DG.BitWriter()
        a = full_dynamic_block(w, False)
        victim(w)
        out.append(stream(name, w.done(), None if content_of is None else a + content_of(a), room=None if content_of else len(a) + REFUSED_ROOM))

    def one_litlen_code_unused_pattern(w):
        DG.dynamic_header(w, True, 257, 1, DG._cl_symbols([0] * 256 + [1] + [0], True))
        w.bits(1, 1)    # the code of 256 is 0; 1 is nobody's
        w.bits(0, 16)
    behind_full("full_dynamic_then_unused_pattern_of_single_litlen_code", one_litlen_code_unused_pattern)
    lit = DG.flat_lengths({97, 256, 257}, 258)
    codes = DG.canonical_codes(lit)

    def one_distance_code(pattern, dist_length):
        def victim(w):
            DG.dynamic_header(w, True, 258, 1, DG._cl_symbols(lit + [dist_length], True))
            w.code(*codes[97])
            w.code(*codes[257])
            w.bits(*pattern)
            w.code(*codes[256])
        return victim
    behind_full("full_dynamic_then_unused_pattern_of_single_distance_code", one_distance_code((1, 1), 1))
    behind_full("full_dynamic_then_match_without_distance_code", one_distance_code((0, 5), 0))
    behind_full("full_dynamic_then_single_distance_code", one_distance_code((0, 1), 1), lambda h: b"a" * 4)
    behind_full("full_dynamic_then_only_end_of_block_code", lambda w: DG.dynamic_block(w, [], True, [0] * 256 + [1], [0]), lambda h: b"")
    for s in (286, 287):
        behind_full(f"full_dynamic_then_fixed_litlen_symbol_{s}", lambda w, s=s: DG.fixed_block(w, [65, ("l", s), 66], True))
    for s in (30, 31):
        behind_full(f"full_dynamic_then_fixed_distance_symbol_{s}", lambda w, s=s: DG.fixed_block(w, list(b"abcdefgh") + [("d", s, 0), 66], True))

    def repeat_16_first(w):
        cl = DG.flat_lengths({16, 17, 18, 0, 1, 8}, 19)
        DG.dynamic_header(w, True, 257, 2, [(16, 0)] + [(8, 0)] * 254 + [(0, 0)] * 2, cl)
        w.bits(0, 24)
    behind_full("full_dynamic_then_repeat_16_first", repeat_16_first)
    inc = DG.flat_lengths(set(range(64, 91)) | {256}, 257)
    inc[64] = 0
    behind_full("full_dynamic_then_litlen_incomplete", lambda w: (DG.dynamic_block(w, [66], True, inc, [1, 1], lenient=True), w.bits(0, 16)))
    ok = DG.flat_lengths(set(range(64, 91)) | {256}, 257)
    behind_full("full_dynamic_then_dist_incomplete_two_codes", lambda w: (DG.dynamic_block(w, [65], True, ok, [2, 2], lenient=True), w.bits(0, 16)))
    # legal: dynamic, fixed, dynamic, fixed; a stored block between two fixed blocks
    w, expect = DG.BitWriter(), bytearray()
    for k, blk in enumerate((DG.dynamic_block, DG.fixed_block, DG.dynamic_block, DG.fixed_block)):
        toks = list(text[100 * k:100 * k + 90]) + ([("m", 30 + k, 50 * k)] if k else []) + [k]
        blk(w, toks, k == 3)
        expect += DG.expand(toks, bytes(expect))
    out.append(stream("dynamic_fixed_dynamic_fixed", w.done(), expect))
    w = DG.BitWriter()
    DG.fixed_block(w, list(text[:70]), False)
    DG.stored_block(w, text[70:170], False)
    toks = [("m", 50, 170), 9, ("m", 258, 1)]
    DG.fixed_block(w, toks, True)
    out.append(stream("fixed_stored_fixed", w.done(), text[:170] + DG.expand(toks, text[:170])))
    return out


# --------------------------------------------------------------------------------------------------------- gzip
def _wrong(member: bytes, wrapper: int, which: int) -> bytes:
    """one bit of the CRC-32 / Adler-32 (which 0) or of ISIZE (which 1; zlib has none: its Adler-32) flipped"""
    at = len(member) - (4 if wrapper == M.ZLIB or which else 8)
    b = bytearray(member)
    b[at + 1] ^= 0x10
    return bytes(b)


@functools.lru_cache(maxsize=None)
def gzip_streams(wrapper: int):
    """-> (primers, victims): the Deflate primers and victims as members of `wrapper`.  Primers and the last victims
    carry the right trailer; the first victims are the same members with a wrong checksum or a wrong ISIZE in turn,
    then come the refused streams.  content: None for every member that is not decoded; what status it gets is
    gzip_membergen.status_model's to say."""
    primers = [stream(p.name, M.wrap(wrapper, p.content or b"", p.chunk), p.content, room=p.room) for p in deflate_primers()]
    victims, _ = deflate_victims()
    wrong, right = [], []
    for k, v in enumerate(x for x in victims if is_legal(x)):
        m = M.wrap(wrapper, v.content, v.chunk)
        right.append(stream(v.name, m, v.content))
        wrong.append(stream(v.name + ("_wrong_checksum", "_wrong_isize")[k % 2], _wrong(m, wrapper, k % 2), None, room=len(v.content)))
    refused = [stream(v.name, M.wrap(wrapper, b"", v.chunk), None, room=v.room) for v in victims if not is_legal(v)]
    return primers, wrong + refused + right


# ------------------------------------------------------------------------------------------------------- layout
def layout(waves, primers, victims):
    """The batch of 3 * waves chunks as indices into primers + victims.  Wave w decodes chunk w, chunk waves + w and
    chunk 2 * waves + w: primer w % P, victim (w // P) % V, and the legal victim (w // P + 1) % V_legal.  Every
    victim follows every primer on some wave, and every wave decodes a legal stream right behind its victim."""
    p, v = len(primers), len(victims)
    legal = [p + i for i, s in enumerate(victims) if is_legal(s)]
    assert p * v <= waves, (p, v, waves)
    return ([w % p for w in range(waves)] + [p + (w // p) % v for w in range(waves)]
            + [legal[(w // p + 1) % len(legal)] for w in range(waves)])


def describe(waves, primers, victims, chunk_index):
    """names a chunk of layout() for a failure message: its wave, the wave's primer and victim, and which of the three"""
    w = chunk_index % waves
    both = list(primers) + list(victims)
    index = layout(waves, primers, victims)
    return (f"wave {w}: primer {both[index[w]].name}, victim {both[index[waves + w]].name}, then {both[index[2 * waves + w]].name}; "
            f"chunk {chunk_index} is the {('primer', 'victim', 'legal stream behind it')[chunk_index // waves]}")
