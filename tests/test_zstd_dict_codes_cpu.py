"""csrc/zstd_dict_compress/zstd_dict_codes.hpp on the CPU: the scalar prepare and the scalar encoder against a blob,
through tests/zstd_dict_codes_driver.cpp (a stand-alone program built with AddressSanitizer and UBSan).  The arbiter of
every frame is ZSTD_decompress_usingDict of libzstd against the original dictionary bytes."""
import random
import struct

import pytest

import zstd_dict_codes_fixtures as X
import zstd_dict_fixtures as F
import zstd_dictgen as D
import zstd_framegen as G


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("zstd_dict_codes")
    return X.build_driver(str(d)), str(d)


@pytest.fixture(scope="module")
def dictionaries():
    trained, _, _ = F.load()
    out = dict(X.planned_dictionaries())
    out.update({"a": trained["a"], "b": trained["b"], "raw": trained["raw"]})
    return out


def compose(content: bytes, parts):
    """parts: bytes (literals) or (ml, offset) (a match of the history content ++ chunk) -> (chunk, tokens)"""
    hist, start, tokens, ll = bytearray(content), len(content), [], 0
    for p in parts:
        if isinstance(p, bytes):
            hist += p
            ll += len(p)
        else:
            ml, off = p
            assert 0 < off <= len(hist)
            for _ in range(ml):
                hist.append(hist[-off])
            tokens.append((ll, ml, off))
            ll = 0
    return bytes(hist[start:]), tokens


def planned_cases(dicts):
    """-> [(name, dictionary name or None, chunk, tokens, checksum)]"""
    rnd = random.Random(7)
    rb = lambda n: bytes(rnd.randrange(256) for _ in range(n))
    model = {k: X.dict_model(v) for k, v in dicts.items()}
    out = []

    def add(name, dname, parts, checksum=False):
        chunk, tokens = compose(model[dname]["content"] if dname else b"", parts)
        assert len(chunk) <= X.MAX_CHUNK
        out.append((name, dname, chunk, tokens, checksum))
    text = lambda n, seed: X.skewed_text(n, seed)
    seq = [text(5, 1), (10, 45), text(3, 2), (6, 12)]
    add("treeless_1_stream", "formatted", [text(300, 3)] + seq)
    add("treeless_4_streams", "formatted", [text(3000, 4)] + seq, checksum=True)
    # one table in Repeat_Mode: the two others hold one code each (RLE)
    ll_mix = [b"", b"", b"", b"", b"", b"", b"", b"", b"", b"", rb(3), rb(9), rb(17), rb(40)]
    add("repeat_ll", "formatted", [rb(64)] + [x for lit in ll_mix for x in (lit, (5, 33))])
    of_mix = [(1 << c) + k - 3 for c in range(2, 16) for k in (0, 1)]
    add("repeat_of", "content_32768", [rb(64)] + [x for off in of_mix for x in (rb(2), (5, off))])
    ml_mix = [3] * 10 + [8, 13, 23, 33]
    add("repeat_ml", "formatted", [rb(64)] + [x for ml in ml_mix for x in (rb(2), (ml, 33))])
    add("repeat_all", "content_32768", [rb(64)] + [x for k, off in enumerate(of_mix)
                                                  for x in (ll_mix[k % len(ll_mix)], (ml_mix[k % len(ml_mix)], off))])
    add("repeat_illegal_of", "few_offset_codes", [rb(64)] + [x for off in of_mix[:16] for x in (rb(2), (5, off))])
    add("repeat_loses_ll", "formatted", [rb(64)] + [x for k in range(30) for x in (rb(1 + k % 15), (5, 33))])
    add("minus_one_codes", "minus_one", [rb(64)] + [x for k in range(40) for x in (rb(k % 36), (4 + k % 3, 33 + k))])
    add("limits", "limits", [text(200, 5)] + [x for k in range(40) for x in (text(k % 20, k), (3 + k, 20 + 3 * k))])
    for dname in ("id_1_byte", "id_2_bytes", "formatted", "id_zero", "raw_text"):
        add(f"dictionary_id_{dname}", dname, [text(100, 6)] + seq)
    add("first_sequence_repeats_the_dictionarys_offset", "formatted", [text(5, 7), (10, 5), text(4, 8), (6, 5)])
    add("first_sequence_without_literals", "formatted", [(10, 5), text(4, 8), (6, 5)])
    add("first_sequence_raw_dictionary_offset_1", "raw_text", [b"q", (10, 1), text(30, 9)])
    add("match_wholly_in_the_tail", "raw_text", [rb(5), (10, 5 + 100), rb(20)])
    add("match_ends_at_the_tails_last_byte", "raw_text", [rb(5), (10, 5 + 10), rb(20)])
    add("match_crosses_into_the_chunk", "raw_text", [rb(20), (10, 20 + 4), rb(20)])
    add("offset_65535", "content_40000", [text(25600, 13), (9, 65535), text(7, 14)])
    add("farthest_tail_byte", "content_32768", [rb(9), (12, 9 + 32768), rb(5)])
    for dname in ("content_7", "content_8", "raw_7", "content_32768", "content_40000", "raw_big", "raw_empty", "a", "b", "raw"):
        add(f"plain_{dname}", dname, [text(60, 10), (8, 20), text(9, 11), (5, 20)], checksum=dname in ("a", "raw_big"))
    add("reaches_content_of_7_bytes", "content_7", [rb(2), (4, 2 + 5), rb(30)])
    for dname in ("formatted", "raw_text"):
        add(f"rle_chunk_{dname}", dname, [b"z" * 500])
        add(f"raw_chunk_{dname}", dname, [rb(300)])
        add(f"empty_chunk_{dname}", dname, [])
        add(f"three_bytes_{dname}", dname, [b"abc"], checksum=True)
    add("no_dictionary", None, [text(300, 12), (10, 45), text(3, 2), (6, 12)])
    # records against the trained dictionaries: matches into "a" / "b" found by a simple search
    for dname, vocab, seed in (("a", F.VOCAB_A, 41), ("b", F.VOCAB_B, 42), ("raw", F.VOCAB_A, 43)):
        content = model[dname]["content"]
        for k, rec in enumerate(F.records(seed, vocab, 6)):
            parts, at = [], 0
            while at < len(rec):
                hit = content.rfind(rec[at:at + 6]) if at + 6 <= len(rec) else -1
                if hit < 0 or len(content) - hit + at > 65535:
                    parts.append(rec[at:at + 1])
                    at += 1
                    continue
                ml = 6
                while at + ml < len(rec) and hit + ml < len(content) and content[hit + ml] == rec[at + ml]:
                    ml += 1
                parts.append((ml, len(content) - hit + at))
                at += ml
            merged = []
            for p in parts:
                if isinstance(p, bytes) and merged and isinstance(merged[-1], bytes):
                    merged[-1] += p
                else:
                    merged.append(p)
            add(f"record_{dname}_{k}", dname, merged, checksum=k % 2 == 1)
    return out


def tags_of(name, info, model, tokens):
    """what a frame reached, for the census"""
    tags = {f"dictionary_id_{info['id_bytes']}_bytes", ("raw_block", "rle_block", "compressed_block")[info["block"]]}
    if info["block"] != 2:
        return tags
    if info["lit_type"] == X.TREELESS:
        tags.add(f"treeless_{info['lit_streams']}_streams")
    rep = tuple(m == X.REPEAT for m in info["modes"])
    if any(rep):
        tags.add("repeat_" + ("all" if all(rep) else "+".join(k for k, r in zip(("ll", "of", "ml"), rep) if r)))
    if model["norms"] and info["seqs"]:
        for k, (key, code_of) in enumerate((("ll", G.ll_code), ("of", lambda v: v.bit_length() - 1), ("ml", G.ml_code))):
            norm = model["norms"][key][0]
            codes = {code_of(s[(0, 2, 1)[k]]) for s in info["seqs"]}
            legal = all(c < len(norm) and norm[c] != 0 for c in codes)
            if len(codes) > 1 and not legal:
                assert info["modes"][k] != X.REPEAT, name
                tags.add("repeat_illegal")
            if len(codes) > 1 and legal and info["modes"][k] != X.REPEAT:
                tags.add("repeat_loses")
    if info["seqs"]:
        ll, ml, ov = info["seqs"][0]
        if ov == 1:
            tags.add("first_sequence_offset_value_1")
        elif ll == 0 and tokens[0][2] == model["rep"][0]:
            tags.add("first_sequence_no_literals_not_repeat")
    return tags


def test_every_frame_comes_back_from_libzstd_and_the_census(driver, dictionaries):
    exe, tmp = driver
    z = D.libzstd()
    assert z is not None, "libzstd.so.1 is the arbiter of this test"
    cases = planned_cases(dictionaries)
    frames = X.encode(exe, tmp, [(chunk, tokens, dictionaries[d] if d else None, cs) for _, d, chunk, tokens, cs in cases])
    census = set()
    for (name, dname, chunk, tokens, cs), frame in zip(cases, frames):
        assert frame is not None, name
        assert len(frame) <= len(chunk) + 18, name
        d = dictionaries[dname] if dname else None
        assert D.arbiter(frame, len(chunk), d) == chunk, name
        assert D.arbiter(frame, len(chunk) + 64, d) == chunk, name
        model = X.dict_model(d or b"")
        info = X.frame_info(frame, model)
        assert info["dict_id"] == model["id"] and info["checksum"] == cs, name
        assert info["id_bytes"] == (0 if model["id"] == 0 else 1 if model["id"] < 256 else 2 if model["id"] < 65536 else 4), name
        if info["block"] == 2:
            assert X.tokens_of(info, model["rep"][0] if d is not None else 0) == tokens, name
        tags = tags_of(name, info, model, tokens)
        print(name, len(chunk), len(frame), sorted(tags))
        census |= tags
        # where a match lies, by the plan
        pos = 0
        for ll, ml, off in tokens if info["block"] == 2 else ():
            pos += ll
            if off > pos:
                census.add("match_wholly_in_tail" if off - pos > ml else "match_ends_at_tail_end" if off - pos == ml else "match_crosses_into_chunk")
            if off == 65535:
                census.add("offset_65535")
            pos += ml
    assert census == {
        "treeless_1_streams", "treeless_4_streams", "repeat_ll", "repeat_of", "repeat_ml", "repeat_all", "repeat_illegal", "repeat_loses",
        "dictionary_id_0_bytes", "dictionary_id_1_bytes", "dictionary_id_2_bytes", "dictionary_id_4_bytes",
        "first_sequence_offset_value_1", "first_sequence_no_literals_not_repeat",
        "match_wholly_in_tail", "match_ends_at_tail_end", "match_crosses_into_chunk", "offset_65535",
        "raw_block", "rle_block", "compressed_block"} | {t for t in census if t.startswith("repeat_") and "+" in t}, sorted(census)
    # with no dictionary the frame is the plain scalar encoder's: no ID field, the first sequence has no offset before it
    plain = [f for (name, *_), f in zip(cases, frames) if name == "no_dictionary"][0]
    assert plain[4] & 3 == 0


def test_prepare_scalar_blobs(driver, dictionaries):
    """the blob's size against the restated formula, its header, the primed table against its restated definition, the
    tail; content of 7 and 8 bytes (T = 0 and 8), of 32768 and 40000 bytes (only the tail)"""
    exe, tmp = driver
    names = sorted(dictionaries)
    got = X.prepare(exe, tmp, [dictionaries[n] for n in names])
    tails = {}
    for name, (status, blob) in zip(names, got):
        d = dictionaries[name]
        model = X.dict_model(d)
        assert status == 0 and len(blob) == X.prepared_size(len(d)), name
        words = struct.unpack_from("<16I", blob)
        t = X.tail_len(len(model["content"]))
        tails[name] = t
        assert words[:5] == (0x45435A48, 1, 1, model["id"], 1 if model["norms"] else 0), name
        assert words[5:8] == tuple(model["rep"]) and words[8] == len(model["content"]) and words[9] == t, name
        if model["norms"]:
            assert words[10:13] == (model["norms"]["ll"][1], model["norms"]["of"][1], model["norms"]["ml"][1]), name
        else:
            assert blob[X.TABLES_AT:X.BASE] == bytes(X.BASE - X.TABLES_AT), name
        assert words[13:] == (0, 0, 0)
        tail = model["content"][len(model["content"]) - t:]
        assert blob[X.BASE:X.BASE + t] == tail and not any(blob[X.BASE + t:]), name
        assert list(struct.unpack_from("<4096H", blob, X.TABLE_AT)) == X.prime_table(tail), name
    assert tails["content_7"] == 0 and tails["raw_7"] == 0 and tails["content_8"] == 8 and tails["raw_empty"] == 0
    assert tails["content_32768"] == tails["content_40000"] == tails["raw_big"] == 32768
    # a probability of -1 round-trips: the blob's norm is the dictionary's
    blob = got[names.index("minus_one")][1]
    norms = struct.unpack_from("<192h", blob, X.BASE - 384)
    assert list(norms[:36]) == X.dict_model(dictionaries["minus_one"])["norms"]["ll"][0] and -1 in norms[:36]


def test_prepare_scalar_refuses_what_the_decoder_refuses(driver):
    exe, tmp = driver
    planned = D.planned_dictionaries()
    got = X.prepare(exe, tmp, [d for _, d, _ in planned])
    for (name, d, legal), (status, blob) in zip(planned, got):
        assert (status == 0) == legal, name
        if not legal:
            assert blob == struct.pack("<16I", 0x45435A48, 1, *([0] * 14)), name


def test_blob_size_query(hc, driver):
    import ctypes
    import subprocess
    exe, _ = driver
    lib = hc.api.zstd_dict_compress_library()
    for n in (0, 1, 7, 8, 15, 16, 17, 2000, 32767, 32768, 32769, 40000, 1 << 20, 1 << 30):
        assert lib.prepared_size(n) == X.prepared_size(n) == hc.batch.ZstdDictEncoder().prepared_size(n), n
        assert int(subprocess.run([exe, "size", str(n)], capture_output=True, text=True, check=True).stdout) == X.prepared_size(n)
        assert lib.prepared_size(n) % 16 == 0
    assert lib.prepared_size(0) == 14080
    t = ctypes.c_size_t(7)
    assert lib.hipcompBatchedZstdDictCompressGetPreparedSize((1 << 30) + 1, ctypes.byref(t)) == 10 and t.value == 7
    assert lib.hipcompBatchedZstdDictCompressGetPreparedSize(100, None) == 10
