"""The batched Zstandard encoder with dictionaries (include/hipcomp/zstd_dict_compress.h,
lib/libhipcomp_zstd_dict_compress.so) on the GPU.  Every buffer of the byte-level tests lies in
decode_guard.GuardedSlots.  The judges of a frame are this library's decoder with dictionaries on the device
(ZstdDictDecoder: status 0, the exact size, the bytes) and libzstd (ZSTD_decompress_usingDict) where it loads; the
scalar encoder of csrc/zstd_dict_compress/zstd_dict_codes.hpp (tests/zstd_dict_codes_driver.cpp) is held to write, from
a kernel frame's tokens, that very frame, and the scalar prepare that very blob."""
import random
import struct

import numpy as np
import pytest

import test_zstd_dict_codes_cpu as C
import zstd_dict_codes_fixtures as X
import zstd_dict_fixtures as F
import zstd_dictgen as D
from decode_guard import GuardedSlots

pytestmark = pytest.mark.gpu
OK, CANNOT, INVALID = 0, 12, 10
MAX = X.MAX_CHUNK
HEADER = 64


def bound(n: int) -> int:
    return n + 18


class Env:
    """every dictionary of the tests, digested by ONE prepare launch of the encoder (blobs in guarded slots) and one of
    the decoder (the judge's blobs)"""

    def __init__(self, hc, torch, dev, tmp):
        self.hc, self.torch, self.dev = hc, torch, dev
        self.exe, self.tmp = X.build_driver(tmp), tmp
        trained, _, _ = F.load()
        named = [(n, d, True) for n, d in X.planned_dictionaries().items()] + [(n, trained[n], True) for n in ("a", "b", "raw")]
        named += [(n, d, ok) for n, d, ok in D.planned_dictionaries()]
        self.names = [n for n, _, _ in named]
        self.dicts = [d for _, d, _ in named]
        self.legal = [ok for _, _, ok in named]
        self.by_name = {}
        for i, n in enumerate(self.names):
            self.by_name.setdefault(n, i)
        self.enc = hc.batch.ZstdDictEncoder()
        self.sizes = [self.enc.prepared_size(len(d)) for d in self.dicts]
        self.src = GuardedSlots(torch, [len(d) for d in self.dicts], dev, offsets=(1, 3, 5, 7, 9, 11, 13, 15), seed=31, chunks=self.dicts)
        self.blobs = GuardedSlots(torch, self.sizes, dev, seed=32, region=[s if ok else HEADER for s, ok in zip(self.sizes, self.legal)])
        self.statuses_t = torch.full((len(self.dicts),), -1, dtype=torch.int32, device=dev)
        st = self.enc.lib.hipcompBatchedZstdDictCompressPrepareAsync(
            self.src.ptrs.data_ptr(), self.src.sizes.data_ptr(), len(self.dicts), self.blobs.ptrs.data_ptr(), self.blobs.caps_t.data_ptr(),
            self.statuses_t.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
        assert st == OK
        torch.cuda.synchronize()
        self.after = self.blobs.after()
        self.statuses = self.statuses_t.cpu().tolist()
        self.ptrs = self.blobs.ptrs.cpu().tolist()
        self.dec_blobs, dec_statuses = hc.batch.ZstdDictDecoder().prepare(self.dicts, dev)
        torch.cuda.synchronize()
        self.dec_statuses = dec_statuses.cpu().tolist()
        self.dec_ptrs = self.dec_blobs.ptrs.cpu().tolist()
        self.models = {}

    def ptr(self, name):
        return 0 if name is None else self.ptrs[self.by_name[name]]

    def dec_ptr(self, name):
        return 0 if name is None else self.dec_ptrs[self.by_name[name]]

    def bytes_of(self, name):
        return None if name is None else self.dicts[self.by_name[name]]

    def model(self, name):
        if name not in self.models:
            self.models[name] = X.dict_model(self.bytes_of(name) or b"")
        return self.models[name]

    def blob(self, i, n):
        at = int(self.blobs.at[i])
        return self.after[at:at + n].tobytes()


@pytest.fixture(scope="module")
def env(hc, cuda, tmp_path_factory):
    import torch
    return Env(hc, torch, cuda, str(tmp_path_factory.mktemp("zstd_dict_compress_gpu")))


def compress_guarded(env, chunks, names, max_chunk=MAX, offsets=(0,), turn=0, checksum=False, untouched=()):
    """-> (frames, sizes): chunk i compressed against the blob of dictionary names[i] (None: a null entry) inside guarded
    slots; containment is asserted here.  untouched: chunks of which not a byte may be written (size 0)"""
    hc, torch, dev = env.hc, env.torch, env.dev
    n = len(chunks)
    cap = bound(max_chunk)
    src = GuardedSlots(torch, [len(c) for c in chunks], dev, offsets=offsets, turn=turn, seed=21, chunks=chunks)
    dst = GuardedSlots(torch, [cap] * n, dev, offsets=offsets, turn=turn + 3, seed=22, region=[0 if i in untouched else cap for i in range(n)])
    enc = hc.batch.ZstdDictEncoder(checksum=checksum)
    tbytes = max(enc.compress_temp_size(n, max_chunk), 8)
    temp = GuardedSlots(torch, [tbytes], dev, seed=23)
    prepared = torch.tensor([env.ptr(nm) for nm in names], dtype=torch.int64, device=dev)
    sizes_t = torch.full((n,), -1, dtype=torch.int64, device=dev)
    st = enc.lib.hipcompBatchedZstdDictCompressAsync(
        src.ptrs.data_ptr(), src.sizes.data_ptr(), max_chunk, n, int(temp.ptrs[0].item()), tbytes, dst.ptrs.data_ptr(),
        sizes_t.data_ptr(), prepared.data_ptr(), enc.opts, int(torch.cuda.current_stream().cuda_stream))
    assert st == OK
    torch.cuda.synchronize()
    assert src.unchanged() is None, src.unchanged()                      # the input is only read
    assert temp.first_guard_change() is None, "temp space: " + str(temp.first_guard_change())
    got = dst.after()
    assert dst.first_guard_change(got) is None, dst.first_guard_change(got)   # nothing at or beyond out_i + bound
    assert env.blobs.first_guard_change() is None and (env.blobs.after() == env.after).all()   # the blobs are only read
    sizes = sizes_t.cpu().tolist()
    for i, (c, s) in enumerate(zip(chunks, sizes)):
        assert (s == 0) if i in untouched else (0 < s <= bound(len(c))), (i, len(c), s)
    return [dst.slot_bytes(got, i, sizes[i]) for i in range(n)], sizes


def judge(env, chunks, names, frames, expect_ok=True):
    """ZstdDictDecoder on the device with the decoder's blobs: status 0, the exact size, the bytes; libzstd where it loads"""
    hc, torch, dev = env.hc, env.torch, env.dev
    cap = max([len(c) for c in chunks] + [1])
    comp = hc.batch.from_host_chunks(frames, dev)
    prepared = torch.tensor([env.dec_ptr(nm) for nm in names], dtype=torch.int64, device=dev)
    dec, actual, statuses = hc.batch.ZstdDictDecoder().decompress(comp, cap, prepared)
    torch.cuda.synchronize()
    st, sz, got = statuses.cpu().tolist(), actual.cpu().tolist(), dec.to_host_chunks()
    if not expect_ok:
        return st, sz, got
    for i, (c, nm) in enumerate(zip(chunks, names)):
        assert st[i] == OK and sz[i] == len(c) and got[i] == c, (i, nm, st[i], sz[i], len(c))
    if D.libzstd() is not None:
        for i, (c, nm, f) in enumerate(zip(chunks, names, frames)):
            assert D.arbiter(f, len(c), env.bytes_of(nm)) == c, (i, nm)


def held_to_the_scalar_encoder(env, chunks, names, frames, checksum):
    """the frame's tokens, given to encode_frame_dict, give the frame; -> the tokens"""
    cases, all_tokens = [], []
    for c, nm, f in zip(chunks, names, frames):
        info = X.frame_info(f, env.model(nm))
        tokens = X.tokens_of(info, env.model(nm)["rep"][0] if nm is not None else 0) or []
        all_tokens.append(tokens if info["block"] == 2 else None)
        cases.append((c, tokens, env.bytes_of(nm), checksum))
    again = X.encode(env.exe, env.tmp, cases)
    for i, (f, g) in enumerate(zip(frames, again)):
        assert f == g, (i, names[i], len(chunks[i]), len(f), None if g is None else len(g))
    return all_tokens


# ---------------------------------------------------------------------------------------------------------- prepare
def test_prepare_is_the_scalar_prepare(env):
    """one launch for every dictionary; every blob byte for byte prepare_scalar's (the table is a definition), the statuses
    those of the decoder's prepare on the same list, nothing outside the blobs written, the dictionaries only read"""
    assert env.src.unchanged() is None, env.src.unchanged()
    assert env.blobs.first_guard_change(env.after) is None, env.blobs.first_guard_change(env.after)
    assert env.statuses == env.dec_statuses
    assert env.statuses == [OK if ok else CANNOT for ok in env.legal]
    want = X.prepare(env.exe, env.tmp, env.dicts)
    for i, (name, (status, blob)) in enumerate(zip(env.names, want)):
        assert (status == 0) == env.legal[i], name
        assert env.blob(i, len(blob)) == blob, name
    assert sum(env.legal) >= 30 and len(env.legal) - sum(env.legal) >= 10


def test_prepare_refuses_a_misaligned_blob_and_a_small_capacity(env):
    hc, torch, dev = env.hc, env.torch, env.dev
    d = env.bytes_of("formatted")
    need = env.enc.prepared_size(len(d))
    dicts = [d] * 4
    src = GuardedSlots(torch, [len(d)] * 4, dev, seed=41, chunks=dicts)
    # blob 0: fine; 1: capacity one short; 2: capacity 63 (not even the header fits); 3: misaligned by 8
    caps = [need, need - 1, 63, need]
    blobs = GuardedSlots(torch, [need + 16] * 4, dev, offsets=(0, 0, 0, 8), seed=42, region=[need, HEADER, 0, 0])
    caps_t = torch.tensor(caps, dtype=torch.int64, device=dev)
    statuses = torch.full((4,), -1, dtype=torch.int32, device=dev)
    st = env.enc.lib.hipcompBatchedZstdDictCompressPrepareAsync(
        src.ptrs.data_ptr(), src.sizes.data_ptr(), 4, blobs.ptrs.data_ptr(), caps_t.data_ptr(), statuses.data_ptr(),
        int(torch.cuda.current_stream().cuda_stream))
    assert st == OK
    torch.cuda.synchronize()
    got = blobs.after()
    assert blobs.first_guard_change(got) is None, blobs.first_guard_change(got)
    assert statuses.cpu().tolist() == [OK, INVALID, INVALID, INVALID]
    assert blobs.slot_bytes(got, 0, need) == env.blob(env.by_name["formatted"], need)
    assert blobs.slot_bytes(got, 1, HEADER) == struct.pack("<16I", 0x45435A48, 1, *([0] * 14))


# -------------------------------------------------------------------------------------------------------- round trip
def round_trip_cases(env):
    """[(name, chunk, dictionary name or None)]: every planned chunk of the CPU test with its dictionary, and the fixture
    records cut to the chunk limit against "a", "b", "raw" and none"""
    dicts = {n: env.bytes_of(n) for n in env.names if env.legal[env.by_name[n]]}
    out = [(name, chunk, dname) for name, dname, chunk, _, _ in C.planned_cases(dicts)]
    data = F.inputs({"a": dicts["a"]})
    for k, (name, content) in enumerate(sorted(data.items())):
        for dname in ("a", "b", "raw", None):
            out.append((f"{name}_{dname}", content[:MAX] if k % 2 else content[-MAX:], dname))
    return out


def test_round_trip_at_every_byte_offset_and_byte_for_byte(env):
    cases = round_trip_cases(env)
    assert len(cases) >= 100 and any(len(c) == MAX for _, c, _ in cases)
    chunks, names = [c for _, c, _ in cases], [d for _, _, d in cases]
    offsets = tuple(range(16))
    seen = set()
    for checksum in (False, True):
        for turn in (0, 5):
            frames, _ = compress_guarded(env, chunks, names, offsets=offsets, turn=turn, checksum=checksum)
            judge(env, chunks, names, frames)
        held_to_the_scalar_encoder(env, chunks, names, frames, checksum)
        for nm, f in zip(names, frames):
            info = X.frame_info(f, env.model(nm))
            assert info["checksum"] == checksum and info["dict_id"] == env.model(nm)["id"]
            if info["block"] == 2:
                seen.add(("treeless" if info["lit_type"] == X.TREELESS else "own_literals"))
                seen |= {"repeat_mode"} if X.REPEAT in info["modes"] else set()
    assert {"treeless", "own_literals", "repeat_mode"} <= seen


# ------------------------------------------------------------------------------------------------- the planned parse
def planned_chunk(tail: bytes, seed: int, plan):
    """plan: ("lit", n) | ("tail", v, ml): a copy of history[v', v' + ml), v' the first position of the tail at or behind v that is the
    greatest of its table slot (the copy may run on into the chunk) |
    ("back", distance, ml): a copy from `distance` bytes back.  -> (chunk, tokens), from the first seed at or after `seed`
    at which no lookup that matters is ambiguous: every 4 bytes at a literal position occur nowhere before it in the
    history, those at a match's start only at its source, whose table slot no later position of the history shares;
    a source in the chunk lies in a literal run at least 128 positions back (an earlier trip stored it); the byte behind
    a match differs from the one behind its source."""
    T = len(tail)
    last_of_slot = set(v for v in X.prime_table(tail) if v) if T else set()
    for s in range(seed, seed + 200):
        rnd = random.Random(s)
        hist, tokens, ll, starts, interior = bytearray(tail), [], 0, {}, set()
        for p in plan:
            if p[0] == "lit":
                hist += bytes(rnd.randrange(256) for _ in range(p[1]))
                ll += p[1]
                continue
            src = p[1] if p[0] == "tail" else len(hist) - p[1]
            while p[0] == "tail" and src not in last_of_slot:   # (the primed slot holds the greatest position: take such a one)
                src += 1
            at = len(hist)
            for k in range(p[2]):
                hist.append(hist[src + k])
            starts[at] = src
            interior |= set(range(at + 1, at + p[2]))
            tokens.append((ll, p[2], at - src))
            ll = 0
        grams, hashes = {}, []
        for q in range(len(hist) - 3):
            grams.setdefault(bytes(hist[q:q + 4]), []).append(q)
            hashes.append(X.hash_of(int.from_bytes(hist[q:q + 4], "little")))
        searchable = lambda x: (x >= T and x not in interior) or x + 4 <= T   # (a match's inside is never stored)
        lengths = dict(zip(starts, (t[1] for t in tokens)))
        ok = True
        for q in range(T, len(hist) - 3):
            if q in interior:
                continue
            before = [x for x in grams[bytes(hist[q:q + 4])] if x < q and searchable(x)]
            if q in starts:
                src, ml = starts[q], lengths[q]
                # the slot still holds the source: no position behind it shares the slot, nor one stored along with it
                rivals = [x for x in range(src - 63 if src >= T else src + 1, q) if x != src and x >= 0 and searchable(x) and hashes[x] == hashes[q]]
                ok = ok and before == [src] and not rivals
                ok = ok and (src < T or (q - src >= 128 and src not in interior))
                ok = ok and (q + ml == len(hist) or hist[q + ml] != hist[src + ml])
            else:
                ok = ok and not before
        if ok:
            return bytes(hist[T:]), tokens
    raise AssertionError("no seed gives an unambiguous plan")


def test_the_planned_parse(env):
    """chunks planned so that no lookup that matters is ambiguous: the kernel's tokens are the planned ones -- a match
    wholly in the tail, at its first and at its last searchable position, ending at its last byte, crossing into the
    chunk, from earlier in the chunk; T = 32768 (of 40000), 8 and 0"""
    plans = []
    for dname in ("raw_big", "content_32768"):
        T = 32768
        plans.append((dname, T, [("lit", 100), ("tail", 1000, 20), ("lit", 80), ("tail", T - 12, 12), ("lit", 90), ("tail", T - 6, 16),
                                 ("lit", 70), ("back", 200, 9), ("lit", 10)]))
        plans.append((dname, T, [("lit", 70), ("tail", 0, 12), ("lit", 100), ("tail", T - 4, 4), ("lit", 5)]))
        # an offset beyond 59000: behind one long match, whose inside leaves the table alone (literals in between would
        # take the slot of any far source)
        plans.append((dname, T, [("lit", 70), ("tail", 4000, 28000), ("lit", 3), ("tail", 0, 10), ("lit", 5)]))
    plans.append(("content_8", 8, [("lit", 80), ("tail", 0, 8), ("lit", 140), ("back", 150, 6), ("lit", 3)]))
    plans.append(("content_7", 0, [("lit", 150), ("back", 140, 30), ("lit", 9)]))
    plans.append((None, 0, [("lit", 150), ("back", 140, 30), ("lit", 9)]))
    chunks, names, want = [], [], []
    for k, (dname, T, plan) in enumerate(plans):
        content = env.model(dname)["content"] if dname else b""
        assert X.tail_len(len(content)) == T
        chunk, tokens = planned_chunk(content[len(content) - T:], 100 * k, plan)
        chunks.append(chunk)
        names.append(dname)
        want.append(tokens)
    frames, _ = compress_guarded(env, chunks, names, offsets=(0, 7), checksum=True)
    judge(env, chunks, names, frames)
    got = held_to_the_scalar_encoder(env, chunks, names, frames, True)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, names[k], g, w)
    assert any(off > 59000 for t in want for _, _, off in t)


def test_a_null_blob_is_the_plain_encoder(env):
    """chunks with device_prepared_dicts[i] == NULL: the bytes of ZstdEncoder on the same chunks, in the same process"""
    hc, torch, dev = env.hc, env.torch, env.dev
    cases = [(n, c) for n, c, d in round_trip_cases(env) if d in (None, "a")]
    chunks = [c for _, c in cases]
    for checksum in (False, True):
        frames, _ = compress_guarded(env, chunks, [None] * len(chunks), offsets=(0, 5, 11), checksum=checksum)
        plain = hc.batch.ZstdEncoder(checksum=checksum).compress(hc.batch.from_host_chunks(chunks, dev), MAX)
        torch.cuda.synchronize()
        assert frames == plain.to_host_chunks()


def test_determinism_and_mixing(env):
    """the same chunk under the same blob: identical bytes at different batch positions, among different neighbours, at
    other addresses and in a second call; different blobs give frames that decode only with their own dictionary"""
    data = F.inputs({"a": env.bytes_of("a")})
    x, y = data["r5000"], data["b5000"]
    a = [x, x, y, x, b"", x]
    na = ["a", "b", "b", "raw", "a", "a"]
    fa, _ = compress_guarded(env, a, na, offsets=(0, 3, 9))
    fa2, _ = compress_guarded(env, a, na, offsets=(0, 3, 9))
    fb, _ = compress_guarded(env, [y, x, x, x], ["b", "raw", "a", "b"], offsets=(5, 1), turn=1)
    assert fa == fa2
    assert fa[0] == fa[5] == fb[2] and fa[1] == fb[3] and fa[3] == fb[1] and fa[2] == fb[0]
    assert len({fa[0], fa[1], fa[3]}) == 3
    judge(env, a, na, fa)
    # the other dictionary: refused by the Dictionary_ID rule
    st, sz, _ = judge(env, [x, x, y], ["b", "a", "a"], [fa[0], fa[1], fa[2]], expect_ok=False)
    assert st == [CANNOT] * 3 and sz == [0] * 3
    if D.libzstd() is not None:
        assert D.arbiter(fa[0], len(x), env.bytes_of("b")) is None and D.arbiter(fa[1], len(x), env.bytes_of("a")) is None


def test_the_dictionary_pays(env):
    """200 records of about 300 bytes: smaller in sum under dictionary "a" than without one (a strict floor); at least one
    frame uses the dictionary's tables"""
    hc, torch, dev = env.hc, env.torch, env.dev
    recs = [b"\n".join(F.records(5000 + i, F.VOCAB_A, 2)) for i in range(200)]
    print("record bytes: mean %.0f" % (sum(map(len, recs)) / len(recs)))
    frames, sizes = compress_guarded(env, recs, ["a"] * len(recs))
    judge(env, recs, ["a"] * len(recs), frames)
    plain = hc.batch.ZstdEncoder().compress(hc.batch.from_host_chunks(recs, dev), MAX)
    torch.cuda.synchronize()
    with_dict, without = sum(sizes), int(plain.sizes.sum().item())
    line = "sum of frames: %d with dictionary a, %d without" % (with_dict, without)
    if D.libzstd() is not None:
        line += "; libzstd level 1: %d with, %d without" % (sum(len(D.compress(r, 1, env.bytes_of("a"))) for r in recs),
                                                            sum(len(D.compress(r, 1, b"")) for r in recs))
    print(line)
    assert with_dict < without
    infos = [X.frame_info(f, env.model("a")) for f in frames]
    uses = sum(1 for i in infos if i["block"] == 2 and (i["lit_type"] == X.TREELESS or X.REPEAT in i["modes"]))
    print("frames with Treeless literals or a Repeat_Mode table: %d of %d" % (uses, len(frames)))
    assert uses >= 1


# --------------------------------------------------------------------------------------------------- remaining cases
def test_graph_capture(env):
    """warm, capture on a side stream, replay twice onto cleared output: the bytes of the direct call"""
    hc, torch, dev = env.hc, env.torch, env.dev
    cases = round_trip_cases(env)[::5]
    chunks, names = [c for _, c, _ in cases], [d for _, _, d in cases]
    n = len(chunks)
    want, _ = compress_guarded(env, chunks, names, checksum=True)
    src = hc.batch.from_host_chunks(chunks, dev)
    enc = hc.batch.ZstdDictEncoder(checksum=True)
    prepared = torch.tensor([env.ptr(nm) for nm in names], dtype=torch.int64, device=dev)
    dst = hc.batch.alloc_batch(n, enc.max_output_chunk_size(MAX), dev, fill=0xEE)
    temp = torch.empty(max(enc.compress_temp_size(n, MAX), 8), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert enc.compress_async(src, MAX, temp, dst, prepared) == 0   # warm: the code object is loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert enc.compress_async(src, MAX, temp, dst, prepared) == 0
    for _ in range(2):
        dst.data.fill_(0xEE)
        dst.sizes.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert dst.to_host_chunks() == want


def test_an_oversized_chunk_and_an_invalid_blob_are_left_alone(env):
    """a chunk above the call's max chunk size, and chunks that name a blob marked invalid: size 0, not a byte of their
    slots written, their neighbours compressed as ever"""
    data = F.inputs({"a": env.bytes_of("a")})["r5000"]
    refused = [n for n, ok in zip(env.names, env.legal) if not ok][:2]
    chunks = [data[:1000], data[:3000], data[1000:1900], data[:1001], b"", data[:500], data[:700]]
    names = ["a", "a", "raw", None, "a", refused[0], refused[1]]
    frames, sizes = compress_guarded(env, chunks, names, max_chunk=1000, offsets=(0, 6), untouched=(1, 3, 5, 6))
    kept = [0, 2, 4]
    judge(env, [chunks[i] for i in kept], [names[i] for i in kept], [frames[i] for i in kept])
    alone, _ = compress_guarded(env, [chunks[i] for i in kept], [names[i] for i in kept], max_chunk=1000)
    assert alone == [frames[i] for i in kept]


def test_the_grid_stride_trip(env):
    """3073 tiny chunks, one more than the grid's waves, against three dictionaries and none in turn"""
    hc, torch, dev = env.hc, env.torch, env.dev
    rec = F.records(77, F.VOCAB_A, 40)
    n = 3073
    chunks = [rec[i % 40][: 20 + i % 50] for i in range(n)]
    names = [("a", "b", "raw", None)[i % 4] for i in range(n)]
    src = hc.batch.from_host_chunks(chunks, dev)
    before = src.data.clone()
    prepared = torch.tensor([env.ptr(nm) for nm in names], dtype=torch.int64, device=dev)
    comp = hc.batch.ZstdDictEncoder(checksum=True).compress(src, prepared, 80)
    dec_prepared = torch.tensor([env.dec_ptr(nm) for nm in names], dtype=torch.int64, device=dev)
    dec, actual, statuses = hc.batch.ZstdDictDecoder().decompress(comp, 80, dec_prepared)
    torch.cuda.synchronize()
    assert torch.equal(src.data, before)
    assert bool((statuses == 0).all()) and torch.equal(actual, src.sizes)
    assert bool((comp.sizes > 0).all()) and bool((comp.sizes <= src.sizes + 18).all())
    assert dec.to_host_chunks() == chunks
