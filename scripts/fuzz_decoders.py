"""Damaged LZ4, Snappy and Cascaded streams (tests/decode_guard.py: bytes changed, inserted, removed, streams cut
short, LZ4 offset pairs, and for Cascaded every place its decoder trusts) decoded on the GPU and by the CPU oracle:
status, reported size and -- on success -- bytes must agree.  The good LZ4 and Snappy streams come from the encoder
(--good encoder), from the valid-stream families of tests/streamgen.py (--good streamgen: their streams of at most
8 KiB of output, each with --per-source / 20 damaged copies) or from both.
   fuzz_decoders.py [--per-source N] [--good encoder|streamgen|both]"""
import argparse, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import datagen
import decode_guard as G
import streamgen as SG
from oracle import oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--per-source", type=int, default=400)
ap.add_argument("--good", choices=("encoder", "streamgen", "both"), default="encoder")
a = ap.parse_args()
hc = importlib.import_module("hipcomp-core_amd")

sources = [datagen.text_like(31, 6000), datagen.harness_like_int32(32, 1500).tobytes(),
           datagen.random_runs_int32(33, 1500).tobytes(), datagen.vocabulary_text(34, 6000, 64, 8),
           datagen.periodic_bytes(35, 5000, 3, 40), datagen.small_alphabet_bytes(36, 5000, 3),
           datagen.tpch_lineitem_text(37, 6000)]
bad = 0
rng = np.random.default_rng(2025)


def streamgen_goods(codec_name):
    """The generator's valid streams of at most 8 KiB of output (both LZ4 kinds)."""
    if codec_name == "LZ4":
        cases = [c for fam in SG.LZ4_FAMILIES for kind in (True, False) for c in SG.lz4_family(fam, kind)]
    else:
        cases = [c for fam in SG.SNAPPY_FAMILIES for c in SG.snappy_family(fam)]
    return [s for s, e, _ in cases if len(e) <= 8192]


for codec_name, comp_fn, dec_fn in (("LZ4", lambda s: O.lz4_compress(s, 1, 65536), O.lz4_decompress),
                                    ("Snappy", O.snappy_compress, O.snappy_decompress),
                                    ("Cascaded", None, O.cascaded_decompress)):
    streams = []
    if codec_name == "Cascaded":
        streams = [s for s, *_ in G.cascaded_corpus(O, 2025, a.per_source // 20)]
    else:
        if a.good != "streamgen":
            for src in sources:
                good = comp_fn(src)
                streams += [good] + G.damaged(codec_name, good, rng, a.per_source)
        if a.good != "encoder":
            for good in streamgen_goods(codec_name):
                streams += [good] + G.damaged(codec_name, good, rng, max(a.per_source // 20, 1))
    for cap in (6000, 3500):
        comp = hc.batch.from_host_chunks(streams, "cuda:0")
        dec, actual, statuses = hc.batch.Codec(codec_name).decompress(comp, cap)
        torch.cuda.synchronize()
        st, ac = statuses.cpu().tolist(), actual.cpu().tolist()
        wrong = 0
        for i, s in enumerate(streams):
            ost, obytes = dec_fn(s, cap)
            if st[i] != ost or ac[i] != len(obytes) or (ost == 0 and dec.chunk_bytes(i, ac[i]) != obytes):
                wrong += 1
                if wrong <= 3:
                    print("MISMATCH", codec_name, cap, i, st[i], ost, ac[i], len(obytes))
        print(f"{codec_name} cap={cap}: {len(streams)} streams, {wrong} differ", flush=True)
        bad += wrong
print("TOTAL BAD", bad)
sys.exit(1 if bad else 0)
