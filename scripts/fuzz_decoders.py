"""Damaged LZ4, Snappy and Cascaded streams (tests/decode_guard.py: bytes changed, inserted, removed, streams cut
short, LZ4 offset pairs, and for Cascaded every place its decoder trusts) decoded on the GPU and by the CPU oracle:
status, reported size and -- on success -- bytes must agree.   fuzz_decoders.py [--per-source N]"""
import argparse, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import datagen
import decode_guard as G
from oracle import oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--per-source", type=int, default=400)
a = ap.parse_args()
hc = importlib.import_module("hipcomp-core_amd")

sources = [datagen.text_like(31, 6000), datagen.harness_like_int32(32, 1500).tobytes(),
           datagen.random_runs_int32(33, 1500).tobytes(), datagen.vocabulary_text(34, 6000, 64, 8),
           datagen.periodic_bytes(35, 5000, 3, 40), datagen.small_alphabet_bytes(36, 5000, 3),
           datagen.tpch_lineitem_text(37, 6000)]
bad = 0
rng = np.random.default_rng(2025)
for codec_name, comp_fn, dec_fn in (("LZ4", lambda s: O.lz4_compress(s, 1, 65536), O.lz4_decompress),
                                    ("Snappy", O.snappy_compress, O.snappy_decompress),
                                    ("Cascaded", None, O.cascaded_decompress)):
    streams = []
    if codec_name == "Cascaded":
        streams = [s for s, *_ in G.cascaded_corpus(O, 2025, a.per_source // 20)]
    else:
        for src in sources:
            good = comp_fn(src)
            streams += [good] + G.damaged(codec_name, good, rng, a.per_source)
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
