"""Quick timing of the Zstandard decoder with dictionaries (lib/libhipcomp_zstd_dict.so) on one GPU:
   quick_zstd_dict.py [--chunks N] [--records N] [--reps R] [--parent-lib FILE] [--out FILE]
HIP events around single launches, warmed up, the jobs alternating launch by launch inside one loop of one process.

(a) The cost of the dictionary plumbing: hipcompBatchedZstdDictDecompressAsync with all-null blobs on N x 64 KiB chunks
    of the bench's TPC-H-like text (libzstd level 3), against hipcompBatchedZstdDecompressAsync on the same frames, the
    latter as TWO jobs so that their difference shows the run-to-run spread.  --parent-lib names a libhipcomp_zstd.so built
    from the parent commit; without it the tree's own is used (its two kernels have the parent's instruction streams,
    DESIGN.md section 18).
(b) The dictionary decode rate: --records records of about 4 KiB that ZSTD_compress_usingDict compressed at level 3 with a
    16 KiB dictionary trained by ZDICT_trainFromBuffer, decoded with the prepared dictionary; GB/s of output, and the
    time of the prepare launch.
libzstd (libzstd.so.1 through ctypes) makes a sample of distinct chunks (256 by default); the batch repeats them.  If
libzstd does not load here, the script says so and stops."""
import argparse, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import bench
import zstd_dict_fixtures as F
import zstd_dictgen as D
import zstd_framegen as G

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--records", type=int, default=100000)
ap.add_argument("--distinct", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if D.libzstd() is None:
    print("libzstd.so.1 does not load here: nothing to decode, nothing timed")
    sys.exit(0)
hc = importlib.import_module("hipcomp-core_amd")
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Job:
    """n chunks (the distinct streams repeated) decoded into slots of `cap` bytes; blobs: the per-chunk prepared
    dictionaries of a ZstdDictDecoder, None for a ZstdDecoder"""

    def __init__(self, dec, streams, sources, n, cap, blobs=None):
        k = len(streams)
        self.dec, self.sources, self.k, self.n, self.cap, self.blobs = dec, sources, k, n, cap, blobs
        table = hc.batch.from_host_chunks(streams, dev)
        pick = torch.arange(n, device=dev) % k
        data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
        self.comp = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, n, table.stride), table.sizes[pick], table.stride)
        self.dst = hc.batch.alloc_batch(n, cap, dev)
        self.caps = torch.full((n,), cap, dtype=torch.int64, device=dev)
        self.actual = torch.zeros(n, dtype=torch.int64, device=dev)
        self.statuses = torch.zeros(n, dtype=torch.int32, device=dev)
        self.temp = torch.empty(max(dec.decompress_temp_size(n, cap), 8), dtype=torch.uint8, device=dev)
        self.ms = []

    def launch(self):
        args = (self.comp, self.caps, self.actual, self.temp, self.dst, self.statuses)
        assert (self.dec.decompress_async(*args) if self.blobs is None else self.dec.decompress_async(*args, self.blobs)) == 0

    def verify(self):
        torch.cuda.synchronize()
        assert bool((self.statuses == 0).all())
        for i in (0, self.k - 1, self.n - 1):
            assert self.dst.chunk_bytes(i, int(self.actual[i].item())) == self.sources[i % self.k]

    def timed(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.launch()
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(e0.elapsed_time(e1))

    def report(self, name):
        ms, out_bytes = self.ms, float(self.actual.sum().item())
        ratio = out_bytes / float(self.comp.sizes.sum().item())
        say(f"{name} n={self.n} ({out_bytes / self.n:.0f} B a chunk, ratio {ratio:.3f}): decode min {min(ms):.3f} ms median "
            f"{sorted(ms)[len(ms) // 2]:.3f} ms max {max(ms):.3f} ms -> {out_bytes / min(ms) / 1e6:.1f} GB/s of output (best of {a.reps})")
        return min(ms), sorted(ms)[len(ms) // 2]


def run(jobs):
    for _ in range(2):   # warm-up
        for _, j in jobs:
            j.launch()
    for _, j in jobs:
        j.verify()
    for _ in range(a.reps):   # alternating inside one loop of one process
        for _, j in jobs:
            j.timed()
    return [j.report(name) for name, j in jobs]


# (a) null blobs against the decoder without dictionaries, that one measured twice
CH = bench.CHUNK
text = bench.gen_text(a.distinct * CH)
sources = [text[i * CH:(i + 1) * CH].tobytes() for i in range(a.distinct)]
frames = [G.compress(s, 3) for s in sources]
plain_lib = hc.api.ZstdLibrary(a.parent_lib) if a.parent_lib else None
which = "parent build" if a.parent_lib else "this tree's build"
ddec = hc.batch.ZstdDictDecoder()
null = torch.zeros(a.chunks, dtype=torch.int64, device=dev)
(p1, p1m), (d0, d0m), (p2, p2m) = run([
    (f"(a) zstd.h, {which}, first", Job(hc.batch.ZstdDecoder(plain_lib), frames, sources, a.chunks, CH)),
    ("(a) zstd_dict.h, all-null blobs", Job(ddec, frames, sources, a.chunks, CH, null)),
    (f"(a) zstd.h, {which}, second", Job(hc.batch.ZstdDecoder(plain_lib), frames, sources, a.chunks, CH))])
say(f"(a) spread of the two zstd.h jobs: min {abs(p1 - p2) / min(p1, p2) * 100:.2f} %, median {abs(p1m - p2m) / min(p1m, p2m) * 100:.2f} %; "
    f"null blobs against their mean: min {(d0 / ((p1 + p2) / 2) - 1) * 100:+.2f} %, median {(d0m / ((p1m + p2m) / 2) - 1) * 100:+.2f} %")
torch.cuda.empty_cache()

# (b) records of about 4 KiB with a 16 KiB trained dictionary
dictionary = D.train(F.records(1, F.VOCAB_A, 4000), 16 * 1024)
recs = [b"\n".join(F.records(100 + i, F.VOCAB_A, 70))[:4096] for i in range(a.distinct)]
comp = [D.compress(r, 3, dictionary) for r in recs]
plain = [G.compress(r, 3) for r in recs]
dicts = hc.batch.from_host_chunks([dictionary], dev)
blobs = hc.batch.alloc_batch(1, ddec.prepared_size(len(dictionary)), dev)
blob_caps = torch.full((1,), ddec.prepared_size(len(dictionary)), dtype=torch.int64, device=dev)
statuses = torch.full((1,), -1, dtype=torch.int32, device=dev)
prepare_ms = []
for rep in range(2 + a.reps):    # two warm-up launches
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert ddec.prepare_async(dicts, blobs, blob_caps, statuses) == 0
    e1.record()
    torch.cuda.synchronize()
    if rep >= 2:
        prepare_ms.append(e0.elapsed_time(e1))
assert statuses.cpu().tolist() == [0]
say(f"(b) prepare launch of one {len(dictionary)} B dictionary (one wave): min {min(prepare_ms):.3f} ms median {sorted(prepare_ms)[len(prepare_ms) // 2]:.3f} ms")
per_chunk = blobs.ptrs[0].repeat(a.records)
say(f"(b) a record of {len(recs[0])} B: {len(comp[0])} B with the dictionary, {len(plain[0])} B without")
run([("(b) zstd_dict.h, 4 KiB records, level 3, 16 KiB dictionary", Job(ddec, comp, recs, a.records, 4096, per_chunk)),
     ("(b) zstd.h, the same records without a dictionary", Job(hc.batch.ZstdDecoder(), plain, recs, a.records, 4096))])
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
