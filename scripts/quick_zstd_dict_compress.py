"""Quick timing of the Zstandard encoder with dictionaries (lib/libhipcomp_zstd_dict_compress.so) on one GPU:
   quick_zstd_dict_compress.py [--records N] [--distinct K] [--reps R] [--out FILE]
HIP events around single launches, 2 warm-up and --reps timed launches, the jobs alternating launch by launch inside one
loop of one process; the dictionary job is run twice so that the difference of the two shows the run-to-run spread.

Jobs, all on --records records of 4096 bytes (the record kind of DESIGN.md section 18 (b)):
  * hipcompBatchedZstdDictCompressAsync under one 16 KiB dictionary trained by ZDICT_trainFromBuffer (twice);
  * hipcompBatchedZstdCompressAsync on the same records;
  * hipcompBatchedZstdDictCompressAsync with all-null blobs (the same frames as the job above).
Printed: times, GB/s of input, compressed bytes per record, libzstd level 1 and 3 sizes with and without the dictionary,
and the prepare launch's time.  If libzstd does not load here there is no dictionary to train: the script says so and stops."""
import argparse, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import zstd_dict_fixtures as F
import zstd_dictgen as D

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=100000)
ap.add_argument("--distinct", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if D.libzstd() is None:
    print("libzstd.so.1 does not load here: no dictionary is trained, nothing timed")
    sys.exit(0)
hc = importlib.import_module("hipcomp-core_amd")
dev = torch.device("cuda:0")
lines = []
REC = 4096


def say(s):
    print(s, flush=True)
    lines.append(s)


dictionary = D.train(F.records(1, F.VOCAB_A, 4000), 16 * 1024)
recs = [b"\n".join(F.records(100 + i, F.VOCAB_A, 70))[:REC] for i in range(a.distinct)]
k, n = len(recs), a.records
table = hc.batch.from_host_chunks(recs, dev)
pick = torch.arange(n, device=dev) % k
data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, n, table.stride), table.sizes[pick], table.stride)
in_bytes = float(src.sizes.sum().item())

denc = hc.batch.ZstdDictEncoder()
dicts = hc.batch.from_host_chunks([dictionary], dev)
size = denc.prepared_size(len(dictionary))
blobs = hc.batch.alloc_batch(1, size, dev)
caps = torch.full((1,), size, dtype=torch.int64, device=dev)
statuses = torch.full((1,), -1, dtype=torch.int32, device=dev)
prepare_ms = []
for rep in range(2 + a.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    assert denc.prepare_async(dicts, blobs, caps, statuses) == 0
    e1.record()
    torch.cuda.synchronize()
    if rep >= 2:
        prepare_ms.append(e0.elapsed_time(e1))
assert statuses.cpu().tolist() == [0]
say(f"prepare launch of one {len(dictionary)} B dictionary (one wave, blob of {size} B): min {min(prepare_ms):.3f} ms median "
    f"{sorted(prepare_ms)[len(prepare_ms) // 2]:.3f} ms")


class Job:
    def __init__(self, enc, prepared=None):
        self.enc, self.prepared = enc, prepared
        self.dst = hc.batch.alloc_batch(n, enc.max_output_chunk_size(REC), dev)
        self.temp = torch.empty(max(enc.compress_temp_size(n, REC), 8), dtype=torch.uint8, device=dev)
        self.ms = []

    def launch(self):
        extra = () if self.prepared is None else (self.prepared,)
        assert self.enc.compress_async(src, REC, self.temp, self.dst, *extra) == 0

    def timed(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.launch()
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(e0.elapsed_time(e1))

    def report(self, name):
        ms = self.ms
        out = float(self.dst.sizes.sum().item())
        say(f"{name} n={n}: min {min(ms):.3f} ms median {sorted(ms)[len(ms) // 2]:.3f} ms max {max(ms):.3f} ms -> "
            f"{in_bytes / min(ms) / 1e6:.1f} GB/s of input (best of {a.reps}), {out / n:.1f} compressed B a record")
        return min(ms), sorted(ms)[len(ms) // 2]


per_chunk = blobs.ptrs[0].repeat(n)
null = torch.zeros(n, dtype=torch.int64, device=dev)
jobs = [("zstd_dict_compress.h, 16 KiB dictionary, first", Job(denc, per_chunk)),
        ("zstd_compress.h, no dictionary", Job(hc.batch.ZstdEncoder())),
        ("zstd_dict_compress.h, all-null blobs", Job(denc, null)),
        ("zstd_dict_compress.h, 16 KiB dictionary, second", Job(denc, per_chunk))]
for _ in range(2):
    for _, j in jobs:
        j.launch()
torch.cuda.synchronize()
# the frames come back: the dictionary job's through libzstd, the null job's are the plain encoder's
frames = jobs[0][1].dst.to_host_chunks()[:k]
for r, f in zip(recs, frames):
    assert D.arbiter(f, len(r), dictionary) == r
assert jobs[1][1].dst.to_host_chunks()[:k] == jobs[2][1].dst.to_host_chunks()[:k]
for _ in range(a.reps):
    for _, j in jobs:
        j.timed()
(d1, d1m), (p, pm), (z, zm), (d2, d2m) = [j.report(name) for name, j in jobs]
say(f"spread of the two dictionary jobs: min {abs(d1 - d2) / min(d1, d2) * 100:.2f} %, median {abs(d1m - d2m) / min(d1m, d2m) * 100:.2f} %; "
    f"all-null blobs against zstd_compress.h: min {(z / p - 1) * 100:+.2f} %, median {(zm / pm - 1) * 100:+.2f} %; "
    f"with the dictionary against zstd_compress.h: min {((d1 + d2) / 2 / p - 1) * 100:+.2f} %")
mean = lambda xs: sum(xs) / len(xs)
say("libzstd, mean compressed B a record: level 1 %.1f with the dictionary, %.1f without; level 3 %.1f with, %.1f without" % (
    mean([len(D.compress(r, 1, dictionary)) for r in recs]), mean([len(D.compress(r, 1, b"")) for r in recs]),
    mean([len(D.compress(r, 3, dictionary)) for r in recs]), mean([len(D.compress(r, 3, b"")) for r in recs])))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
