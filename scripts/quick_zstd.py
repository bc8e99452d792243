"""Quick Zstandard decode timing of the built companion library on one GPU:
   quick_zstd.py [--chunks N] [--reps R] [--out FILE]
Times hipcompBatchedZstdDecompressAsync with HIP events on N x 64 KiB chunks of the bench's TPC-H-like text
compressed by libzstd at level 3 on the host, and on N chunks of random bytes (libzstd then writes raw blocks).  In
the same loop of the same process, alternating launch by launch: hipcompBatchedDeflateDecompressAsync on the same
text at zlib level 6.  For context: one host thread of ZSTD_decompress over a sample of the same chunks.  libzstd
(libzstd.so.1 through ctypes) compresses a sample of distinct chunks (256 by default); the batch repeats them.  If
libzstd does not load here, the script says so and stops."""
import argparse, importlib, os, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import bench
import zstd_framegen as G

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--distinct", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if G.libzstd() is None:
    print("libzstd.so.1 does not load here: nothing to decode, nothing timed")
    sys.exit(0)
hc = importlib.import_module("hipcomp-core_amd")
dev = torch.device("cuda:0")
CH = bench.CHUNK
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Job:
    def __init__(self, dec, streams, sources):
        k = len(streams)
        self.dec, self.sources, self.k = dec, sources, k
        table = hc.batch.from_host_chunks(streams, dev)
        pick = torch.arange(a.chunks, device=dev) % k
        data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
        self.comp = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, a.chunks, table.stride), table.sizes[pick], table.stride)
        self.dst = hc.batch.alloc_batch(a.chunks, CH, dev)
        self.caps = torch.full((a.chunks,), CH, dtype=torch.int64, device=dev)
        self.actual = torch.zeros(a.chunks, dtype=torch.int64, device=dev)
        self.statuses = torch.zeros(a.chunks, dtype=torch.int32, device=dev)
        tbytes = dec.decompress_temp_size(a.chunks, CH)
        self.temp = torch.empty(tbytes, dtype=torch.uint8, device=dev) if tbytes else None
        self.ms = []

    def launch(self):
        assert self.dec.decompress_async(self.comp, self.caps, self.actual, self.temp, self.dst, self.statuses) == 0

    def verify(self):
        torch.cuda.synchronize()
        assert bool((self.statuses == 0).all()) and bool((self.actual == CH).all())
        for i in (0, self.k - 1, a.chunks - 1):
            assert self.dst.chunk_bytes(i, CH) == self.sources[i % self.k]

    def timed(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.launch()
        e1.record()
        torch.cuda.synchronize()
        self.ms.append(e0.elapsed_time(e1))

    def report(self, name):
        ms, out_bytes = self.ms, a.chunks * CH
        ratio = out_bytes / float(self.comp.sizes.sum().item())
        say(f"{name} n={a.chunks} x {CH} B (ratio {ratio:.3f}): decode min {min(ms):.3f} ms median {sorted(ms)[len(ms) // 2]:.3f} ms "
            f"max {max(ms):.3f} ms -> {out_bytes / min(ms) / 1e6:.1f} GB/s of output (best of {a.reps})")


def raw_deflate(s):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    return c.compress(s) + c.flush()


text = bench.gen_text(a.distinct * CH)
sources = [text[i * CH:(i + 1) * CH].tobytes() for i in range(a.distinct)]
rng = np.random.default_rng(1)
noise = [rng.integers(0, 256, CH, dtype=np.uint8).tobytes() for _ in range(a.distinct)]
frames = [G.compress(s, 3) for s in sources]
jobs = [("zstd tpch text (libzstd level 3)", Job(hc.batch.ZstdDecoder(), frames, sources)),
        ("deflate tpch text (zlib level 6)", Job(hc.batch.DeflateDecoder(), [raw_deflate(s) for s in sources], sources)),
        ("zstd random bytes (raw blocks)", Job(hc.batch.ZstdDecoder(), [G.compress(s, 3) for s in noise], noise))]
for _ in range(2):   # warm-up
    for _, j in jobs:
        j.launch()
for _, j in jobs:
    j.verify()
for _ in range(a.reps):   # alternating inside one loop of one process
    for _, j in jobs:
        j.timed()
for name, j in jobs:
    j.report(name)
t0, n_host = time.perf_counter(), 0
while time.perf_counter() - t0 < 1.0:
    for f in frames:
        G.arbiter(f, CH)
    n_host += len(frames)
say(f"one host thread of ZSTD_decompress on the same text chunks: {n_host * CH / (time.perf_counter() - t0) / 1e9:.3f} GB/s of output")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
