"""Quick Deflate decode timing of the built companion library on one GPU:
   quick_deflate.py [--chunks N] [--reps R] [--out FILE]
Times hipcompBatchedDeflateDecompressAsync with HIP events on N x 64 KiB chunks of the bench's TPC-H-like text
compressed by zlib at level 6, and on N chunks of random bytes (zlib then writes stored blocks).  For context, in
the same run: one host thread of zlib.decompress over a sample of the same chunks, and this library's Snappy
decoder on the same text.  zlib compresses a sample of distinct chunks on the host (256 by default); the batch
repeats them, so that building it does not take longer than measuring it."""
import argparse, importlib, os, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--distinct", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
hc = importlib.import_module("hipcomp-core_amd")
dev = torch.device("cuda:0")
CH = bench.CHUNK
dec = hc.batch.DeflateDecoder()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def deflate_row(name, sources):
    streams = []
    for s in sources:
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
        streams.append(c.compress(s) + c.flush())
    k = len(streams)
    table = hc.batch.from_host_chunks(streams, dev)
    pick = torch.arange(a.chunks, device=dev) % k
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    comp = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, a.chunks, table.stride), table.sizes[pick], table.stride)
    dst = hc.batch.alloc_batch(a.chunks, CH, dev)
    caps = torch.full((a.chunks,), CH, dtype=torch.int64, device=dev)
    actual = torch.zeros(a.chunks, dtype=torch.int64, device=dev)
    statuses = torch.zeros(a.chunks, dtype=torch.int32, device=dev)
    for _ in range(2):   # warm-up
        assert dec.decompress_async(comp, caps, actual, None, dst, statuses) == 0
    torch.cuda.synchronize()
    assert bool((statuses == 0).all()) and bool((actual == CH).all())
    for i in (0, k - 1, a.chunks - 1):
        assert dst.chunk_bytes(i, CH) == sources[i % k]
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decompress_async(comp, caps, actual, None, dst, statuses)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    out_bytes = a.chunks * CH
    ratio = out_bytes / float(comp.sizes.sum().item())
    say(f"deflate {name} n={a.chunks} x {CH} B (zlib level 6, ratio {ratio:.3f}): decode min {min(ms):.3f} ms "
        f"median {sorted(ms)[len(ms) // 2]:.3f} ms max {max(ms):.3f} ms -> {out_bytes / min(ms) / 1e6:.1f} GB/s of output "
        f"(best of {a.reps})")
    t0 = time.perf_counter()
    n_host = 0
    while time.perf_counter() - t0 < 1.0:
        for s in streams:
            zlib.decompress(s, -15)
        n_host += k
    dt = time.perf_counter() - t0
    say(f"  one host thread of zlib.decompress on the same chunks: {n_host * CH / dt / 1e9:.3f} GB/s of output")


text = bench.gen_text(a.distinct * CH)
deflate_row("tpch text", [text[i * CH:(i + 1) * CH].tobytes() for i in range(a.distinct)])
rng = np.random.default_rng(1)
deflate_row("random bytes (stored blocks)", [rng.integers(0, 256, CH, dtype=np.uint8).tobytes() for _ in range(a.distinct)])

data = torch.from_numpy(np.tile(text, (a.chunks + a.distinct - 1) // a.distinct)[: a.chunks * CH]).to(dev)
job = bench.CodecJob(hc, hc.default_library(), "Snappy", hc.SnappyOpts(0), data)
job.compress(); job.decompress(); torch.cuda.synchronize()
job.verify()
tc, td = bench.time_phases(job, a.reps)
say(f"snappy (this library) on the same text n={job.n}: decode min {min(td):.3f} ms -> {job.total / min(td) / 1e6:.1f} GB/s of output "
    f"(ratio {job.total / job.compressed_bytes():.3f})")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
