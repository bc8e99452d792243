"""Quick Deflate compress timing of the built companion library on one GPU:
   quick_deflate_compress.py [--chunks N] [--reps R] [--out FILE]
Times hipcompBatchedDeflateCompressAsync with HIP events (2 warm-up launches, R timed ones, best and median) on
N x 64 KiB chunks of the bench's TPC-H-like text and of random bytes, and the decode of the new streams by
DeflateDecoder.  For context, in the same run and on the same chunks: one host thread of zlib at level 1, level 6
and level 1 with Z_FIXED, and this library's Snappy and LZ4 encoders on the same text.  The batch repeats a sample
of distinct chunks (256 by default), as scripts/quick_deflate.py does."""
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
enc, dec = hc.batch.DeflateEncoder(), hc.batch.DeflateDecoder()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), sorted(ms)[len(ms) // 2]


def host_zlib(name, sources, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    t0, n, out = time.perf_counter(), 0, 0
    for s in sources:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        out += len(c.compress(s) + c.flush())
        n += len(s)
        if time.perf_counter() - t0 > 2.0:
            break
    dt = time.perf_counter() - t0
    say(f"  one host thread of zlib {name} on the same chunks: {n / dt / 1e9:.3f} GB/s of input, ratio {n / out:.3f}")


def row(name, sources):
    k = len(sources)
    table = hc.batch.from_host_chunks(sources, dev)
    pick = torch.arange(a.chunks, device=dev) % k
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, a.chunks, table.stride), table.sizes[pick], table.stride)
    dst = hc.batch.alloc_batch(a.chunks, enc.max_output_chunk_size(CH), dev)
    temp = torch.empty(max(enc.compress_temp_size(a.chunks, CH), 8), dtype=torch.uint8, device=dev)

    def compress():
        assert enc.compress_async(src, CH, temp, dst) == 0
    best, median = timed(compress)
    total = a.chunks * CH
    ratio = total / float(dst.sizes.sum().item())
    for i in (0, k - 1, a.chunks - 1):
        assert zlib.decompress(dst.chunk_bytes(i), -15) == sources[i % k]
    say(f"deflate compress {name} n={a.chunks} x {CH} B: min {best:.3f} ms median {median:.3f} ms -> "
        f"{total / best / 1e6:.2f} GB/s of input, ratio {ratio:.3f} (temp {temp.numel() / 2**20:.0f} MiB, best of {a.reps})")
    out = hc.batch.alloc_batch(a.chunks, CH, dev)
    caps = torch.full((a.chunks,), CH, dtype=torch.int64, device=dev)
    actual = torch.zeros(a.chunks, dtype=torch.int64, device=dev)
    statuses = torch.zeros(a.chunks, dtype=torch.int32, device=dev)

    def decompress():
        assert dec.decompress_async(dst, caps, actual, None, out, statuses) == 0
    best, median = timed(decompress)
    assert bool((statuses == 0).all()) and bool((actual == CH).all())
    assert torch.equal(out.data[: a.chunks * CH].view(a.chunks, CH), data.view(a.chunks, table.stride)[:, :CH])
    say(f"  DeflateDecoder on these streams: min {best:.3f} ms median {median:.3f} ms -> {total / best / 1e6:.1f} GB/s of output")
    host_zlib("level 1", sources, 1)
    host_zlib("level 6", sources, 6)
    host_zlib("level 1 Z_FIXED", sources, 1, zlib.Z_FIXED)


text = bench.gen_text(a.distinct * CH)
row("tpch text", [text[i * CH:(i + 1) * CH].tobytes() for i in range(a.distinct)])
rng = np.random.default_rng(1)
row("random bytes", [rng.integers(0, 256, CH, dtype=np.uint8).tobytes() for _ in range(a.distinct)])

data = torch.from_numpy(np.tile(text, (a.chunks + a.distinct - 1) // a.distinct)[: a.chunks * CH]).to(dev)
for codec, opts in (("Snappy", hc.SnappyOpts(0)), ("LZ4", hc.LZ4Opts(hc.hipcompType.CHAR))):
    job = bench.CodecJob(hc, hc.default_library(), codec, opts, data)
    job.compress(); job.decompress(); torch.cuda.synchronize()
    job.verify()
    tc, td = bench.time_phases(job, a.reps)
    say(f"{codec} (this library) on the same text n={job.n}: compress min {min(tc):.3f} ms -> {job.total / min(tc) / 1e6:.1f} GB/s of input "
        f"(ratio {job.total / job.compressed_bytes():.3f})")
    del job
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
