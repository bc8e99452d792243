"""Quick Zstandard compress timing of the built companion library on one GPU:
   quick_zstd_compress.py [--chunks N] [--reps R] [--out FILE]
Times hipcompBatchedZstdCompressAsync with HIP events (2 warm-up launches, R timed ones, best and median) on
N x 64 KiB chunks of the bench's TPC-H-like text and of random bytes, and the decode of the new frames by
ZstdDecoder.  For context, in the same process and on the same chunks: this library's Deflate, Snappy and LZ4
encoders, and one host thread of libzstd at levels -1, 1 and 3 where libzstd.so.1 loads.  The batch repeats a
sample of distinct chunks (256 by default), as scripts/quick_deflate_compress.py does."""
import argparse, importlib, os, sys, time
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
hc = importlib.import_module("hipcomp-core_amd")
dev = torch.device("cuda:0")
CH = bench.CHUNK
dec = hc.batch.ZstdDecoder()
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


def host_libzstd(sources, level):
    if G.libzstd() is None:
        say(f"  libzstd.so.1 does not load here: no host figure at level {level}")
        return
    t0, n, out = time.perf_counter(), 0, 0
    for s in sources:
        out += len(G.compress(s, level))
        n += len(s)
        if time.perf_counter() - t0 > 2.0:
            break
    dt = time.perf_counter() - t0
    say(f"  one host thread of libzstd level {level} on the same chunks: {n / dt / 1e9:.3f} GB/s of input, ratio {n / out:.3f}")


def row(name, sources):
    k = len(sources)
    table = hc.batch.from_host_chunks(sources, dev)
    pick = torch.arange(a.chunks, device=dev) % k
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, a.chunks, table.stride), table.sizes[pick], table.stride)
    total = a.chunks * CH
    for label, enc in (("zstd", hc.batch.ZstdEncoder()), ("zstd with checksum", hc.batch.ZstdEncoder(checksum=True)),
                       ("deflate", hc.batch.DeflateEncoder())):
        dst = hc.batch.alloc_batch(a.chunks, enc.max_output_chunk_size(CH), dev)
        temp = torch.empty(max(enc.compress_temp_size(a.chunks, CH), 8), dtype=torch.uint8, device=dev)

        def compress():
            assert enc.compress_async(src, CH, temp, dst) == 0
        best, median = timed(compress)
        ratio = total / float(dst.sizes.sum().item())
        say(f"{label} compress {name} n={a.chunks} x {CH} B: min {best:.3f} ms median {median:.3f} ms -> "
            f"{total / best / 1e6:.2f} GB/s of input, ratio {ratio:.3f} (temp {temp.numel() / 2**20:.0f} MiB, best of {a.reps})")
        if label == "deflate":
            continue
        if G.libzstd() is not None:
            for i in (0, k - 1, a.chunks - 1):
                assert G.arbiter(dst.chunk_bytes(i), CH) == sources[i % k]
        out = hc.batch.alloc_batch(a.chunks, CH, dev)
        caps = torch.full((a.chunks,), CH, dtype=torch.int64, device=dev)
        actual = torch.zeros(a.chunks, dtype=torch.int64, device=dev)
        statuses = torch.zeros(a.chunks, dtype=torch.int32, device=dev)
        dtemp = torch.empty(max(dec.decompress_temp_size(a.chunks, CH), 8), dtype=torch.uint8, device=dev)

        def decompress():
            assert dec.decompress_async(dst, caps, actual, dtemp, out, statuses) == 0
        best, median = timed(decompress)
        assert bool((statuses == 0).all()) and bool((actual == CH).all())
        assert torch.equal(out.data[: a.chunks * CH].view(a.chunks, CH), data.view(a.chunks, table.stride)[:, :CH])
        say(f"  ZstdDecoder on these frames: min {best:.3f} ms median {median:.3f} ms -> {total / best / 1e6:.1f} GB/s of output")
        del out, dst, temp
    for level in (-1, 1, 3):
        host_libzstd(sources, level)
    flat = data.view(a.chunks, table.stride)[:, :CH].contiguous().view(-1)
    for codec, opts in (("Snappy", hc.SnappyOpts(0)), ("LZ4", hc.LZ4Opts(hc.hipcompType.CHAR))):
        job = bench.CodecJob(hc, hc.default_library(), codec, opts, flat)
        job.compress(); job.decompress(); torch.cuda.synchronize()
        job.verify()
        tc, td = bench.time_phases(job, a.reps)
        say(f"  {codec} (this library) on the same chunks n={job.n}: compress min {min(tc):.3f} ms -> {job.total / min(tc) / 1e6:.1f} GB/s of input "
            f"(ratio {job.total / job.compressed_bytes():.3f})")
        del job


text = bench.gen_text(a.distinct * CH)
row("tpch text", [text[i * CH:(i + 1) * CH].tobytes() for i in range(a.distinct)])
rng = np.random.default_rng(1)
row("random bytes", [rng.integers(0, 256, CH, dtype=np.uint8).tobytes() for _ in range(a.distinct)])
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
