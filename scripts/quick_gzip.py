"""Quick timing of the gzip / zlib entry points against the raw Deflate calls they wrap, on one GPU:
   quick_gzip.py [--chunks N] [--reps R] [--out FILE]
On N x 64 KiB chunks of the bench's TPC-H-like text and of random bytes: hipcompBatchedGzipCompressAsync (gzip and
zlib) against hipcompBatchedDeflateCompressAsync, and hipcompBatchedGzipDecompressAsync (gzip and zlib) against
hipcompBatchedDeflateDecompressAsync, HIP events around each call, 2 warm-up and R timed launches, best and median.
The three calls of a comparison alternate inside one loop of the same process, so that they meet the same machine.
The raw calls are the yardstick: what the wrapper adds is the framing kernels and one checksum pass over the
uncompressed bytes.  The batch repeats a sample of distinct chunks (256 by default), as scripts/quick_deflate.py does."""
import argparse, importlib, os, sys, zlib
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
codecs = {w: hc.batch.GzipCodec(w) for w in ("gzip", "zlib")}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_in_turn(fns):
    """{name: fn} -> {name: (best ms, median ms)}, the calls alternating"""
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(a.reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: (min(v), sorted(v)[len(v) // 2]) for name, v in ms.items()}


def report(what, times, total):
    raw_best = times["raw"][0]
    for name, (best, median) in times.items():
        extra = "" if name == "raw" else f"  (+{best - raw_best:.3f} ms, {100 * (best / raw_best - 1):+.1f} % on the raw call)"
        say(f"  {what} {name:4s}: min {best:.3f} ms median {median:.3f} ms -> {total / best / 1e6:.1f} GB/s of uncompressed bytes{extra}")


def row(name, sources):
    k = len(sources)
    n = a.chunks
    total = n * CH
    table = hc.batch.from_host_chunks(sources, dev)
    pick = torch.arange(n, device=dev) % k
    data = table.data[: k * table.stride].view(k, table.stride)[pick].contiguous().view(-1)
    src = hc.batch.ChunkBatch(data, hc.batch.make_ptrs(data, n, table.stride), table.sizes[pick], table.stride)
    say(f"{name}, n={n} x {CH} B (best of {a.reps}):")

    outs = {"raw": hc.batch.alloc_batch(n, enc.max_output_chunk_size(CH), dev)}
    temps = {"raw": torch.empty(max(enc.compress_temp_size(n, CH), 8), dtype=torch.uint8, device=dev)}
    for w, c in codecs.items():
        outs[w] = hc.batch.alloc_batch(n, c.max_output_chunk_size(CH), dev)
        temps[w] = torch.empty(max(c.compress_temp_size(n, CH), 8), dtype=torch.uint8, device=dev)

    def compress_with(coder, w):
        def go():
            assert coder.compress_async(src, CH, temps[w], outs[w]) == 0
        return go
    fns = {"raw": compress_with(enc, "raw")}
    fns.update({w: compress_with(c, w) for w, c in codecs.items()})
    report("compress", timed_in_turn(fns), total)
    for i in (0, k - 1, n - 1):
        assert zlib.decompress(outs["raw"].chunk_bytes(i), -15) == sources[i % k]
        assert zlib.decompress(outs["gzip"].chunk_bytes(i), 31) == sources[i % k]
        assert zlib.decompress(outs["zlib"].chunk_bytes(i), 15) == sources[i % k]
    assert torch.equal(outs["gzip"].sizes, outs["raw"].sizes + 18) and torch.equal(outs["zlib"].sizes, outs["raw"].sizes + 6)

    out = hc.batch.alloc_batch(n, CH, dev)
    caps = torch.full((n,), CH, dtype=torch.int64, device=dev)
    actual = torch.zeros(n, dtype=torch.int64, device=dev)
    statuses = torch.zeros(n, dtype=torch.int32, device=dev)
    dtemp = torch.empty(max(codecs["gzip"].decompress_temp_size(n, CH), 8), dtype=torch.uint8, device=dev)

    def check():
        torch.cuda.synchronize()
        assert bool((statuses == 0).all()) and bool((actual == CH).all())
        assert torch.equal(out.data[: n * CH].view(n, CH), data.view(n, table.stride)[:, :CH])
        out.data.zero_()
        statuses.fill_(-1)

    def raw_decompress():
        assert dec.decompress_async(outs["raw"], caps, actual, None, out, statuses) == 0

    def decompress_with(w):
        def go():
            assert codecs[w].decompress_async(outs[w], caps, actual, dtemp, out, statuses) == 0
        return go
    fns = {"raw": raw_decompress, "gzip": decompress_with("gzip"), "zlib": decompress_with("zlib")}
    for fn in fns.values():   # every route returns the chunks before any is timed
        fn()
        check()
    report("decompress", timed_in_turn(fns), total)


text = bench.gen_text(a.distinct * CH)
row("tpch text", [text[i * CH:(i + 1) * CH].tobytes() for i in range(a.distinct)])
rng = np.random.default_rng(1)
row("random bytes", [rng.integers(0, 256, CH, dtype=np.uint8).tobytes() for _ in range(a.distinct)])
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
