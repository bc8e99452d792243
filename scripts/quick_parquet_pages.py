"""quick_parquet_pages.py [--chunks N ...] [--reps R] [--bytes B] [--page P]: time one decompress_parquet_pages call of
the Snappy manager against what a user does without it: walk the page headers on the host from a host copy of the same
chunks, copy the lists of the compressed parts to the device, make one hipcompBatchedSnappyDecompressAsync over all of
them.

Builds tests/parquet_pages_driver.cpp against include/ and lib/libhipcomp.so and runs its `time` command: N column
chunks (default 64 and 512) of B bytes (default 262144) of the bench's text (bench.gen_text) each, cut into V1 data pages
of P bytes (default 8192) with a CRC each by the writer of tests/parquet_pagegen.py; the pages are compressed with
pyarrow's Snappy where pyarrow is there, else written as literals (the output says which).  16 different chunks, taken
in turn, every item at an address of its own.  HIP events around each way, the two alternating inside every repetition,
1 warm-up and R timed repetitions (default 10), medians; the host walk and the copies of today's way are inside its
time, as the one synchronisation of the call is inside the call's.  NoComputeNoVerify: today's way checks no CRC either.
`same`: items whose bytes are the same both ways.  DESIGN.md section 26 and profiles/r17_parquet_pages.txt are where a
run on an MI355X is recorded."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, nargs="+", default=[64, 512])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--bytes", type=int, default=262144)
ap.add_argument("--page", type=int, default=8192)
a = ap.parse_args()

import bench  # noqa: E402
import parquet_pagegen as G  # noqa: E402

try:
    import pyarrow
    codec = pyarrow.Codec("snappy")
    compress, how = (lambda part: codec.compress(part).to_pybytes()), "pyarrow " + pyarrow.__version__
except ImportError:
    compress, how = G.snappy_literals, "literals"

tmp = tempfile.mkdtemp(prefix="quick_parquet_pages")
exe = os.path.join(tmp, "parquet_pages_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                os.path.join(ROOT, "tests", "parquet_pages_driver.cpp"), "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe],
               check=True, timeout=600)
kinds = 16
text = bench.gen_text(a.bytes * kinds).tobytes()
chunks = [G.text_chunk(text[k * a.bytes:(k + 1) * a.bytes], a.page, compress) for k in range(kinds)]
assert all(G.model(c, G.SNAPPY, 2)[1] == text[k * a.bytes:(k + 1) * a.bytes] for k, c in enumerate(chunks[:2]))
pool = os.path.join(tmp, "pool.bin")
with open(pool, "wb") as f:
    f.write(b"".join(chunks))
starts = [sum(len(c) for c in chunks[:k]) for k in range(kinds)]
print("pages compressed with", how, "- chunk of", a.bytes, "bytes in pages of", a.page, ":", len(chunks[0]), "bytes")
for n in a.chunks:
    lines = ["case 0 1 own 0 0 0 0 %s %d" % (os.path.join(tmp, "unused.out"), n)]
    lines += ["%s %d %d E E" % (pool, starts[i % kinds], len(chunks[i % kinds])) for i in range(n)]
    path = os.path.join(tmp, "time_%d.list" % n)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "time", path, str(a.reps)], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %d chunks: %d\n%s" % (n, r.returncode, r.stderr[-2000:]))
    print(r.stdout.strip())
