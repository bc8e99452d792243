"""quick_parquet_hybrid.py [--items N] [--values V] [--reps R]: time one decode_parquet_hybrid call of the Cascaded manager
against two things: a device-to-device copy of as many bytes as the call writes (the ceiling that memory sets), and what
a user does without the call: copy the streams to the host, decode them there with one thread (the decoder of
hipcomp-core_amd/csrc/parquet_hybrid_plan.hpp, compiled -O2), copy the values back.

Builds tests/parquet_hybrid_driver.cpp (with its host decoder) against include/ and lib/libhipcomp.so and runs its `time`
command per case: N items (default 4096) of V values (default 5000) each, written by tests/parquet_hybridgen.py, 16
different streams taken in turn, every item at an address of its own.
  index_w1, index_w6, index_w12   dictionary indices behind their width byte, as parquet-mr cuts them: bit-packed runs of at
                                  most 504 values, an RLE run where a value repeats (about one run in five)
  index_w12_uint                  the same streams decoded to 4-byte elements
  index_w12_long_runs             one bit-packed run per stream, as pyarrow writes where nothing repeats
  levels_short_runs               definition levels (width 1) of a mostly valid column: RLE runs of 1 to 40 values and
                                  bit-packed runs of 1 to 3 groups alternating, behind their 4-byte length
HIP events around each way, the three alternating inside every repetition, 2 warm-ups and R timed repetitions (default
10), medians; the copies and the host's decode are inside today's time.  `same`: the call and the host wrote the same
values and every status is success.  DESIGN.md section 27 and profiles/r18_parquet_hybrid.txt are where a run on an MI355X
is recorded."""
import argparse
import os
import random
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=4096)
ap.add_argument("--values", type=int, default=5000)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

import parquet_hybridgen as G  # noqa: E402

KINDS = 16


def index_stream(rng, w, values, most):
    parts, done = [bytes([w])], 0
    while done < values:
        if most and rng.random() < 0.2:
            c = min(rng.randrange(8, 400), values - done)
            parts.append(G.rle(c, rng.getrandbits(w), w))
        else:
            c = min(most or values, values - done)
            parts.append(G.packed([rng.getrandbits(w) for _ in range(c)], w))
        done += c
    return b"".join(parts)


def level_stream(rng, values):
    parts, done = [], 0
    while done < values:
        c = min(rng.randrange(1, 41), values - done)
        parts.append(G.rle(c, 1, 1))
        done += c
        if done < values:
            c = min(8 * rng.randrange(1, 4), values - done)
            parts.append(G.packed([rng.getrandbits(1) for _ in range(c)], 1))
            done += c
    runs = b"".join(parts)
    return struct.pack("<I", len(runs)) + runs


rng = random.Random(18)
cases = [("index_w1", G.WIDTH_PREFIXED, G.UCHAR, [index_stream(rng, 1, a.values, 504) for _ in range(KINDS)]),
         ("index_w6", G.WIDTH_PREFIXED, G.UCHAR, [index_stream(rng, 6, a.values, 504) for _ in range(KINDS)]),
         ("index_w12", G.WIDTH_PREFIXED, G.USHORT, [index_stream(rng, 12, a.values, 504) for _ in range(KINDS)])]
cases.append(("index_w12_uint", G.WIDTH_PREFIXED, G.UINT, cases[2][3]))
cases.append(("index_w12_long_runs", G.WIDTH_PREFIXED, G.USHORT, [index_stream(rng, 12, a.values, 0) for _ in range(KINDS)]))
cases.append(("levels_short_runs", G.LENGTH_PREFIXED, G.UCHAR, [level_stream(rng, a.values) for _ in range(KINDS)]))

tmp = tempfile.mkdtemp(prefix="quick_parquet_hybrid")
exe = os.path.join(tmp, "parquet_hybrid_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-DHYBRID_HOST_DECODER", "-I", os.path.join(ROOT, "include"),
                "-I", os.path.join(ROOT, "hipcomp-core_amd", "csrc"), os.path.join(ROOT, "tests", "parquet_hybrid_driver.cpp"),
                "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe], check=True, timeout=600)
for name, form, element, streams in cases:
    width = 1 if form == G.LENGTH_PREFIXED else 0
    assert all(G.model(s, form, width, a.values, a.values, element)[0] == G.SUCCESS for s in streams[:2])
    pool = os.path.join(tmp, name + ".bin")
    with open(pool, "wb") as f:
        f.write(b"".join(streams))
    starts = [sum(len(s) for s in streams[:k]) for k in range(KINDS)]
    lines = ["case %d %d 0 0 0 %s %d" % (form, element, os.path.join(tmp, "unused.out"), a.items)]
    lines += ["%s %d %d %d %d %d 1" % (pool, starts[i % KINDS], len(streams[i % KINDS]), width, a.values, a.values) for i in range(a.items)]
    path = os.path.join(tmp, name + ".list")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "time", path, str(a.reps)], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %s: %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
    print(name, r.stdout.strip(), flush=True)
