"""quick_parquet_delta.py [--items N] [--values V] [--reps R]: time one decode_parquet_delta call of the Cascaded manager
against two things: a device-to-device copy of as many bytes as the call writes (the ceiling that memory sets), and what
a user does without the call: copy the streams to the host, decode them there with one thread (the decoder of
hipcomp-core_amd/csrc/parquet_delta_plan.hpp, compiled -O2), copy the elements back.

Builds tests/parquet_delta_driver.cpp (with its host decoder) against include/ and lib/libhipcomp.so and runs its `time`
command per case: N items (default 4096) of V values (default 5000) each, written by the encoder of
tests/parquet_deltagen.py, 16 different streams taken in turn, every item at an address of its own.
  int_w6            INT, blocks of 128 in 4 miniblocks of 32 (as pyarrow cuts INT32): steps below 64, widths of about 6
  longlong_w10      LONGLONG, blocks of 256 in 4 miniblocks of 64 (as pyarrow cuts INT64): steps below 1024
  longlong_w40      the same with steps below 2^40
  longlong_w0       a constant column: every width is 0, a block is its header
  offsets_int       the lengths (0 to 8) of a DELTA_LENGTH_BYTE_ARRAY page with its string bytes behind, to INT offsets
HIP events around each way, the three alternating inside every repetition, 2 warm-ups and R timed repetitions (default
10), medians; the copies and the host's decode are inside today's time.  `same`: the call and the host wrote the same
elements and every status is success.  DESIGN.md section 28 and profiles/r19_parquet_delta.txt are where a run on an
MI355X is recorded."""
import argparse
import os
import random
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

import parquet_deltagen as G  # noqa: E402

KINDS = 16


def sums(rng, values, step_bits):
    out, at = [], rng.getrandbits(20)
    for _ in range(values):
        at += rng.getrandbits(step_bits) if step_bits else 0
        out.append(at)
    return out


def lengths_page(rng, values):
    lengths = [rng.randrange(0, 9) for _ in range(values)]
    return G.encode(lengths, 128, 4, 32) + rng.randbytes(sum(lengths))


rng = random.Random(19)
cases = [("int_w6", G.VALUES, G.INT, [G.encode(sums(rng, a.values, 6), 128, 4, 32) for _ in range(KINDS)]),
         ("longlong_w10", G.VALUES, G.LONGLONG, [G.encode(sums(rng, a.values, 10), 256, 4, 64) for _ in range(KINDS)]),
         ("longlong_w40", G.VALUES, G.LONGLONG, [G.encode(sums(rng, a.values, 40), 256, 4, 64) for _ in range(KINDS)]),
         ("longlong_w0", G.VALUES, G.LONGLONG, [G.encode(sums(rng, a.values, 0), 256, 4, 64) for _ in range(KINDS)]),
         ("offsets_int", G.OFFSETS, G.INT, [lengths_page(rng, a.values) for _ in range(KINDS)])]

tmp = tempfile.mkdtemp(prefix="quick_parquet_delta")
exe = os.path.join(tmp, "parquet_delta_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-DDELTA_HOST_DECODER", "-I", os.path.join(ROOT, "include"),
                "-I", os.path.join(ROOT, "hipcomp-core_amd", "csrc"), os.path.join(ROOT, "tests", "parquet_delta_driver.cpp"),
                "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe], check=True, timeout=600)
for name, output, element, streams in cases:
    capacity = a.values + (output == G.OFFSETS)
    assert all(G.model(s, a.values, capacity, output, element)[0] == G.SUCCESS for s in streams[:2])
    pool = os.path.join(tmp, name + ".bin")
    with open(pool, "wb") as f:
        f.write(b"".join(streams))
    starts = [sum(len(s) for s in streams[:k]) for k in range(KINDS)]
    lines = ["case %d %d 0 0 1 0 %s %d" % (output, element, os.path.join(tmp, "unused.out"), a.items)]
    lines += ["%s %d %d %d %d" % (pool, starts[i % KINDS], len(streams[i % KINDS]), a.values, capacity) for i in range(a.items)]
    path = os.path.join(tmp, name + ".list")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "time", path, str(a.reps)], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %s: %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
    print(name, r.stdout.strip(), flush=True)
