"""quick_parquet_dict.py [--items N] [--rows V] [--reps R] [--big-mib M]: time one gather_parquet_dictionary or
gather_parquet_dictionary_strings call of the Cascaded manager against two things: a device-to-device copy of as many
bytes as the call's outputs take (the ceiling that memory sets), and what a user does without the call: copy indices,
levels and dictionary to the host, gather there with one thread (the functions of
hipcomp-core_amd/csrc/parquet_dict_plan.hpp, compiled -O2), copy the outputs back.

Builds tests/parquet_dict_driver.cpp (with its host path) against include/ and lib/libhipcomp.so and runs its `time`
command per case: N items (default 4096) of V rows (default 5000) each, 16 different sets of indices taken in turn, every item with arrays and outputs of its own, all items on one dictionary (as the pages of a column chunk are).
With levels every seventh row is null.
  fixed4_dense_small, fixed4_levels_small    4-byte entries, a dictionary of 1024 entries (4 KiB: it stays in the caches)
  fixed8_dense_small, fixed8_levels_small    8-byte entries, 1024 entries
  fixed4_levels_big, fixed8_levels_big       a dictionary of M MiB (default 512: larger than the caches), uniform indices
  strings_short                              1024 entries of 0 to 8 bytes, with levels
  strings_mixed                              1000 such entries and 24 of 1, 63, 64, 65 and 300 bytes, with levels
HIP events around each way, the three alternating inside every repetition, 2 warm-ups and R timed repetitions (default
10), medians; the copies and the host's gather are inside today's time.  `same`: the call and the host wrote the same
bytes and every status is success.  DESIGN.md section 29 and profiles/r20_parquet_dict.txt are where a run on an MI355X
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
ap.add_argument("--rows", type=int, default=5000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--big-mib", type=int, default=512)
a = ap.parse_args()

import parquet_dictgen as G  # noqa: E402

KINDS = 16
rng = random.Random(20)
tmp = tempfile.mkdtemp(prefix="quick_parquet_dict")
exe = os.path.join(tmp, "parquet_dict_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-DDICT_HOST_PATH", "-I", os.path.join(ROOT, "include"),
                "-I", os.path.join(ROOT, "hipcomp-core_amd", "csrc"), os.path.join(ROOT, "tests", "parquet_dict_driver.cpp"),
                "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe], check=True, timeout=600)

levels = bytes(0 if r % 7 == 0 else 1 for r in range(a.rows))
valid = levels.count(1)
short = [rng.randbytes(rng.randrange(0, 9)) for _ in range(1024)]
mixed = short[:1000] + [rng.randbytes(n) for n in (1, 63, 64, 65, 300, 300) * 4]
big = a.big_mib << 20
# name -> (kind, entry_bytes, has_levels, the dictionary's body, its entries)
cases = [("fixed4_dense_small", G.FIXED, 4, 0, rng.randbytes(4096), 1024), ("fixed4_levels_small", G.FIXED, 4, 1, rng.randbytes(4096), 1024),
         ("fixed8_dense_small", G.FIXED, 8, 0, rng.randbytes(8192), 1024), ("fixed8_levels_small", G.FIXED, 8, 1, rng.randbytes(8192), 1024),
         ("fixed4_levels_big", G.FIXED, 4, 1, None, big // 4), ("fixed8_levels_big", G.FIXED, 8, 1, None, big // 8),
         ("strings_short", G.STRINGS, 0, 1, G.byte_array_body(short), 1024), ("strings_mixed", G.STRINGS, 0, 1, G.byte_array_body(mixed), 1024)]
big_body = None
for name, kind, entry_bytes, has_levels, body, entries in cases:
    if body is None:
        big_body = body = big_body or b"".join(rng.randbytes(min(1 << 24, big - at)) for at in range(0, big, 1 << 24))
    count = valid if has_levels else a.rows
    blob = bytearray(body)
    offsets, listed = b"", None
    if kind == G.STRINGS:
        listed = G.index_dictionary(body, entries, entries + 1)
        offsets = struct.pack("<%di" % len(listed), *listed)
    at_offsets = len(blob)
    blob += offsets
    at_levels = len(blob)
    blob += levels
    at_indices, totals = [], []
    for _ in range(KINDS):
        picks = [rng.randrange(entries) for _ in range(count)]
        at_indices.append(len(blob))
        blob += struct.pack("<%dI" % count, *picks)
        totals.append(sum(listed[k + 1] - listed[k] for k in picks) if listed else 0)   # (the byte capacity: exact)
    pool = os.path.join(tmp, name + ".bin")
    with open(pool, "wb") as f:
        f.write(blob)
    lines = ["case %s %d %d 0 0 0 %s %d" % (kind, entry_bytes, has_levels, os.path.join(tmp, "unused.out"), a.items)]
    for i in range(a.items):
        words = [kind, 0, len(body), entries]
        if kind == G.STRINGS:
            words += [at_offsets, entries + 1]
        words += [at_indices[i % KINDS], count, has_levels, at_levels, a.rows, 1]
        words += [a.rows, entry_bytes] if kind == G.FIXED else [a.rows + 1, totals[i % KINDS]]
        lines.append(" ".join(str(w) for w in words))
    path = os.path.join(tmp, name + ".list")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "time", pool, path, str(a.reps)], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %s: %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
    print(name, r.stdout.strip(), flush=True)
    if " same 1 " not in r.stdout:
        sys.exit("%s: the call and the host path did not write the same bytes, or a status is no success" % name)
