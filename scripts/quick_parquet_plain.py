"""quick_parquet_plain.py [--items N] [--rows V] [--reps R]: time one place_parquet_values, place_parquet_booleans or
place_parquet_strings call of the Cascaded manager against two things: a device-to-device copy of as many bytes as the
call's outputs take (the ceiling that memory sets), and what a user does without the call: copy the sources, the levels
and the offsets to the host, place the values there with one thread (the functions of
hipcomp-core_amd/csrc/parquet_plain_plan.hpp, compiled -O2), copy the outputs back.

Builds tests/parquet_plain_driver.cpp (with its host path) against include/ and lib/libhipcomp.so and runs its `time`
command per case: N items (default 4096) of V rows (default 5000) each, 16 different sources taken in turn, every item
with outputs of its own.  With levels every seventh row is null.
  values4_dense_plain, values4_levels_plain, values4_dense_split, values4_levels_split    4-byte values
  values8_dense_plain, values8_levels_plain, values8_dense_split, values8_levels_split    8-byte values
  values12_levels_plain                      12-byte values (INT96), in units of 4 bytes
  booleans_levels                            PLAIN BOOLEAN bits to a values bitmap
  strings_short_prefixed                     values of 0 to 8 bytes, length-prefixed, with levels
  strings_mixed_prefixed, strings_mixed_packed   such values with one in 40 of 1, 63, 64, 65 or 300 bytes, under both layouts
HIP events around each way, the three alternating inside every repetition, 2 warm-ups and R timed repetitions (default
10), medians; the copies and the host's placing are inside today's time.  `same`: the call and the host wrote the same
bytes and every status is success.  DESIGN.md section 30 and profiles/r21_parquet_plain.txt are where a run on an MI355X
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
a = ap.parse_args()

import parquet_dictgen as DG  # noqa: E402
import parquet_plaingen as G  # noqa: E402

KINDS = 16
rng = random.Random(21)
tmp = tempfile.mkdtemp(prefix="quick_parquet_plain")
exe = os.path.join(tmp, "parquet_plain_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-DPLAIN_HOST_PATH", "-I", os.path.join(ROOT, "include"),
                "-I", os.path.join(ROOT, "hipcomp-core_amd", "csrc"), os.path.join(ROOT, "tests", "parquet_plain_driver.cpp"),
                "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe], check=True, timeout=600)

levels = bytes(0 if r % 7 == 0 else 1 for r in range(a.rows))
LONG = (1, 63, 64, 65, 300)


def words(count, mixed):
    return [rng.randbytes(LONG[k % 5] if mixed and k % 40 == 7 else rng.randrange(0, 9)) for k in range(count)]


# name, kind, value_bytes, layout, has_levels, mixed strings
cases = [("values%d_%s_%s" % (w, "levels" if lv else "dense", G.LAYOUT_NAME[y]), G.VALUES, w, y, lv, False)
         for w in (4, 8) for y in (G.PLAIN, G.SPLIT) for lv in (0, 1)]
cases += [("values12_levels_plain", G.VALUES, 12, G.PLAIN, 1, False), ("booleans_levels", G.BOOLEANS, 0, 0, 1, False),
          ("strings_short_prefixed", G.STRINGS, 0, G.LENGTH_PREFIXED, 1, False),
          ("strings_mixed_prefixed", G.STRINGS, 0, G.LENGTH_PREFIXED, 1, True), ("strings_mixed_packed", G.STRINGS, 0, G.PACKED, 1, True)]
for name, kind, value_bytes, layout, has_levels, mixed in cases:
    count = levels.count(1) if has_levels else a.rows
    blob = bytearray(levels)
    sources = []                             # (place, bytes, place of the offsets, their count, the byte total)
    for _ in range(KINDS):
        at_offsets, offsets = 0, []
        if kind == G.VALUES:
            body = rng.randbytes(count * value_bytes)       # (split or not: the bytes are random either way)
        elif kind == G.BOOLEANS:
            body = rng.randbytes((count + 7) // 8)
        else:
            there = words(count, mixed)
            body = DG.byte_array_body(there) if layout == G.LENGTH_PREFIXED else b"".join(there)
            offsets = DG.offsets_of(there)
            at_offsets = len(blob)
            blob += struct.pack("<%di" % len(offsets), *offsets)
        sources.append((len(blob), len(body), at_offsets, len(offsets), offsets[-1] if offsets else 0))
        blob += body
    pool = os.path.join(tmp, name + ".bin")
    with open(pool, "wb") as f:
        f.write(blob)
    lines = ["case %s %d %d %d 0 0 0 %s %d" % (kind, value_bytes, layout, has_levels, os.path.join(tmp, "unused.out"), a.items)]
    for i in range(a.items):
        at, size, at_offsets, num_offsets, total = sources[i % KINDS]
        line = [kind, at, size, 0, count, has_levels, 0, a.rows, 1]
        if kind == G.VALUES:
            line += [a.rows, value_bytes, layout]
        elif kind == G.BOOLEANS:
            line += [a.rows]
        else:
            line += [at_offsets, num_offsets, a.rows + 1, total, layout]
        lines.append(" ".join(str(w) for w in line))
    path = os.path.join(tmp, name + ".list")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "time", pool, path, str(a.reps)], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %s: %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
    print(name, r.stdout.strip(), flush=True)
    if " same 1 " not in r.stdout:
        sys.exit("%s: the call and the host path did not write the same bytes, or a status is no success" % name)
