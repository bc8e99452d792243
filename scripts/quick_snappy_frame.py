"""quick_snappy_frame.py [--chunks N] [--reps R]: time the Snappy manager's framed-stream methods against its
container methods.

Builds tests/snappy_frame_driver.cpp against include/ and lib/libhipcomp.so and runs its `timing` command on the
bench's text data (bench.gen_text) and on uniform random bytes (N x 64 KiB, default 100 000): compress_frame /
decompress_frame against compress / decompress of the same manager, the calls alternating inside every repetition, HIP
events, 2 warm-up and R timed repetitions (default 10), NoComputeNoVerify and ComputeAndVerify.  Random bytes do not
compress, so their stream holds stored chunks only: that run's decompress_frame is the serial walk, the scan and a
copy.  Then `timing_read` on a stream made here on the CPU: 1024 stored chunks of 64 KiB with 1024 one-byte padding
chunks between them.  Prints one table with the ratio container / framed beside each row; DESIGN.md section 21 and
profiles/r12_snappy_frame.txt are where a run on an MI355X is recorded."""
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
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

import bench  # noqa: E402
import snappy_framegen as G  # noqa: E402

tmp = tempfile.mkdtemp(prefix="quick_snappy_frame")
exe = os.path.join(tmp, "snappy_frame_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                os.path.join(ROOT, "tests", "snappy_frame_driver.cpp"), "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe],
               check=True)


def run(*args):
    r = subprocess.run([exe, *[str(x) for x in args]], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %s\n%s" % (args, r.stderr[-2000:]))
    return r.stdout.splitlines()


rows = []
for name in ("uniform", "text"):
    path = "-"
    if name == "text":
        path = os.path.join(tmp, "text.bin")
        with open(path, "wb") as f:
            f.write(bench.gen_text(a.chunks * 65536).tobytes())
    for line in run("timing", path, a.chunks, a.reps):
        w = line.split()
        if "median_ms" in w and len(w) == 8:
            frame, cont = float(w[4]), float(w[7])
            rows.append("%-8s policy %s %-18s %9.4f ms   %-12s %9.4f ms   container/framed %.2f" % (
                name, w[1], w[2], frame, w[5], cont, cont / frame))
        else:
            rows.append("%-8s %s" % (name, line))
    print("\n".join(rows[-6:]), flush=True)
pieces = [G.noise(65536, k) for k in range(1024)]
stream = [G.IDENTIFIER]
for piece, crc in zip(pieces, G.crc32c_many(pieces)):
    stream += [G.stored_chunk(piece, G.mask(crc)), G.padding(1)]
path = os.path.join(tmp, "stored_and_padding.sz")
with open(path, "wb") as f:
    f.write(b"".join(stream))
for line in run("timing_read", path, a.reps):
    rows.append("%-36s %s" % ("stored_64KiB_x1024_with_padding", line))
    print(rows[-1], flush=True)
