"""quick_lz4_frame.py [--chunks N] [--reps R]: time the LZ4 manager's frame methods against its container methods.

Builds tests/lz4_frame_driver.cpp against include/ and lib/libhipcomp.so and runs its `timing` command on the
bench's text data (bench.gen_text) and on uniform random bytes as incompressible as the bench's (N x 64 KiB, default
100 000): compress_frame / decompress_frame against compress /
decompress of the same manager, the calls alternating inside every repetition, HIP events, 2 warm-up and R timed
repetitions (default 10), NoComputeNoVerify and ComputeAndVerify.  Then `timing_read` on three frames made here on
the CPU with liblz4 (64 MiB of text as a 4 MiB-block independent frame and as a frame with C.Checksum, 4 MiB of it as
a linked frame), each under a
non-verifying and a verifying policy.  Prints one table with the ratio frame / container beside each row; DESIGN.md
section 20 and profiles/r08_lz4_frame.txt are where a run on an MI355X is recorded."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "lz4_frame"))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

import bench  # noqa: E402

tmp = tempfile.mkdtemp(prefix="quick_lz4_frame")
exe = os.path.join(tmp, "lz4_frame_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                os.path.join(ROOT, "tests", "lz4_frame_driver.cpp"), "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe],
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
            rows.append("%-8s policy %s %-18s %9.4f ms   %-12s %9.4f ms   container/frame %.2f" % (
                name, w[1], w[2], frame, w[5], cont, cont / frame))
        else:
            rows.append("%-8s %s" % (name, line))
try:
    import make_fixtures as F
    text = bench.gen_text(64 << 20).tobytes()
    frames = {"independent_4MiB_blocks": F.one_call(text, code=7, linked=False, bsum=False, csum=False, size=True, level=0),
              # (one wavefront decodes a linked frame, block after block: 4 MiB of it)
              "linked_64KiB_blocks_4MiB": F.one_call(text[:4 << 20], code=4, linked=True, bsum=False, csum=False, size=True, level=0),
              "independent_64KiB_content_checksum": F.one_call(text, code=4, linked=False, bsum=False, csum=True, size=True, level=0)}
    for name, frame in frames.items():
        path = os.path.join(tmp, name + ".lz4")
        with open(path, "wb") as f:
            f.write(frame)
        for line in run("timing_read", path, a.reps):
            rows.append("%-36s %s" % (name, line))
except OSError:
    rows.append("liblz4.so.1 absent: the three liblz4 frames were not made and not timed")
print("\n".join(rows))
