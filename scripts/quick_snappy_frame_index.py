"""quick_snappy_frame_index.py [--chunks N] [--reps R]: time the Snappy manager's read of a seekable framed stream
against its read of the same stream without an index and against decompress of the container.

Builds tests/snappy_frame_index_driver.cpp against include/ and lib/libhipcomp.so and runs its `timing` command on
uniform random bytes as incompressible as the bench's and on the bench's text data (bench.gen_text), N x 64 KiB
(default 100 000): decompress_frame of the stream compress_frame(..., SnappyFrameIndex::Leading) wrote,
decompress_frame of the stream compress_frame wrote, and decompress, the calls alternating inside every repetition,
HIP events, 2 warm-up and R timed repetitions (default 10), medians, NoComputeNoVerify and ComputeAndVerify.  The two
writes are timed in the same loop, and so are decompress_frame_range of 1 MiB from the middle of the indexed stream,
the read of the stream without an index after another buffer was configured (the indexed passes are then launched
and refuse on the device) and configure_frame_decompression itself (host clock).  What a read finds in the caches
depends on the calls before it, so the stream without an index is also timed in the calls and the order of
quick_snappy_frame.py (`timing_plain`), once configured last and once with another buffer configured behind it: these
are the figures to compare with quick_snappy_frame.py's decompress_frame on a build without the index.  `walked` is
the number of data chunks decompress_frame found by following the chain: 0 for the indexed stream.  DESIGN.md
section 23 and profiles/r13_snappy_frame_index.txt are where a run on an MI355X is recorded."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

import bench  # noqa: E402

tmp = tempfile.mkdtemp(prefix="quick_snappy_frame_index")
exe = os.path.join(tmp, "snappy_frame_index_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                os.path.join(ROOT, "tests", "snappy_frame_index_driver.cpp"), "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe],
               check=True)

for name in ("uniform", "text"):
    rows = []
    path = "-"
    if name == "text":
        path = os.path.join(tmp, "text.bin")
        with open(path, "wb") as f:
            f.write(bench.gen_text(a.chunks * 65536).tobytes())
    r = subprocess.run([exe, "timing", path, str(a.chunks), str(a.reps)], capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        sys.exit("driver failed: %s\n%s" % (name, r.stderr[-2000:]))
    indexed = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[2] == "decompress_frame_indexed":
            indexed[w[1]], plain, cont = float(w[4]), float(w[7]), float(w[10])
            rows.append("%-8s policy %s decompress_frame indexed %9.4f ms   unindexed %9.4f ms   decompress %9.4f ms   "
                        "indexed/unindexed %.3f   indexed/decompress %.2f" % (name, w[1], indexed[w[1]], plain, cont,
                                                                              indexed[w[1]] / plain, indexed[w[1]] / cont))
        elif w[2] == "decompress_frame_plain_displaced":
            rows.append("%-8s policy %s decompress_frame unindexed, another buffer configured last %9.4f ms   "
                        "configure_frame_decompression unindexed %9.4f ms   indexed %9.4f ms" % (
                            name, w[1], float(w[4]), float(w[7]), float(w[10])))
        elif w[2] == "compress_frame_indexed":
            rows.append("%-8s policy %s compress_frame   indexed %9.4f ms   unindexed %9.4f ms   decompress_frame_range of 1 MiB %9.4f ms   "
                        "range/indexed read %.4f" % (name, w[1], float(w[4]), float(w[7]), float(w[10]), float(w[10]) / indexed[w[1]]))
        else:
            rows.append("%-8s %s" % (name, line))
    # the stream without an index in the calls and the order of quick_snappy_frame.py: the figures to hold against that
    # script's on another build of the library
    for how in ("configured", "displaced"):
        r = subprocess.run([exe, "timing_plain", path, str(a.chunks), str(a.reps), how], capture_output=True, text=True, timeout=1200)
        if r.returncode != 0:
            sys.exit("driver failed: %s\n%s" % (name, r.stderr[-2000:]))
        for line in r.stdout.splitlines():
            w = line.split()
            rows.append("%-8s policy %s decompress_frame unindexed, %s, in quick_snappy_frame.py's order of calls %9.4f ms "
                        "(min %.4f max %.4f, walked %s)" % (name, w[1], "configured last" if how == "configured" else
                                                            "another buffer configured last", float(w[4]), float(w[6]), float(w[8]), w[16]))
    print("\n".join(rows), flush=True)
