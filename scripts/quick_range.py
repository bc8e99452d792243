"""quick_range.py [--chunks N] [--reps R] [--lib DIR]: decompress_range of the LZ4 manager against decompress of the
same container (N x 64 KiB uniform random bytes, default 100 000), HIP events around each call: ranges of 1 byte, one
chunk's worth, 1 % and 50 % of the buffer, none aligned to chunks, under NoComputeNoVerify and ComputeAndVerify.
Builds tests/hlif_range_driver.cpp against include/ and the library in DIR (default hipcomp-core_amd/lib) and runs its
`timing` command as a child process; DESIGN.md section 12 quotes its output."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--lib", default=os.path.join(ROOT, "hipcomp-core_amd", "lib"))
a = ap.parse_args()
lib = os.path.abspath(a.lib)
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "hlif_range_driver")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hlif_range_driver.cpp"), "-L", lib, "-lhipcomp", "-Wl,-rpath," + lib, "-o", exe],
                   check=True)
    sys.exit(subprocess.run([exe, "timing", str(a.chunks), str(a.reps)], timeout=900).returncode)
