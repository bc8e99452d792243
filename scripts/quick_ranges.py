"""quick_ranges.py [--chunks N] [--reps R] [--data uniform|text] [--lib DIR]: one decompress_ranges of the LZ4 manager
against a loop of decompress_range calls and against a decompress of everything, on a container of N x 64 KiB
(default 100 000) of uniform random bytes or of the TPC-H-like text bench.py uses: R = 1, 16, 1024 and 16 384 ranges
of 256 bytes at seeded random places, then a range per chunk that together cover every chunk, under
NoComputeNoVerify and ComputeAndVerify.  Host clock around the call(s) plus the stream synchronisation, the calls
alternating inside every repetition, 2 warm-up repetitions, medians in milliseconds.  Builds
tests/hlif_ranges_driver.cpp against include/ and the library in DIR (default hipcomp-core_amd/lib) and runs its
`timing` command as a child process; DESIGN.md section 24 quotes its output."""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=100000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--data", choices=("uniform", "text"), default="uniform")
ap.add_argument("--lib", default=os.path.join(ROOT, "hipcomp-core_amd", "lib"))
a = ap.parse_args()
lib = os.path.abspath(a.lib)
with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "hlif_ranges_driver")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hlif_ranges_driver.cpp"), "-L", lib, "-lhipcomp", "-Wl,-rpath," + lib, "-o", exe],
                   check=True)
    extra = []
    if a.data == "text":
        # 64 MiB of the benchmark's text, which the driver repeats to the size asked for
        gen = ctypes.CDLL(os.path.join(ROOT, "benchdata", "libbenchdata.so"))
        n = min(a.chunks * 65536, 64 << 20)
        buf = ctypes.create_string_buffer(n)
        gen.benchdata_tpch_lineitem_text.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int]
        gen.benchdata_tpch_lineitem_text(buf, n, 1, 8)
        path = os.path.join(tmp, "text.bin")
        with open(path, "wb") as f:
            f.write(buf.raw)
        extra = [path]
    print("data", a.data, "chunks", a.chunks, "reps", a.reps, flush=True)
    sys.exit(subprocess.run([exe, "timing", str(a.chunks), str(a.reps), *extra], timeout=900).returncode)
