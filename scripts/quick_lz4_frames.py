"""quick_lz4_frames.py [--items N ...] [--reps R]: time one decompress_frames call of the LZ4 manager against the loop
of configure_frame_decompression + decompress_frame over the same items.

Builds tests/lz4_frames_driver.cpp against include/ and lib/libhipcomp.so and runs its `timing` command on the
Arrow-shaped case: N items (default 64 and 512) of 400 000 bytes of the bench's text (bench.gen_text) each, as a frame
of linked 64 KiB blocks without a content size -- what Arrow IPC writes -- and as a frame of independent blocks.  The
frames are assembled here from liblz4's own blocks (ctypes: LZ4_compress_fast_continue for the linked ones,
LZ4_compress_default for the others), every item at an address of its own.  HIP events around each way, the two
alternating inside every repetition, 2 warm-up and R timed repetitions (default 10), medians.  The loop is the code
of the parent commit, untouched by the batch; `ratio` is loop / batch.  DESIGN.md section 25 and
profiles/r15_lz4_frames.txt are where a run on an MI355X is recorded."""
import argparse
import ctypes
import ctypes.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIB = os.path.join(ROOT, "hipcomp-core_amd", "lib")

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, nargs="+", default=[64, 512])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--bytes", type=int, default=400000)
a = ap.parse_args()

import bench  # noqa: E402
import lz4_framegen as G  # noqa: E402

L = ctypes.CDLL(ctypes.util.find_library("lz4") or "liblz4.so.1")
L.LZ4_createStream.restype = ctypes.c_void_p
L.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
L.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
L.LZ4_freeStream.argtypes = [ctypes.c_void_p]


def frame_of(data: bytes, linked: bool) -> bytes:
    """64 KiB blocks, no content size, no checksums; a block that does not shrink is stored"""
    src = ctypes.create_string_buffer(data, len(data))   # (one buffer: the stream's history is the bytes in front)
    stream = L.LZ4_createStream() if linked else None
    blocks = []
    for at in range(0, len(data), 65536):
        n = min(65536, len(data) - at)
        dst = ctypes.create_string_buffer(n + n // 255 + 16)
        chunk = ctypes.cast(ctypes.addressof(src) + at, ctypes.c_char_p)
        got = L.LZ4_compress_fast_continue(stream, chunk, dst, n, len(dst), 1) if linked else L.LZ4_compress_default(chunk, dst, n, len(dst))
        blocks.append((data[at:at + n], True) if got <= 0 or got >= n else (dst.raw[:got], False))
    if linked:
        L.LZ4_freeStream(stream)
    return G.frame(blocks, 4, linked)


tmp = tempfile.mkdtemp(prefix="quick_lz4_frames")
exe = os.path.join(tmp, "lz4_frames_driver")
subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                os.path.join(ROOT, "tests", "lz4_frames_driver.cpp"), "-L", LIB, "-lhipcomp", "-Wl,-rpath," + LIB, "-o", exe],
               check=True, timeout=600)
text = bench.gen_text(a.bytes).tobytes()
for kind in ("linked", "independent"):
    frame = frame_of(text, kind == "linked")
    assert G.decode(frame) == text, "the frame assembled here does not decode to the text"
    path = os.path.join(tmp, kind + ".lz4")
    with open(path, "wb") as f:
        f.write(frame)
    for items in a.items:
        r = subprocess.run([exe, "timing", str(items), kind, str(a.reps), path], capture_output=True, text=True, timeout=1200)
        if r.returncode != 0:
            sys.exit("driver failed: %s %d\n%s" % (kind, items, r.stderr[-2000:]))
        print(r.stdout.strip())
