"""Writes the LZ4 frame fixtures of this directory with the system's liblz4 (1.9.3 when they were made) and
manifest.json: per file the SHA-256 of the frame and of its content, the content's length and what the frame carries.
The tests read the files and the manifest only; they need no liblz4 for them.

    python tests/golden/lz4_frame/make_fixtures.py
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import datagen  # noqa: E402
import lz4_framegen as G  # noqa: E402

L = ctypes.CDLL("liblz4.so.1")


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


for f in ("LZ4F_compressFrameBound", "LZ4F_compressFrame", "LZ4F_compressBound", "LZ4F_compressBegin", "LZ4F_compressUpdate",
          "LZ4F_flush", "LZ4F_compressEnd", "LZ4F_createCompressionContext"):
    getattr(L, f).restype = ctypes.c_size_t
L.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_compressBound.argtypes = [ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_createCompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
L.LZ4F_freeCompressionContext.argtypes = [ctypes.c_void_p]
L.LZ4F_compressBegin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_compressUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_flush.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_compressEnd.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
L.LZ4F_isError.argtypes = [ctypes.c_size_t]


def prefs(code, linked, bsum, csum, size, level):
    p = Preferences()
    p.frameInfo.blockSizeID = code
    p.frameInfo.blockMode = 0 if linked else 1
    p.frameInfo.contentChecksumFlag = 1 if csum else 0
    p.frameInfo.blockChecksumFlag = 1 if bsum else 0
    p.frameInfo.contentSize = 1 if size else 0   # (LZ4F_compressFrame writes the true size where this is not 0)
    p.compressionLevel = level
    return p


def one_call(data, **kw):
    p = prefs(**kw)
    cap = L.LZ4F_compressFrameBound(len(data), ctypes.byref(p))
    dst = ctypes.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, data, len(data), ctypes.byref(p))
    assert not L.LZ4F_isError(n)
    return dst.raw[:n]


def streamed(pieces, **kw):
    """compressBegin, then per piece compressUpdate + flush: blocks shorter than the block maximum inside the frame"""
    p = prefs(**kw)
    p.frameInfo.contentSize = 0
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(ctx), 100))
    cap = L.LZ4F_compressBound(max(len(x) for x in pieces), ctypes.byref(p)) + 64
    dst = ctypes.create_string_buffer(cap)
    out = b""

    def take(n):
        nonlocal out
        assert not L.LZ4F_isError(n)
        out += dst.raw[:n]
    take(L.LZ4F_compressBegin(ctx, dst, cap, ctypes.byref(p)))
    for x in pieces:
        take(L.LZ4F_compressUpdate(ctx, dst, cap, x, len(x), None))
        take(L.LZ4F_flush(ctx, dst, cap, None))
    take(L.LZ4F_compressEnd(ctx, dst, cap, None))
    L.LZ4F_freeCompressionContext(ctx)
    return out


def cut(data, sizes):
    out, at = [], 0
    for k in range(10 ** 6):
        if at >= len(data):
            return out
        n = sizes[k % len(sizes)]
        out.append(data[at:at + n])
        at += n


def main():
    text = datagen.text_like(11, 200 << 10)[:200 << 10]
    runs = datagen.random_runs_int32(12, 50 << 10).tobytes()
    harness = datagen.harness_like_int32(13, 48 << 10).tobytes()
    noise = datagen.splitmix64(14, 12 << 10).tobytes()[:90000]
    files = {
        "text_64k_independent": (one_call(text, code=4, linked=False, bsum=False, csum=False, size=False, level=0), text),
        "text_64k_linked_csum": (one_call(text, code=4, linked=True, bsum=False, csum=True, size=False, level=0), text),
        "text_256k_linked_hc_bsum": (one_call(text, code=5, linked=True, bsum=True, csum=False, size=False, level=9), text),
        "runs_1m_independent_size": (one_call(runs, code=6, linked=False, bsum=False, csum=False, size=True, level=0), runs),
        "harness_4m_linked_all": (one_call(harness, code=7, linked=True, bsum=True, csum=True, size=True, level=0), harness),
        "text_64k_independent_hc_all": (one_call(text[:150000], code=4, linked=False, bsum=True, csum=True, size=True, level=9),
                                        text[:150000]),
        "noise_64k_stored": (one_call(noise, code=4, linked=False, bsum=True, csum=False, size=True, level=0), noise),
        "noise_64k_linked_stored": (one_call(noise[:70000] + text[:30000], code=4, linked=True, bsum=False, csum=True, size=False,
                                             level=0), noise[:70000] + text[:30000]),
        "flushed_linked": (streamed(cut(text[:120000], (1000, 30000, 7, 65536, 3, 9000)), code=4, linked=True, bsum=False,
                                    csum=True, size=False, level=0), text[:120000]),
        "flushed_independent": (streamed(cut(runs[:150000], (5, 70000, 1, 20000)), code=5, linked=False, bsum=True, csum=False,
                                         size=False, level=0), runs[:150000]),
        "empty": (one_call(b"", code=4, linked=True, bsum=False, csum=True, size=False, level=0), b""),
    }
    a = one_call(text[:50000], code=4, linked=True, bsum=False, csum=False, size=True, level=0)
    b = one_call(runs[:50000], code=4, linked=False, bsum=False, csum=True, size=False, level=0)
    files["two_frames_skippable"] = (a + G.skippable(b"between the frames", 7) + b, text[:50000] + runs[:50000])
    manifest = {"liblz4": L.LZ4_versionNumber()}
    for name, (frame, content) in sorted(files.items()):
        assert len(frame) < 126 * 1000, (name, len(frame))
        frames = G.parse(frame)
        assert G.decode(frame) == content, name
        with open(os.path.join(HERE, name + ".lz4"), "wb") as f:
            f.write(frame)
        manifest[name] = {
            "frame_sha256": hashlib.sha256(frame).hexdigest(), "frame_bytes": len(frame),
            "content_sha256": hashlib.sha256(content).hexdigest(), "content_bytes": len(content),
            "blocks": sum(len(f["blocks"]) for f in frames),
            "linked": [f["linked"] for f in frames], "stored_blocks": sum(s for f in frames for _, s, _ in f["blocks"]),
            "all_declare_size": all(f["content_size"] is not None for f in frames),
            "bare": any(not f["block_sums"] and not f["content_sum"] for f in frames),
        }
        print(name, len(frame), manifest[name]["blocks"], manifest[name]["stored_blocks"])
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
