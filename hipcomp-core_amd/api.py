"""ctypes binding of the batched codec C ABI (include/hipcomp/*.h).

One :class:`HipcompLibrary` wraps one shared object that exports the 18
``hipcompBatched*`` symbols -- the product ``lib/libhipcomp.so`` by default.
The same class can bind any other library with that ABI (the tests bind the
reference build ``oracle/_ref/libhipcomp_ref.so`` this way to compare bytes on
the GPU); the product never does.

Method names, argument order and meaning are the C functions' (reference
include/hipcomp/lz4.h:106-243, snappy.h:80-195, cascaded.h:142-295).  Device
pointers are passed as plain integers (``tensor.data_ptr()``), streams as the
raw ``hipStream_t`` handle (``torch.cuda.current_stream().cuda_stream``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_int, c_size_t, c_void_p

# torch bundles its own HIP runtime (torch/lib/libamdhip64.so).  It must be in
# the process before libhipcomp.so is loaded so that the library binds to that
# same runtime; otherwise the loader pulls a second copy from /opt/rocm and the
# two runtimes do not share devices or allocations (hipPointerGetAttributes on
# a torch tensor then fails with "no ROCm-capable device").  A C/C++ caller has
# exactly one runtime and needs none of this.
import torch  # noqa: F401  (import order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "libhipcomp.so")
# the same sources built with -DHC_MEASUREMENT_KNOBS (csrc/Makefile VARIANT=knobs): honours
# HIPCOMP_LZ4_SHAPE / HIPCOMP_LZ4_GEOMETRY / HIPCOMP_LZ4_SPAN -- tests and measurement scripts only
KNOBS_LIB = os.path.join(_HERE, "lib", "libhipcomp_knobs.so")
# the batched Deflate decoder (include/hipcomp/deflate.h, csrc/deflate/): a companion library, so that
# libhipcomp.so stays exactly the reference's surface
DEFLATE_LIB = os.path.join(_HERE, "lib", "libhipcomp_deflate.so")
# the batched Deflate encoder (include/hipcomp/deflate_compress.h, csrc/deflate_compress/): a second companion
DEFLATE_COMPRESS_LIB = os.path.join(_HERE, "lib", "libhipcomp_deflate_compress.so")
# gzip / zlib / BGZF members around the Deflate codec (include/hipcomp/gzip.h, csrc/gzip/): a third companion, which
# links the two Deflate libraries (found next to it through its run path)
GZIP_LIB = os.path.join(_HERE, "lib", "libhipcomp_gzip.so")
# the batched Zstandard decoder (include/hipcomp/zstd.h, csrc/zstd/): a fourth companion, on its own
ZSTD_LIB = os.path.join(_HERE, "lib", "libhipcomp_zstd.so")
# the batched Zstandard encoder (include/hipcomp/zstd_compress.h, csrc/zstd_compress/): a fifth companion, on its own
ZSTD_COMPRESS_LIB = os.path.join(_HERE, "lib", "libhipcomp_zstd_compress.so")
# the batched Zstandard decoder for frames that use dictionaries (include/hipcomp/zstd_dict.h, csrc/zstd_dict/): a sixth
ZSTD_DICT_LIB = os.path.join(_HERE, "lib", "libhipcomp_zstd_dict.so")


class hipcompStatus:
    """include/hipcomp/shared_types.h"""

    Success = 0
    ErrorInvalidValue = 10
    ErrorNotSupported = 11
    ErrorCannotDecompress = 12
    ErrorBadChecksum = 13
    ErrorCannotVerifyChecksums = 14
    ErrorCudaError = 1000
    ErrorInternal = 10000


class hipcompType:
    """include/hipcomp.h"""

    CHAR = 0
    UCHAR = 1
    SHORT = 2
    USHORT = 3
    INT = 4
    UINT = 5
    LONGLONG = 6
    ULONGLONG = 7
    BITS = 0xFF

    _SIZES = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 8, 7: 8, 0xFF: 1}

    @classmethod
    def size_of(cls, t: int) -> int:
        return cls._SIZES[t]


class LZ4Opts(ctypes.Structure):
    _fields_ = [("data_type", c_int)]


class SnappyOpts(ctypes.Structure):
    _fields_ = [("reserved", c_int)]


class CascadedOpts(ctypes.Structure):
    _fields_ = [
        ("chunk_size", c_size_t),
        ("type", c_int),
        ("num_RLEs", c_int),
        ("num_deltas", c_int),
        ("use_bp", c_int),
    ]


class DeflateOpts(ctypes.Structure):
    _fields_ = [("algo", c_int)]


class GzipOpts(ctypes.Structure):
    _fields_ = [("wrapper", c_int)]


class ZstdOpts(ctypes.Structure):
    _fields_ = [("level", c_int), ("checksum", c_int)]


WRAPPER_GZIP, WRAPPER_ZLIB, WRAPPER_BGZF = 0, 1, 2
WRAPPERS = {"gzip": WRAPPER_GZIP, "zlib": WRAPPER_ZLIB, "bgzf": WRAPPER_BGZF}
BGZF_MAX_CHUNK_BYTES = 65280
BGZF_EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

LZ4_DEFAULT_OPTS = LZ4Opts(hipcompType.CHAR)
DEFLATE_DEFAULT_OPTS = DeflateOpts(0)
ZSTD_DEFAULT_OPTS = ZstdOpts(0, 0)
DEFLATE_COMPRESS_MAX_CHUNK_BYTES = 65536
SNAPPY_DEFAULT_OPTS = SnappyOpts(0)
CASCADED_DEFAULT_OPTS = CascadedOpts(4096, hipcompType.INT, 2, 1, 1)

_OPTS = {"LZ4": LZ4Opts, "Snappy": SnappyOpts, "Cascaded": CascadedOpts}


def _sigs(codec: str):
    opts = _OPTS[codec]
    p = c_void_p
    return {
        f"hipcompBatched{codec}CompressGetTempSize": [c_size_t, c_size_t, opts, POINTER(c_size_t)],
        f"hipcompBatched{codec}CompressGetMaxOutputChunkSize": [c_size_t, opts, POINTER(c_size_t)],
        f"hipcompBatched{codec}CompressAsync": [p, p, c_size_t, c_size_t, p, c_size_t, p, p, opts, p],
        f"hipcompBatched{codec}DecompressGetTempSize": [c_size_t, c_size_t, POINTER(c_size_t)],
        f"hipcompBatched{codec}DecompressAsync": [p, p, p, p, c_size_t, p, c_size_t, p, p, p],
        f"hipcompBatched{codec}GetDecompressSizeAsync": [p, p, p, c_size_t, p],
    }


ABI_SYMBOLS = tuple(name for codec in _OPTS for name in _sigs(codec))


class HipcompLibrary:
    """A loaded shared object exporting the batched codec C ABI."""

    def __init__(self, path: str = DEFAULT_LIB, codecs=("LZ4", "Snappy", "Cascaded")):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc`). There is no fallback path."
            )
        self.path = path
        # RTLD_LOCAL: several libraries with the same symbol names can coexist
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        self.codecs = tuple(codecs)
        for codec in self.codecs:
            for name, argtypes in _sigs(codec).items():
                fn = getattr(self._dll, name)  # AttributeError if not exported
                fn.argtypes = argtypes
                fn.restype = c_int
                setattr(self, name, fn)

    # -- size queries as plain Python -----------------------------------
    def compress_temp_size(self, codec: str, batch: int, max_chunk: int, opts) -> int:
        out = c_size_t(0)
        st = getattr(self, f"hipcompBatched{codec}CompressGetTempSize")(batch, max_chunk, opts, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatched{codec}CompressGetTempSize -> status {st}")
        return out.value

    def max_output_chunk_size(self, codec: str, max_chunk: int, opts) -> int:
        out = c_size_t(0)
        st = getattr(self, f"hipcompBatched{codec}CompressGetMaxOutputChunkSize")(max_chunk, opts, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatched{codec}CompressGetMaxOutputChunkSize -> status {st}")
        return out.value

    def cascaded_select_opts(self, ptrs: int, sizes: int, batch: int, type_tag: int, temp: int, temp_bytes: int, stream: int = 0):
        """hipcompBatchedCascadedSelectOpts (include/hipcomp/cascaded_select.h, an API of this library's own):
        -> (CascadedOpts, estimated ratio).  Synchronises the stream."""
        fn = self._dll.hipcompBatchedCascadedSelectOpts
        fn.restype = c_int
        fn.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_size_t, POINTER(CascadedOpts), POINTER(ctypes.c_double), c_void_p]
        opts, ratio = CascadedOpts(), ctypes.c_double(0.0)
        st = fn(ptrs, sizes, batch, type_tag, temp, temp_bytes, ctypes.byref(opts), ctypes.byref(ratio), stream)
        if st != 0:
            raise RuntimeError(f"hipcompBatchedCascadedSelectOpts -> status {st}")
        return opts, ratio.value

    def cascaded_select_temp_size(self) -> int:
        out = c_size_t(0)
        fn = self._dll.hipcompBatchedCascadedSelectOptsGetTempSize
        fn.restype = c_int
        fn.argtypes = [POINTER(c_size_t)]
        assert fn(ctypes.byref(out)) == 0
        return out.value

    def decompress_temp_size(self, codec: str, num_chunks: int, max_chunk: int) -> int:
        out = c_size_t(0)
        st = getattr(self, f"hipcompBatched{codec}DecompressGetTempSize")(num_chunks, max_chunk, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatched{codec}DecompressGetTempSize -> status {st}")
        return out.value


_default = None


_knobs = None


def knobs_library() -> HipcompLibrary:
    """The test / measurement build that reads the launch-shape knobs from the environment."""
    global _knobs
    if _knobs is None:
        _knobs = HipcompLibrary(KNOBS_LIB, codecs=_available_codecs(KNOBS_LIB))
    return _knobs


class DeflateLibrary:
    """lib/libhipcomp_deflate.so: the three functions of include/hipcomp/deflate.h, bound like the decode
    calls of :class:`HipcompLibrary` (same argument order)."""

    def __init__(self, path: str = DEFLATE_LIB):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc/deflate`). There is no fallback path."
            )
        self.path = path
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        p = c_void_p
        for name, argtypes in (
            ("hipcompBatchedDeflateDecompressGetTempSize", [c_size_t, c_size_t, POINTER(c_size_t)]),
            ("hipcompBatchedDeflateDecompressAsync", [p, p, p, p, c_size_t, p, c_size_t, p, p, p]),
            ("hipcompBatchedDeflateGetDecompressSizeAsync", [p, p, p, c_size_t, p]),
        ):
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = c_int
            setattr(self, name, fn)

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedDeflateDecompressGetTempSize(num_chunks, max_chunk, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedDeflateDecompressGetTempSize -> status {st}")
        return out.value


_deflate = None


def deflate_library() -> DeflateLibrary:
    """The Deflate companion library, loaded at the first call (after torch, as above) and once."""
    global _deflate
    if _deflate is None:
        _deflate = DeflateLibrary(DEFLATE_LIB)
    return _deflate


class DeflateCompressLibrary:
    """lib/libhipcomp_deflate_compress.so: the three functions of include/hipcomp/deflate_compress.h, bound
    like the compress calls of :class:`HipcompLibrary` (same argument order)."""

    def __init__(self, path: str = DEFLATE_COMPRESS_LIB):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc/deflate_compress`). There is no fallback path."
            )
        self.path = path
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        p = c_void_p
        for name, argtypes in (
            ("hipcompBatchedDeflateCompressGetTempSize", [c_size_t, c_size_t, DeflateOpts, POINTER(c_size_t)]),
            ("hipcompBatchedDeflateCompressGetMaxOutputChunkSize", [c_size_t, DeflateOpts, POINTER(c_size_t)]),
            ("hipcompBatchedDeflateCompressAsync", [p, p, c_size_t, c_size_t, p, c_size_t, p, p, DeflateOpts, p]),
        ):
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = c_int
            setattr(self, name, fn)

    def compress_temp_size(self, batch: int, max_chunk: int, opts=DEFLATE_DEFAULT_OPTS) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedDeflateCompressGetTempSize(batch, max_chunk, opts, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedDeflateCompressGetTempSize -> status {st}")
        return out.value

    def max_output_chunk_size(self, max_chunk: int, opts=DEFLATE_DEFAULT_OPTS) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedDeflateCompressGetMaxOutputChunkSize(max_chunk, opts, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedDeflateCompressGetMaxOutputChunkSize -> status {st}")
        return out.value


_deflate_compress = None


def deflate_compress_library() -> DeflateCompressLibrary:
    """The Deflate encoder's library, loaded at the first call (after torch, as above) and once."""
    global _deflate_compress
    if _deflate_compress is None:
        _deflate_compress = DeflateCompressLibrary(DEFLATE_COMPRESS_LIB)
    return _deflate_compress


class GzipLibrary:
    """lib/libhipcomp_gzip.so: the seven functions of include/hipcomp/gzip.h (same argument order)."""

    def __init__(self, path: str = GZIP_LIB):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc/gzip`, after the two Deflate libraries). There is no fallback path."
            )
        self.path = path
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        p = c_void_p
        for name, argtypes in (
            ("hipcompBatchedGzipDecompressGetTempSize", [c_size_t, c_size_t, POINTER(c_size_t)]),
            ("hipcompBatchedGzipGetDecompressSizeAsync", [p, p, p, c_size_t, c_int, p, c_size_t, p]),
            ("hipcompBatchedGzipDecompressAsync", [p, p, p, p, c_size_t, p, c_size_t, p, p, c_int, p]),
            ("hipcompBatchedGzipCompressGetTempSize", [c_size_t, c_size_t, GzipOpts, POINTER(c_size_t)]),
            ("hipcompBatchedGzipCompressGetMaxOutputChunkSize", [c_size_t, GzipOpts, POINTER(c_size_t)]),
            ("hipcompBatchedGzipCompressAsync", [p, p, c_size_t, c_size_t, p, c_size_t, p, p, GzipOpts, p]),
            ("hipcompBgzfSplitHost", [c_void_p, c_size_t, POINTER(c_size_t), c_size_t, POINTER(c_size_t), POINTER(c_size_t)]),
        ):
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = c_int
            setattr(self, name, fn)

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedGzipDecompressGetTempSize(num_chunks, max_chunk, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedGzipDecompressGetTempSize -> status {st}")
        return out.value

    def compress_temp_size(self, batch: int, max_chunk: int, wrapper: int = WRAPPER_GZIP) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedGzipCompressGetTempSize(batch, max_chunk, GzipOpts(wrapper), ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedGzipCompressGetTempSize -> status {st}")
        return out.value

    def max_output_chunk_size(self, max_chunk: int, wrapper: int = WRAPPER_GZIP) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedGzipCompressGetMaxOutputChunkSize(max_chunk, GzipOpts(wrapper), ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedGzipCompressGetMaxOutputChunkSize -> status {st}")
        return out.value

    def bgzf_split(self, data: bytes, capacity=None):
        """hipcompBgzfSplitHost on a BGZF file in host memory: -> (block offsets, where the walk stopped);
        the file was whole exactly when that is len(data).  Block i is data[offsets[i]:offsets[i + 1]], the last
        one ends where the walk stopped."""
        if capacity is None:
            capacity = len(data) // 28 + 1   # no BGZF block is shorter than the empty one
        offsets = (c_size_t * max(capacity, 1))()
        count, stopped = c_size_t(0), c_size_t(0)
        st = self.hipcompBgzfSplitHost(ctypes.c_char_p(data), len(data), offsets, capacity,
                                       ctypes.byref(count), ctypes.byref(stopped))
        if st != 0:
            raise RuntimeError(f"hipcompBgzfSplitHost -> status {st}")
        return list(offsets[:count.value]), stopped.value


_gzip = None


def gzip_library() -> GzipLibrary:
    """The gzip companion library, loaded at the first call (after torch, as above) and once."""
    global _gzip
    if _gzip is None:
        _gzip = GzipLibrary(GZIP_LIB)
    return _gzip


def default_library() -> HipcompLibrary:
    """The product library, loaded once.  Raises ImportError if not built."""
    global _default
    if _default is None:
        _default = HipcompLibrary(DEFAULT_LIB, codecs=_available_codecs(DEFAULT_LIB))
    return _default


def _available_codecs(path: str):
    # During bring-up the library may export a subset of the codecs; bind what
    # is there and let a missing one fail at the call site (AttributeError).
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: run __graft_entry__.build() first. There is no fallback path."
        )
    dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    out = []
    for codec in _OPTS:
        try:
            getattr(dll, f"hipcompBatched{codec}CompressAsync")
            out.append(codec)
        except AttributeError:
            pass
    return tuple(out)


# Loading at import time makes a missing build fail loudly and early.
default_library()


class ZstdLibrary:
    """lib/libhipcomp_zstd.so: the three functions of include/hipcomp/zstd.h, bound like :class:`DeflateLibrary`
    (same argument order)."""

    def __init__(self, path: str = ZSTD_LIB):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc/zstd`). There is no fallback path."
            )
        self.path = path
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        p = c_void_p
        for name, argtypes in (
            ("hipcompBatchedZstdDecompressGetTempSize", [c_size_t, c_size_t, POINTER(c_size_t)]),
            ("hipcompBatchedZstdDecompressAsync", [p, p, p, p, c_size_t, p, c_size_t, p, p, p]),
            ("hipcompBatchedZstdGetDecompressSizeAsync", [p, p, p, c_size_t, p]),
        ):
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = c_int
            setattr(self, name, fn)

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedZstdDecompressGetTempSize(num_chunks, max_chunk, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedZstdDecompressGetTempSize -> status {st}")
        return out.value


_zstd = None


def zstd_library() -> ZstdLibrary:
    """The Zstandard companion library, loaded at the first call (after torch, as above) and once."""
    global _zstd
    if _zstd is None:
        _zstd = ZstdLibrary(ZSTD_LIB)
    return _zstd


class ZstdDictLibrary:
    """lib/libhipcomp_zstd_dict.so: the five functions of include/hipcomp/zstd_dict.h, bound like
    :class:`ZstdLibrary` (the decode calls take one more array, the chunks' prepared dictionaries)."""

    def __init__(self, path: str = ZSTD_DICT_LIB):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc/zstd_dict`). There is no fallback path."
            )
        self.path = path
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        p = c_void_p
        for name, argtypes in (
            ("hipcompBatchedZstdDictGetPreparedSize", [c_size_t, POINTER(c_size_t)]),
            ("hipcompBatchedZstdDictPrepareAsync", [p, p, c_size_t, p, p, p, p]),
            ("hipcompBatchedZstdDictDecompressGetTempSize", [c_size_t, c_size_t, POINTER(c_size_t)]),
            ("hipcompBatchedZstdDictGetDecompressSizeAsync", [p, p, p, p, c_size_t, p]),
            ("hipcompBatchedZstdDictDecompressAsync", [p, p, p, p, c_size_t, p, c_size_t, p, p, p, p]),
        ):
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = c_int
            setattr(self, name, fn)

    def prepared_size(self, dict_bytes: int) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedZstdDictGetPreparedSize(dict_bytes, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedZstdDictGetPreparedSize -> status {st}")
        return out.value

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedZstdDictDecompressGetTempSize(num_chunks, max_chunk, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedZstdDictDecompressGetTempSize -> status {st}")
        return out.value


_zstd_dict = None


def zstd_dict_library() -> ZstdDictLibrary:
    """The Zstandard dictionary companion library, loaded at the first call (after torch, as above) and once."""
    global _zstd_dict
    if _zstd_dict is None:
        _zstd_dict = ZstdDictLibrary(ZSTD_DICT_LIB)
    return _zstd_dict


class ZstdCompressLibrary:
    """lib/libhipcomp_zstd_compress.so: the three functions of include/hipcomp/zstd_compress.h, bound like
    :class:`DeflateCompressLibrary` (same argument order)."""

    def __init__(self, path: str = ZSTD_COMPRESS_LIB):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C hipcomp-core_amd/csrc/zstd_compress`). There is no fallback path."
            )
        self.path = path
        self._dll = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        p = c_void_p
        for name, argtypes in (
            ("hipcompBatchedZstdCompressGetTempSize", [c_size_t, c_size_t, ZstdOpts, POINTER(c_size_t)]),
            ("hipcompBatchedZstdCompressGetMaxOutputChunkSize", [c_size_t, ZstdOpts, POINTER(c_size_t)]),
            ("hipcompBatchedZstdCompressAsync", [p, p, c_size_t, c_size_t, p, c_size_t, p, p, ZstdOpts, p]),
        ):
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = c_int
            setattr(self, name, fn)

    def compress_temp_size(self, batch: int, max_chunk: int, opts=ZSTD_DEFAULT_OPTS) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedZstdCompressGetTempSize(batch, max_chunk, opts, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedZstdCompressGetTempSize -> status {st}")
        return out.value

    def max_output_chunk_size(self, max_chunk: int, opts=ZSTD_DEFAULT_OPTS) -> int:
        out = c_size_t(0)
        st = self.hipcompBatchedZstdCompressGetMaxOutputChunkSize(max_chunk, opts, ctypes.byref(out))
        if st != 0:
            raise RuntimeError(f"hipcompBatchedZstdCompressGetMaxOutputChunkSize -> status {st}")
        return out.value


_zstd_compress = None


def zstd_compress_library() -> ZstdCompressLibrary:
    """The Zstandard encoder's library, loaded at the first call (after torch, as above) and once."""
    global _zstd_compress
    if _zstd_compress is None:
        _zstd_compress = ZstdCompressLibrary(ZSTD_COMPRESS_LIB)
    return _zstd_compress
