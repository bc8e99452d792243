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
from typing import NamedTuple, Optional

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
_P, _SIZE_OUT = c_void_p, POINTER(c_size_t)


def _compress_sigs(codec: str, opts):
    return {
        f"hipcompBatched{codec}CompressGetTempSize": [c_size_t, c_size_t, opts, _SIZE_OUT],
        f"hipcompBatched{codec}CompressGetMaxOutputChunkSize": [c_size_t, opts, _SIZE_OUT],
        f"hipcompBatched{codec}CompressAsync": [_P, _P, c_size_t, c_size_t, _P, c_size_t, _P, _P, opts, _P],
    }


def _decompress_sigs(codec: str):
    return {
        f"hipcompBatched{codec}DecompressGetTempSize": [c_size_t, c_size_t, _SIZE_OUT],
        f"hipcompBatched{codec}DecompressAsync": [_P, _P, _P, _P, c_size_t, _P, c_size_t, _P, _P, _P],
        f"hipcompBatched{codec}GetDecompressSizeAsync": [_P, _P, _P, c_size_t, _P],
    }


def _sigs(codec: str):
    return {**_compress_sigs(codec, _OPTS[codec]), **_decompress_sigs(codec)}


ABI_SYMBOLS = tuple(name for codec in _OPTS for name in _sigs(codec))


def _load(path: str, how: str):
    """The one place that loads a shared object (after torch, as above).  RTLD_LOCAL: several libraries with
    the same symbol names can coexist."""
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: {how} There is no fallback path.")
    return ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)


def _build_hint(subdir: str = "", note: str = "") -> str:
    return ("build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C hipcomp-core_amd/csrc{subdir}`{note}).")


def _bind(obj, dll, sigs):
    for name, argtypes in sigs.items():
        fn = getattr(dll, name)  # AttributeError if not exported
        fn.argtypes = argtypes
        fn.restype = c_int
        setattr(obj, name, fn)


def _size_query(lib, name: str, *args) -> int:
    """Call ``lib.<name>(*args, &out)``, a ...Get...Size function whose last parameter is a size_t*."""
    out = c_size_t(0)
    st = getattr(lib, name)(*args, ctypes.byref(out))
    if st != 0:
        raise RuntimeError(f"{name} -> status {st}")
    return out.value


class HipcompLibrary:
    """A loaded shared object exporting the batched codec C ABI."""

    def __init__(self, path: str = DEFAULT_LIB, codecs=("LZ4", "Snappy", "Cascaded")):
        self._dll = _load(path, _build_hint())
        self.path = path
        self.codecs = tuple(codecs)
        for codec in self.codecs:
            _bind(self, self._dll, _sigs(codec))

    # -- size queries as plain Python -----------------------------------
    def compress_temp_size(self, codec: str, batch: int, max_chunk: int, opts) -> int:
        return _size_query(self, f"hipcompBatched{codec}CompressGetTempSize", batch, max_chunk, opts)

    def max_output_chunk_size(self, codec: str, max_chunk: int, opts) -> int:
        return _size_query(self, f"hipcompBatched{codec}CompressGetMaxOutputChunkSize", max_chunk, opts)

    def decompress_temp_size(self, codec: str, num_chunks: int, max_chunk: int) -> int:
        return _size_query(self, f"hipcompBatched{codec}DecompressGetTempSize", num_chunks, max_chunk)

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
        fn = self._dll.hipcompBatchedCascadedSelectOptsGetTempSize
        fn.restype = c_int
        fn.argtypes = [_SIZE_OUT]
        return _size_query(self._dll, "hipcompBatchedCascadedSelectOptsGetTempSize")


def _available_codecs(path: str):
    # During bring-up the library may export a subset of the codecs; bind what
    # is there and let a missing one fail at the call site (AttributeError).
    dll = _load(path, "run __graft_entry__.build() first.")
    return tuple(codec for codec in _OPTS if hasattr(dll, f"hipcompBatched{codec}CompressAsync"))


_default = None
_knobs = None


def default_library() -> HipcompLibrary:
    """The product library, loaded once.  Raises ImportError if not built."""
    global _default
    if _default is None:
        _default = HipcompLibrary(DEFAULT_LIB, codecs=_available_codecs(DEFAULT_LIB))
    return _default


def knobs_library() -> HipcompLibrary:
    """The test / measurement build that reads the launch-shape knobs from the environment."""
    global _knobs
    if _knobs is None:
        _knobs = HipcompLibrary(KNOBS_LIB, codecs=_available_codecs(KNOBS_LIB))
    return _knobs


# Loading at import time makes a missing build fail loudly and early.  (No companion is loaded here.)
default_library()


# -- the companion libraries ------------------------------------------------------------------------------
class Companion(NamedTuple):
    """One companion of libhipcomp.so: lib/<lib>, built by csrc/<csrc_dir>/Makefile, exporting exactly ``sigs``
    (every function returns hipcompStatus_t); ``codec`` is the name inside ``hipcompBatched<codec>...``."""

    lib: str
    csrc_dir: str
    codec: str
    sigs: dict
    build_note: str = ""
    default_opts: object = None

    @property
    def path(self) -> str:
        return os.path.join(_HERE, "lib", self.lib)


# The decode and compress calls have the shape of the main library's (_sigs); what differs is spelled out.
COMPANIONS = {
    "deflate": Companion("libhipcomp_deflate.so", "deflate", "Deflate", _decompress_sigs("Deflate")),
    "deflate_compress": Companion("libhipcomp_deflate_compress.so", "deflate_compress", "Deflate",
                                  _compress_sigs("Deflate", DeflateOpts), default_opts=DEFLATE_DEFAULT_OPTS),
    "gzip": Companion("libhipcomp_gzip.so", "gzip", "Gzip", {
        **_decompress_sigs("Gzip"), **_compress_sigs("Gzip", GzipOpts),
        # the wrapper in front of the stream; the size scan also takes temp space
        "hipcompBatchedGzipDecompressAsync": [_P, _P, _P, _P, c_size_t, _P, c_size_t, _P, _P, c_int, _P],
        "hipcompBatchedGzipGetDecompressSizeAsync": [_P, _P, _P, c_size_t, c_int, _P, c_size_t, _P],
        "hipcompBgzfSplitHost": [c_void_p, c_size_t, _SIZE_OUT, c_size_t, _SIZE_OUT, _SIZE_OUT],
    }, build_note=", after the two Deflate libraries"),
    "zstd": Companion("libhipcomp_zstd.so", "zstd", "Zstd", _decompress_sigs("Zstd")),
    "zstd_compress": Companion("libhipcomp_zstd_compress.so", "zstd_compress", "Zstd",
                               _compress_sigs("Zstd", ZstdOpts), default_opts=ZSTD_DEFAULT_OPTS),
    "zstd_dict": Companion("libhipcomp_zstd_dict.so", "zstd_dict", "ZstdDict", {
        **_decompress_sigs("ZstdDict"),
        # one more array, the chunks' prepared dictionaries: after the sizes, and in front of the stream
        "hipcompBatchedZstdDictGetDecompressSizeAsync": [_P, _P, _P, _P, c_size_t, _P],
        "hipcompBatchedZstdDictDecompressAsync": [_P, _P, _P, _P, c_size_t, _P, c_size_t, _P, _P, _P, _P],
        "hipcompBatchedZstdDictGetPreparedSize": [c_size_t, _SIZE_OUT],
        "hipcompBatchedZstdDictPrepareAsync": [_P, _P, c_size_t, _P, _P, _P, _P],
    }),
    "zstd_dict_compress": Companion("libhipcomp_zstd_dict_compress.so", "zstd_dict_compress", "ZstdDict", {
        # the compress calls of zstd_compress with one more array, the chunks' prepared dictionaries, in front of the
        # opts; the prepare calls in the shape of zstd_dict's
        "hipcompBatchedZstdDictCompressGetTempSize": [c_size_t, c_size_t, ZstdOpts, _SIZE_OUT],
        "hipcompBatchedZstdDictCompressGetMaxOutputChunkSize": [c_size_t, ZstdOpts, _SIZE_OUT],
        "hipcompBatchedZstdDictCompressAsync": [_P, _P, c_size_t, c_size_t, _P, c_size_t, _P, _P, _P, ZstdOpts, _P],
        "hipcompBatchedZstdDictCompressGetPreparedSize": [c_size_t, _SIZE_OUT],
        "hipcompBatchedZstdDictCompressPrepareAsync": [_P, _P, c_size_t, _P, _P, _P, _P],
    }, default_opts=ZSTD_DEFAULT_OPTS),
}
(DEFLATE_LIB, DEFLATE_COMPRESS_LIB, GZIP_LIB, ZSTD_LIB, ZSTD_COMPRESS_LIB, ZSTD_DICT_LIB,
 ZSTD_DICT_COMPRESS_LIB) = (spec.path for spec in COMPANIONS.values())   # in the table's order


class CompanionLibrary:
    """One loaded companion library: the functions of its COMPANIONS entry as attributes (same argument order as
    the header), and its size queries as plain Python -- those of them that the library exports."""

    companion = None   # the COMPANIONS key; the subclasses below name theirs

    def __init__(self, path: Optional[str] = None):
        self.spec = spec = COMPANIONS[self.companion]
        self.path = path = path or spec.path
        self._dll = _load(path, _build_hint("/" + spec.csrc_dir, spec.build_note))
        _bind(self, self._dll, spec.sigs)

    def _opts(self, opts):
        return self.spec.default_opts if opts is None else opts

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        return _size_query(self, f"hipcompBatched{self.spec.codec}DecompressGetTempSize", num_chunks, max_chunk)

    def compress_temp_size(self, batch: int, max_chunk: int, opts=None) -> int:
        return _size_query(self, f"hipcompBatched{self.spec.codec}CompressGetTempSize", batch, max_chunk, self._opts(opts))

    def max_output_chunk_size(self, max_chunk: int, opts=None) -> int:
        return _size_query(self, f"hipcompBatched{self.spec.codec}CompressGetMaxOutputChunkSize", max_chunk, self._opts(opts))


class DeflateLibrary(CompanionLibrary):
    companion = "deflate"


class DeflateCompressLibrary(CompanionLibrary):
    companion = "deflate_compress"


class ZstdLibrary(CompanionLibrary):
    companion = "zstd"


class ZstdCompressLibrary(CompanionLibrary):
    companion = "zstd_compress"


class GzipLibrary(CompanionLibrary):
    """Its compress size queries take the wrapper (WRAPPER_GZIP, _ZLIB or _BGZF) where the others take opts."""

    companion = "gzip"

    def _opts(self, wrapper):
        return GzipOpts(WRAPPER_GZIP if wrapper is None else wrapper)

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


class ZstdDictLibrary(CompanionLibrary):
    companion = "zstd_dict"

    def prepared_size(self, dict_bytes: int) -> int:
        return _size_query(self, "hipcompBatchedZstdDictGetPreparedSize", dict_bytes)


class ZstdDictCompressLibrary(CompanionLibrary):
    companion = "zstd_dict_compress"

    def prepared_size(self, dict_bytes: int) -> int:
        return _size_query(self, "hipcompBatchedZstdDictCompressGetPreparedSize", dict_bytes)


COMPANION_CLASSES = {cls.companion: cls for cls in (DeflateLibrary, DeflateCompressLibrary, GzipLibrary, ZstdLibrary,
                                                     ZstdCompressLibrary, ZstdDictLibrary, ZstdDictCompressLibrary)}
_companions = {}


def companion_library(name: str) -> CompanionLibrary:
    """The companion library ``name`` (a COMPANIONS key), loaded at the first call (after torch, as above) and once."""
    if name not in _companions:
        _companions[name] = COMPANION_CLASSES[name]()
    return _companions[name]


def deflate_library() -> DeflateLibrary:
    return companion_library("deflate")


def deflate_compress_library() -> DeflateCompressLibrary:
    return companion_library("deflate_compress")


def gzip_library() -> GzipLibrary:
    return companion_library("gzip")


def zstd_library() -> ZstdLibrary:
    return companion_library("zstd")


def zstd_compress_library() -> ZstdCompressLibrary:
    return companion_library("zstd_compress")


def zstd_dict_library() -> ZstdDictLibrary:
    return companion_library("zstd_dict")


def zstd_dict_compress_library() -> ZstdDictCompressLibrary:
    return companion_library("zstd_dict_compress")
