"""Chunk lists in HBM and thin call helpers over the C ABI.

Plumbing only (device memory and streams come from torch); every codec
operation below is one call into ``libhipcomp.so``.  Layout: a batch of chunks
is ONE contiguous ``uint8`` device buffer with a fixed stride per chunk plus
two device arrays the C ABI consumes directly -- chunk addresses (``void*[]``)
and chunk sizes (``size_t[]``), both built on the device so no host transfer
sits inside a timed region.  The stride is a multiple of 16 bytes so every
chunk starts 16-byte aligned (Cascaded requires element alignment; LZ4 typed
modes require ``sizeof(T)`` alignment).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import api
from .api import HipcompLibrary, default_library


def _stream_handle(stream=None) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass
class ChunkBatch:
    """``n`` chunks at ``data[i*stride : i*stride + sizes[i]]`` on one device."""

    data: torch.Tensor   # uint8 [n * stride] (device)
    ptrs: torch.Tensor   # int64 [n] device addresses (void*[])
    sizes: torch.Tensor  # int64 [n] bytes (size_t[])
    stride: int

    @property
    def n(self) -> int:
        return int(self.ptrs.numel())

    @property
    def device(self):
        return self.data.device

    def chunk_bytes(self, i: int, size: Optional[int] = None) -> bytes:
        """Host copy of chunk ``i`` (test helper)."""
        if size is None:
            size = int(self.sizes[i].item())
        return self.data[i * self.stride : i * self.stride + size].cpu().numpy().tobytes()

    def to_host_chunks(self):
        sizes = self.sizes.cpu().numpy()
        host = self.data.cpu().numpy()
        return [host[i * self.stride : i * self.stride + int(sizes[i])].tobytes() for i in range(self.n)]


def make_ptrs(data: torch.Tensor, n: int, stride: int) -> torch.Tensor:
    base = data.data_ptr()
    return base + torch.arange(n, device=data.device, dtype=torch.int64) * stride


def alloc_batch(n: int, stride: int, device="cuda", fill: Optional[int] = None) -> ChunkBatch:
    stride = _round_up(max(stride, 1), 16)
    if fill is None:
        data = torch.empty(max(n * stride, 16), dtype=torch.uint8, device=device)
    else:
        data = torch.full((max(n * stride, 16),), fill, dtype=torch.uint8, device=device)
    return ChunkBatch(data, make_ptrs(data, n, stride), torch.zeros(n, dtype=torch.int64, device=device), stride)


def from_host_chunks(chunks: Sequence[bytes], device="cuda", stride: Optional[int] = None) -> ChunkBatch:
    n = len(chunks)
    mx = max([len(c) for c in chunks], default=0)
    stride = _round_up(max(stride or mx, 1), 16)
    host = np.zeros(max(n * stride, 16), dtype=np.uint8)
    for i, c in enumerate(chunks):
        host[i * stride : i * stride + len(c)] = np.frombuffer(c, dtype=np.uint8)
    data = torch.from_numpy(host).to(device)
    sizes = torch.tensor([len(c) for c in chunks], dtype=torch.int64, device=device)
    return ChunkBatch(data, make_ptrs(data, n, stride), sizes, stride)


def from_device_buffer(data: torch.Tensor, chunk_bytes: int) -> ChunkBatch:
    """View a contiguous uint8 device buffer as equal chunks (last may be short)."""
    assert data.dtype == torch.uint8 and data.is_contiguous()
    assert chunk_bytes % 16 == 0
    total = data.numel()
    n = (total + chunk_bytes - 1) // chunk_bytes
    sizes = torch.full((n,), chunk_bytes, dtype=torch.int64, device=data.device)
    if n and total % chunk_bytes:
        sizes[-1] = total % chunk_bytes
    return ChunkBatch(data, make_ptrs(data, n, chunk_bytes), sizes, chunk_bytes)


def _check(status: int, what: str):
    if status != api.hipcompStatus.Success:
        raise RuntimeError(f"{what} returned hipcompStatus_t {status}")


def _temp(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)


class _Calls:
    """What the wrapper classes below share: ``self.lib`` exports ``hipcompBatched<abi><suffix>``, where abi is
    the class's ``_abi`` or, without one, its ``name``."""

    _abi = None

    def _cname(self, suffix: str, abi: Optional[str] = None) -> str:
        return f"hipcompBatched{abi or self._abi or self.name}{suffix}"

    def _f(self, suffix: str, abi: Optional[str] = None):
        return getattr(self.lib, self._cname(suffix, abi))


class _EncodeCalls(_Calls):
    """The compress half over ``self.lib`` and ``self.opts``: the size queries, the raw call (the caller owns
    every buffer) and compress(), which allocates like a caller of the C API would."""

    _refuses_small_max_chunk = True

    def compress_temp_size(self, batch: int, max_chunk: int) -> int:
        return self.lib.compress_temp_size(batch, max_chunk, self.opts)

    def max_output_chunk_size(self, max_chunk: int) -> int:
        return self.lib.max_output_chunk_size(max_chunk, self.opts)

    def compress_async(self, src: ChunkBatch, max_chunk: int, temp: Optional[torch.Tensor],
                       dst: ChunkBatch, stream=None, *extra) -> int:
        """``extra``: what the class's C call takes in front of the opts."""
        return self._f("CompressAsync")(
            _ptr(src.ptrs), _ptr(src.sizes), max_chunk, src.n,
            _ptr(temp), 0 if temp is None else temp.numel(),
            _ptr(dst.ptrs), _ptr(dst.sizes), *extra, self.opts, _stream_handle(stream))

    def compress(self, src: ChunkBatch, max_chunk: Optional[int] = None, *extra) -> ChunkBatch:
        """``max_chunk`` is the value handed to the C API as max_uncompressed_chunk_bytes (it sizes the temp
        space and the output slots, the bytes do not depend on it); by default the real largest chunk.
        ``extra``: what the class's compress_async takes after ``dst``."""
        real_max = int(src.sizes.max().item()) if src.n else 0
        if max_chunk is None:
            max_chunk = real_max
        if self._refuses_small_max_chunk and max_chunk < real_max:   # (the C call would leave such a chunk uncompressed, with size 0)
            raise ValueError(f"max_chunk {max_chunk} is smaller than the largest chunk of the batch ({real_max} bytes)")
        # (where a small max_chunk is refused, max_chunk >= real_max here and the larger of the two is max_chunk itself)
        dst = alloc_batch(src.n, self.max_output_chunk_size(max(real_max, max_chunk)), src.device)
        temp = _temp(self.compress_temp_size(src.n, max_chunk), src.device)
        _check(self.compress_async(src, max_chunk, temp, dst, *extra), self._cname("CompressAsync"))
        return dst


class _DecodeCalls(_Calls):
    """The decode half over ``self.lib``: the temp size query, the raw calls and the allocating decompress() and
    get_decompress_size().  A class whose C calls take one more argument overrides the method that passes it."""

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        return self.lib.decompress_temp_size(num_chunks, max_chunk)

    def _decompress_call(self, comp, out_caps, actual, temp, dst, statuses, stream, *extra) -> int:
        return self._f("DecompressAsync")(
            _ptr(comp.ptrs), _ptr(comp.sizes), _ptr(out_caps), _ptr(actual), comp.n,
            _ptr(temp), 0 if temp is None else temp.numel(),
            _ptr(dst.ptrs), _ptr(statuses), *extra, _stream_handle(stream))

    def decompress_async(self, comp: ChunkBatch, out_caps: torch.Tensor, actual: Optional[torch.Tensor],
                         temp: Optional[torch.Tensor], dst: ChunkBatch,
                         statuses: Optional[torch.Tensor], stream=None) -> int:
        return self._decompress_call(comp, out_caps, actual, temp, dst, statuses, stream)

    def get_decompress_size_async(self, comp: ChunkBatch, sizes_out: torch.Tensor, stream=None) -> int:
        return self._f("GetDecompressSizeAsync")(
            _ptr(comp.ptrs), _ptr(comp.sizes), _ptr(sizes_out), comp.n, _stream_handle(stream))

    def _decode_temp(self, comp: ChunkBatch, max_chunk: int) -> Optional[torch.Tensor]:
        return _temp(self.decompress_temp_size(comp.n, max_chunk), comp.device)

    def _decompress(self, comp: ChunkBatch, out_capacity: int, *extra, with_status: bool = True):
        """``extra``: what the class's decompress_async takes after ``statuses``."""
        dev = comp.device
        dst = alloc_batch(comp.n, out_capacity, dev)
        caps = torch.full((comp.n,), out_capacity, dtype=torch.int64, device=dev)
        actual = torch.full((comp.n,), -1, dtype=torch.int64, device=dev) if with_status else None
        statuses = torch.full((comp.n,), -1, dtype=torch.int32, device=dev) if with_status else None
        temp = self._decode_temp(comp, out_capacity)
        _check(self.decompress_async(comp, caps, actual, temp, dst, statuses, *extra), self._cname("DecompressAsync"))
        if actual is not None:
            dst.sizes = actual
        return dst, actual, statuses

    def decompress(self, comp: ChunkBatch, out_capacity: int):
        return self._decompress(comp, out_capacity)

    def _get_decompress_size(self, comp: ChunkBatch, call) -> torch.Tensor:
        out = torch.full((comp.n,), -1, dtype=torch.int64, device=comp.device)
        _check(call(out), self._cname("GetDecompressSizeAsync"))
        return out

    def get_decompress_size(self, comp: ChunkBatch) -> torch.Tensor:
        return self._get_decompress_size(comp, lambda out: self.get_decompress_size_async(comp, out))


class _PrepareCalls(_Calls):
    """The prepare half over ``self.lib``: dictionaries become blobs on the device.  The C functions are
    ``hipcompBatched<_prepare_abi>PrepareAsync`` and ``...GetPreparedSize``."""

    _prepare_abi = None

    def prepared_size(self, dict_bytes: int) -> int:
        return api._size_query(self.lib, self._cname("GetPreparedSize", self._prepare_abi), dict_bytes)

    def prepare_async(self, dicts: ChunkBatch, blobs: ChunkBatch, capacities: torch.Tensor, statuses: torch.Tensor,
                      stream=None) -> int:
        return self._f("PrepareAsync", self._prepare_abi)(
            _ptr(dicts.ptrs), _ptr(dicts.sizes), dicts.n, _ptr(blobs.ptrs), _ptr(capacities), _ptr(statuses),
            _stream_handle(stream))

    def prepare(self, dictionaries: Sequence[bytes], device="cuda"):
        """-> (blobs, statuses): blob i at ``blobs.ptrs[i]`` (16-byte aligned, ``blobs.sizes[i]`` bytes), status i
        hipcompSuccess or why dictionary i has no valid blob."""
        dicts = from_host_chunks(dictionaries, device)
        sizes = [self.prepared_size(len(d)) for d in dictionaries]
        blobs = alloc_batch(dicts.n, max(sizes, default=16), device)
        blobs.sizes = torch.tensor(sizes, dtype=torch.int64, device=device)
        statuses = torch.full((dicts.n,), -1, dtype=torch.int32, device=device)
        _check(self.prepare_async(dicts, blobs, blobs.sizes, statuses), self._cname("PrepareAsync", self._prepare_abi))
        return blobs, statuses


class Codec(_EncodeCalls, _DecodeCalls):
    """Calls of one codec ("LZ4", "Snappy" or "Cascaded") on one library."""

    # compress(): ``max_chunk`` may be below the largest chunk (for LZ4 it sizes the hash table and so takes
    # part in the result); the output buffers are sized from the larger of the two
    _refuses_small_max_chunk = False

    def __init__(self, name: str, opts=None, lib: Optional[HipcompLibrary] = None):
        self.name = name
        self.lib = lib or default_library()
        if opts is None:
            opts = {"LZ4": api.LZ4_DEFAULT_OPTS, "Snappy": api.SNAPPY_DEFAULT_OPTS,
                    "Cascaded": api.CASCADED_DEFAULT_OPTS}[name]
        self.opts = opts

    # (the main library's size queries take the codec's name)
    def compress_temp_size(self, batch: int, max_chunk: int) -> int:
        return self.lib.compress_temp_size(self.name, batch, max_chunk, self.opts)

    def max_output_chunk_size(self, max_chunk: int) -> int:
        return self.lib.max_output_chunk_size(self.name, max_chunk, self.opts)

    def decompress_temp_size(self, num_chunks: int, max_chunk: int) -> int:
        return self.lib.decompress_temp_size(self.name, num_chunks, max_chunk)

    def decompress(self, comp: ChunkBatch, out_capacity: int, with_status: bool = True):
        return self._decompress(comp, out_capacity, with_status=with_status)


class DeflateDecoder(_DecodeCalls):
    """The batched Deflate decoder (include/hipcomp/deflate.h, lib/libhipcomp_deflate.so) over ChunkBatch:
    the decode half of :class:`Codec`, chunk i being one raw Deflate stream.  It needs no temp space, and
    decompress() passes none."""

    name = "Deflate"

    def __init__(self, lib=None):
        self.lib = lib or api.deflate_library()

    def _decode_temp(self, comp: ChunkBatch, max_chunk: int) -> None:
        return None


class DeflateEncoder(_EncodeCalls):
    """The batched Deflate encoder (include/hipcomp/deflate_compress.h, lib/libhipcomp_deflate_compress.so)
    over ChunkBatch: the compress half of :class:`Codec`, chunk i becoming one raw Deflate stream.  Chunks hold
    at most 65536 bytes."""

    name = "Deflate"

    def __init__(self, opts=None, lib=None):
        self.lib = lib or api.deflate_compress_library()
        self.opts = api.DEFLATE_DEFAULT_OPTS if opts is None else opts


class GzipCodec(_EncodeCalls, _DecodeCalls):
    """gzip, zlib or BGZF members around the Deflate codec (include/hipcomp/gzip.h, lib/libhipcomp_gzip.so) over
    ChunkBatch, shaped like :class:`DeflateEncoder` and :class:`DeflateDecoder`: chunk i becomes, or is, one member
    with its header and its verified CRC-32 / Adler-32 trailer.  Chunks to compress hold at most 65536 bytes
    (BGZF: 65280).  The decode calls take the wrapper, and the size scan takes temp space too."""

    _abi = "Gzip"

    def __init__(self, wrapper: str = "gzip", lib=None):
        if wrapper not in api.WRAPPERS:
            raise ValueError(f"wrapper must be one of {sorted(api.WRAPPERS)}, not {wrapper!r}")
        self.name = wrapper
        self.wrapper = api.WRAPPERS[wrapper]
        self.opts = api.GzipOpts(self.wrapper)
        self.lib = lib or api.gzip_library()

    # (the library's compress size queries take the wrapper, not the struct)
    def compress_temp_size(self, batch: int, max_chunk: int) -> int:
        return self.lib.compress_temp_size(batch, max_chunk, self.wrapper)

    def max_output_chunk_size(self, max_chunk: int) -> int:
        return self.lib.max_output_chunk_size(max_chunk, self.wrapper)

    def decompress_async(self, comp: ChunkBatch, out_caps: torch.Tensor, actual: Optional[torch.Tensor],
                         temp: Optional[torch.Tensor], dst: ChunkBatch,
                         statuses: Optional[torch.Tensor], stream=None) -> int:
        return self._decompress_call(comp, out_caps, actual, temp, dst, statuses, stream, self.wrapper)

    def get_decompress_size_async(self, comp: ChunkBatch, sizes_out: torch.Tensor, temp: Optional[torch.Tensor],
                                  stream=None) -> int:
        return self._f("GetDecompressSizeAsync")(
            _ptr(comp.ptrs), _ptr(comp.sizes), _ptr(sizes_out), comp.n, self.wrapper,
            _ptr(temp), 0 if temp is None else temp.numel(), _stream_handle(stream))

    def get_decompress_size(self, comp: ChunkBatch) -> torch.Tensor:
        temp = self._decode_temp(comp, 0)
        return self._get_decompress_size(comp, lambda out: self.get_decompress_size_async(comp, out, temp))


class ZstdDecoder(_DecodeCalls):
    """The batched Zstandard decoder (include/hipcomp/zstd.h, lib/libhipcomp_zstd.so) over ChunkBatch, shaped
    like :class:`DeflateDecoder`: chunk i is zero or more concatenated frames.  Unlike Deflate the decoder needs
    temp space; decompress() allocates what the library asks for."""

    name = "Zstd"

    def __init__(self, lib=None):
        self.lib = lib or api.zstd_library()


class ZstdDictDecoder(_DecodeCalls, _PrepareCalls):
    """The batched Zstandard decoder for frames that use dictionaries (include/hipcomp/zstd_dict.h,
    lib/libhipcomp_zstd_dict.so) over ChunkBatch, shaped like :class:`ZstdDecoder`.  prepare() digests
    dictionaries into blobs on the device; the decode calls take ``prepared``, an int64 tensor with the address
    of every chunk's blob (0: no dictionary)."""

    name = _prepare_abi = "ZstdDict"

    def __init__(self, lib=None):
        self.lib = lib or api.zstd_dict_library()

    def decompress_async(self, comp: ChunkBatch, out_caps: torch.Tensor, actual: Optional[torch.Tensor],
                         temp: Optional[torch.Tensor], dst: ChunkBatch, statuses: Optional[torch.Tensor],
                         prepared: torch.Tensor, stream=None) -> int:
        return self._decompress_call(comp, out_caps, actual, temp, dst, statuses, stream, _ptr(prepared))

    def get_decompress_size_async(self, comp: ChunkBatch, prepared: torch.Tensor, sizes_out: torch.Tensor, stream=None) -> int:
        return self.lib.hipcompBatchedZstdDictGetDecompressSizeAsync(
            _ptr(comp.ptrs), _ptr(comp.sizes), _ptr(prepared), _ptr(sizes_out), comp.n, _stream_handle(stream))

    def decompress(self, comp: ChunkBatch, out_capacity: int, prepared: torch.Tensor):
        return self._decompress(comp, out_capacity, prepared)

    def get_decompress_size(self, comp: ChunkBatch, prepared: torch.Tensor) -> torch.Tensor:
        return self._get_decompress_size(comp, lambda out: self.get_decompress_size_async(comp, prepared, out))


class ZstdEncoder(_EncodeCalls):
    """The batched Zstandard encoder (include/hipcomp/zstd_compress.h, lib/libhipcomp_zstd_compress.so) over
    ChunkBatch, shaped like :class:`DeflateEncoder`: chunk i becomes one Zstandard frame, with the content
    checksum where ``checksum`` is set.  Chunks hold at most 65536 bytes."""

    name = "Zstd"

    def __init__(self, checksum: bool = False, lib=None):
        self.lib = lib or api.zstd_compress_library()
        self.opts = api.ZstdOpts(0, 1 if checksum else 0)


class ZstdDictEncoder(_EncodeCalls, _PrepareCalls):
    """The batched Zstandard encoder for frames that use dictionaries (include/hipcomp/zstd_dict_compress.h,
    lib/libhipcomp_zstd_dict_compress.so) over ChunkBatch, shaped like :class:`ZstdEncoder`.  prepare() digests
    dictionaries into compression blobs on the device (they are not :class:`ZstdDictDecoder`'s blobs); the compress
    calls take ``prepared``, an int64 tensor with the address of every chunk's blob (0: no dictionary, the frame
    of :class:`ZstdEncoder`).  Chunks hold at most 32768 bytes."""

    name = "ZstdDict"
    _prepare_abi = "ZstdDictCompress"

    def __init__(self, checksum: bool = False, lib=None):
        self.lib = lib or api.zstd_dict_compress_library()
        self.opts = api.ZstdOpts(0, 1 if checksum else 0)

    def compress_async(self, src: ChunkBatch, max_chunk: int, temp: Optional[torch.Tensor], dst: ChunkBatch,
                       prepared: torch.Tensor, stream=None) -> int:
        return super().compress_async(src, max_chunk, temp, dst, stream, _ptr(prepared))

    def compress(self, src: ChunkBatch, prepared: torch.Tensor, max_chunk: Optional[int] = None) -> ChunkBatch:
        return super().compress(src, max_chunk, prepared)
