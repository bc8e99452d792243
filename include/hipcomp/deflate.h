/*
 * hipcomp/deflate.h -- batched raw-Deflate (RFC 1951) decoder, C ABI.
 *
 * A format of this library's own: the reference ships no open Deflate.  The three entry points live in
 * lib/libhipcomp_deflate.so, a companion of libhipcomp.so, and follow the decode calls of hipcomp/lz4.h and
 * hipcomp/snappy.h: same argument order, same ownership, every array device-resident, every call
 * asynchronous on `stream`.  There is no encoder.
 *
 * Stream format.  Chunk i is ONE RAW DEFLATE STREAM: a sequence of blocks (stored, fixed or dynamic, all
 * three are decoded) that ends with the block whose BFINAL bit is set.  Bytes behind that block are ignored.
 * There is no zlib or gzip wrapper: the caller strips it.  A zlib stream has a 2-byte header (6 with a preset
 * dictionary, which this decoder does not take) and a 4-byte Adler-32 trailer.  A gzip member has a header of
 * 10 bytes plus its optional fields (FEXTRA, FNAME, FCOMMENT, FHCRC) and an 8-byte trailer: CRC-32, then
 * ISIZE, the uncompressed size modulo 2^32, in the member's last 4 bytes (little endian) -- the place to take
 * an output capacity from.  Input and output may lie at any byte alignment; nothing in the interface limits a
 * chunk's size below size_t.
 *
 * Success: statuses[i] = hipcompSuccess, actual[i] = the decoded size, exactly that many bytes written at
 * device_uncompressed_ptrs[i].
 * Failure: statuses[i] = hipcompErrorCannotDecompress and actual[i] = 0 -- the stream is not legal Deflate,
 * it ends before its final block does, or its output exceeds device_uncompressed_bytes[i].  The bytes of
 * [out_i, out_i + capacity_i) are then unspecified.  A failing chunk does not disturb its neighbours.
 * Containment: whatever the input, chunk i reads only [comp_i, comp_i + comp_bytes_i) and writes only
 * [out_i, out_i + capacity_i).  A match distance that reaches before the start of the chunk's own output is
 * an error, never a read.
 *
 * Every function returns hipcompErrorInvalidValue for a null required pointer; batch_size == 0 is success
 * and launches nothing.  The calls launch on `stream` and never synchronise, allocate or read the host: they
 * can be captured into a HIP graph.
 */
#ifndef HIPCOMP_DEFLATE_H
#define HIPCOMP_DEFLATE_H

#include "hipcomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* temp_bytes = 0: the decoder needs no temp space (device_temp_ptr may be NULL, and calls in flight share
 * nothing). */
hipcompStatus_t hipcompBatchedDeflateDecompressGetTempSize(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes);

/* Decodes every chunk without writing: device_uncompressed_bytes[i] = its decoded size, or 0 for a stream
 * that hipcompBatchedDeflateDecompressAsync would refuse for a reason other than capacity. */
hipcompStatus_t hipcompBatchedDeflateGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream);

/* Decompress; device_uncompressed_bytes[i] is the capacity of output i; the actual-bytes and statuses
 * arrays may be NULL. */
hipcompStatus_t hipcompBatchedDeflateDecompressAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t* device_actual_uncompressed_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif
