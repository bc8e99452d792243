/*
 * hipcomp/deflate_compress.h -- batched raw-Deflate (RFC 1951) encoder, C ABI.
 *
 * The other half of hipcomp/deflate.h.  The three entry points live in lib/libhipcomp_deflate_compress.so, a
 * second companion of libhipcomp.so, and follow the compress calls of hipcomp/snappy.h: same argument order,
 * same ownership, every array device-resident, every call asynchronous on `stream`.
 *
 * Stream format.  Chunk i becomes ONE COMPLETE RAW DEFLATE STREAM at device_compressed_ptrs[i]: one dynamic
 * block, one fixed block, or stored blocks, the last block with BFINAL set; device_compressed_bytes[i] is its
 * exact length.  zlib.decompress(stream, -15), any inflate and hipcompBatchedDeflateDecompressAsync return the
 * chunk.  There is no zlib or gzip wrapper: the caller adds it (a gzip member is a 10-byte header, the stream,
 * then CRC-32 and ISIZE of the uncompressed bytes; INTEGRATION.md has the example).  The bytes are this
 * encoder's own: a greedy parse with a minimum match of 4 bytes, distances up to 32768 and matches up to 258
 * bytes, one block per chunk, the block kind chosen by exact cost.
 *
 * Chunk limit.  HIPCOMP_DEFLATE_COMPRESS_MAX_CHUNK_BYTES = 65536: a chunk is at most two windows, so every
 * match candidate lies inside the chunk and a 16-bit position is enough.  A max chunk size above it gives
 * hipcompErrorInvalidValue from all three calls; larger inputs are split by the caller, as for the other
 * batched codecs.  A chunk whose device_uncompressed_bytes[i] exceeds the max_uncompressed_chunk_bytes of the
 * call is not compressed: device_compressed_bytes[i] = 0 and nothing is written for it.
 *
 * Output bound.  max_compressed_bytes = n + 5 * max(1, ceil(n / 65535)): the chunk as stored blocks (65546
 * for 65536 bytes, what zlib level 0 writes).  The encoder never writes a longer stream: where the Huffman-
 * coded form of a chunk would not be shorter it writes the stored form.  Whatever the input, chunk i reads
 * only its input and writes only [out_i, out_i + max_compressed_bytes(max_uncompressed_chunk_bytes)).
 *
 * Temp space.  One token buffer per wave in flight, not per chunk: hipcompBatchedDeflateCompressGetTempSize
 * grows with batch_size up to 3072 waves (what an MI355X holds at once) and is constant beyond (about 64 KiB per wave at the chunk limit).
 * A temp_bytes smaller than the query's answer, or a device_temp_ptr that is not aligned to 4 bytes, gives
 * hipcompErrorInvalidValue.  Two calls in flight at once need a temp buffer each.
 *
 * Determinism.  A chunk's output bytes depend only on its input bytes: not on its place in the batch, its
 * neighbours, the batch size, max_uncompressed_chunk_bytes, the addresses or the run.  Graph replays and
 * repeated calls give identical bytes.  This holds on one device model: which of several equal-hash positions
 * of a parse step stays in the match table is the hardware's rule, so another architecture may choose other
 * (equally valid) matches.
 *
 * Every function returns hipcompErrorInvalidValue for a null required pointer and for format_opts.algo != 0;
 * batch_size == 0 is success and launches nothing.  The calls launch on `stream` and never synchronise,
 * allocate or read the host: they can be captured into a HIP graph.  Input and output may lie at any byte
 * alignment.
 */
#ifndef HIPCOMP_DEFLATE_COMPRESS_H
#define HIPCOMP_DEFLATE_COMPRESS_H

#include "hipcomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* algo: 0 is the only value */
typedef struct
{
  int algo;
} hipcompBatchedDeflateOpts_t;

static const hipcompBatchedDeflateOpts_t hipcompBatchedDeflateDefaultOpts = {0};

#define HIPCOMP_DEFLATE_COMPRESS_MAX_CHUNK_BYTES 65536

hipcompStatus_t hipcompBatchedDeflateCompressGetTempSize(
    size_t batch_size,
    size_t max_chunk_bytes,
    hipcompBatchedDeflateOpts_t format_opts,
    size_t* temp_bytes);

/* max_compressed_bytes = n + 5 * max(1, ceil(n / 65535)) */
hipcompStatus_t hipcompBatchedDeflateCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes,
    hipcompBatchedDeflateOpts_t format_opts,
    size_t* max_compressed_bytes);

hipcompStatus_t hipcompBatchedDeflateCompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    hipcompBatchedDeflateOpts_t format_opts,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif
