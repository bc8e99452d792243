/*
 * hipcomp/gzip.h -- batched gzip (RFC 1952), zlib (RFC 1950) and BGZF members around the Deflate codec, C ABI.
 *
 * hipcomp/deflate.h and hipcomp/deflate_compress.h stop at the raw RFC 1951 stream.  These entry points add what
 * stands around it: on the way in they parse and strip the header, decode the stream and VERIFY the trailer's
 * CRC-32 (gzip, BGZF) or Adler-32 (zlib) against the decoded bytes; on the way out they write header and trailer
 * with the checksum of the input chunk.  They live in lib/libhipcomp_gzip.so, a third companion library, which
 * links the two Deflate libraries and calls their C ABI: the Deflate kernels exist once.  Argument order,
 * ownership and checks follow the two Deflate headers: every array device-resident, every call asynchronous on
 * `stream`.
 *
 * One member per chunk.  Chunk i of a decode call is ONE gzip member or ONE zlib stream: its header at
 * device_compressed_ptrs[i], its trailer in the chunk's LAST 8 (gzip) or 4 (zlib) bytes.  The trailer is taken
 * from there, not from behind the stream's final block.
 * Multi-member input (a .gz file of several members, a BGZF file) is split by the caller before the call;
 * hipcompBgzfSplitHost does it for BGZF.  HIPCOMP_WRAPPER_BGZF on decode is accepted and means gzip: a BGZF
 * block is a gzip member, its 'BC' extra field is skipped like any other.
 *
 * gzip header.  ID 1f 8b, CM 8, the reserved FLG bits 5-7 zero; MTIME, XFL and OS are skipped, and so are FEXTRA,
 * FNAME and FCOMMENT; FHCRC is verified.  A field that runs into the trailer, or a chunk below 18 bytes, is
 * refused.  zlib header: CM 8, CINFO <= 7, FCHECK right, FDICT clear (a preset dictionary is refused); a chunk
 * below 6 bytes is refused.  The window CINFO declares is not enforced: distances up to 32768 are taken.
 *
 * Decode results.
 *   statuses[i] = hipcompSuccess, actual[i] = the decoded size: the header is legal, the stream decodes into the
 *     capacity, the checksum of the decoded bytes equals the trailer's and (gzip) ISIZE equals the size mod 2^32.
 *   statuses[i] = hipcompErrorCannotDecompress, actual[i] = 0: the header is refused, or the raw decoder refuses
 *     the stream (hipcomp/deflate.h says when).
 *   statuses[i] = hipcompErrorBadChecksum, actual[i] = 0: the stream decoded but the checksum or ISIZE differs.
 *   The bytes of [out_i, out_i + capacity_i) are unspecified after a failure.  Containment is the raw decoder's:
 *   chunk i reads only [comp_i, comp_i + comp_bytes_i) and writes only [out_i, out_i + capacity_i).
 *
 * A documented difference from zlib.  The raw decoder ignores bytes behind its final block.  A member with slack
 * between the final block and the trailer -- the trailer still in the chunk's last bytes -- is therefore NOT
 * refused by this library when its checksum fits; zlib reads its trailer right behind the final block and
 * refuses such a member (gzip.decompress reports a CRC failure).
 *
 * The size query strips the header and runs the raw decoder's size query on the payload: 0 for a refused header
 * or a stream the raw decoder refuses.  ISIZE is not trusted for it, and no checksum is taken.
 *
 * Compress.  Chunk i becomes one member at device_compressed_ptrs[i] with a fixed header:
 *   gzip  1f 8b 08 00 00000000 00 ff                                    (10 bytes, then the stream, CRC-32, ISIZE)
 *   zlib  78 01                                                         (2 bytes, then the stream, Adler-32)
 *   BGZF  1f 8b 08 04 00000000 00 ff 06 00 42 43 02 00 <BSIZE>          (18 bytes, then the stream, CRC-32, ISIZE)
 * BSIZE is the member's length - 1.  The payload bytes are the raw encoder's: what
 * hipcompBatchedDeflateCompressAsync writes for the same chunk.  Determinism carries over: a member's bytes depend
 * only on its input bytes and the wrapper, on one device model (hipcomp/deflate_compress.h).
 * Output bound: max_member_bytes = the raw encoder's bound n + 5 * max(1, ceil(n / 65535)) plus 18 (gzip), 6 (zlib)
 * or 26 (BGZF); nothing is written at or beyond it.  The chunk limit is the raw encoder's 65536 bytes; for BGZF it
 * is HIPCOMP_BGZF_MAX_CHUNK_BYTES, so that a stored member stays within the 65536 bytes BSIZE can express.  A
 * chunk larger than max_uncompressed_chunk_bytes is not compressed: device_compressed_bytes[i] = 0, no bytes.
 * A BGZF file is the members back to back followed by hipcompBgzfEofBlock.
 *
 * Temp space.  Decode: 40 bytes per member.  Compress: the raw encoder's temp space and 8 bytes per chunk.  A
 * temp_bytes below the query's answer or a device_temp_ptr not aligned to 8 bytes gives hipcompErrorInvalidValue.
 * Two calls in flight at once need a temp buffer each.
 *
 * Every function returns hipcompErrorInvalidValue for a null required pointer, an unknown wrapper and a chunk
 * size above the limit, before anything is launched; batch_size == 0 is success and launches nothing.  The
 * device calls launch on `stream` and never synchronise, allocate or read the host: they can be captured into a
 * HIP graph.  Input and output may lie at any byte alignment.  hipcompBgzfSplitHost is host code.
 */
#ifndef HIPCOMP_GZIP_H
#define HIPCOMP_GZIP_H

#include "hipcomp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum
{
  HIPCOMP_WRAPPER_GZIP = 0,
  HIPCOMP_WRAPPER_ZLIB = 1,
  HIPCOMP_WRAPPER_BGZF = 2
} hipcompDeflateWrapper_t;

/* wrapper: a hipcompDeflateWrapper_t */
typedef struct
{
  int wrapper;
} hipcompBatchedGzipOpts_t;

static const hipcompBatchedGzipOpts_t hipcompBatchedGzipDefaultOpts = {HIPCOMP_WRAPPER_GZIP};

/* htslib's block size: a stored member of it stays within 65536 bytes */
#define HIPCOMP_BGZF_MAX_CHUNK_BYTES 65280

/* the empty BGZF block that ends a BGZF file */
#define HIPCOMP_BGZF_EOF_BLOCK_BYTES 28
static const unsigned char hipcompBgzfEofBlock[HIPCOMP_BGZF_EOF_BLOCK_BYTES] = {
    0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
    0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

hipcompStatus_t hipcompBatchedGzipDecompressGetTempSize(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes);

/* device_uncompressed_bytes[i] = the decoded size of member i, or 0 (see above) */
hipcompStatus_t hipcompBatchedGzipGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipcompDeflateWrapper_t wrapper,
    void* device_temp_ptr,
    size_t temp_bytes,
    hipStream_t stream);

/* Decompress and verify; device_uncompressed_bytes[i] is the capacity of output i; the actual-bytes and
 * statuses arrays may be NULL. */
hipcompStatus_t hipcompBatchedGzipDecompressAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t* device_actual_uncompressed_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses,
    hipcompDeflateWrapper_t wrapper,
    hipStream_t stream);

hipcompStatus_t hipcompBatchedGzipCompressGetTempSize(
    size_t batch_size,
    size_t max_chunk_bytes,
    hipcompBatchedGzipOpts_t format_opts,
    size_t* temp_bytes);

/* max_member_bytes = n + 5 * max(1, ceil(n / 65535)) + 18 (gzip), 6 (zlib) or 26 (BGZF) */
hipcompStatus_t hipcompBatchedGzipCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes,
    hipcompBatchedGzipOpts_t format_opts,
    size_t* max_member_bytes);

hipcompStatus_t hipcompBatchedGzipCompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    hipcompBatchedGzipOpts_t format_opts,
    hipStream_t stream);

/* Walks the BSIZE chain of a BGZF file in HOST memory: offsets[i] is where block i starts, *count how many
 * blocks were found (at most `capacity`), *stopped_at where the walk ended: n for a whole file, else the offset
 * of the first block that is not whole (truncated, no 'BC' field, a BSIZE that points past the end) or of block
 * number `capacity`.  Block i is [offsets[i], offsets[i + 1]), the last one ends at *stopped_at. */
hipcompStatus_t hipcompBgzfSplitHost(
    const void* host_bytes,
    size_t n,
    size_t* offsets,
    size_t capacity,
    size_t* count,
    size_t* stopped_at);

#ifdef __cplusplus
}
#endif

#endif
