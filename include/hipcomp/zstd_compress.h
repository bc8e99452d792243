/*
 * hipcomp/zstd_compress.h -- batched Zstandard (RFC 8878) encoder, C ABI.
 *
 * The other half of hipcomp/zstd.h.  The three entry points live in lib/libhipcomp_zstd_compress.so, a fifth
 * companion of libhipcomp.so, and follow the compress calls of hipcomp/deflate_compress.h: same argument order,
 * same ownership, every array device-resident, every call asynchronous on `stream`.
 *
 * Frame.  Chunk i becomes ONE COMPLETE ZSTANDARD FRAME at device_compressed_ptrs[i]: the magic number, a frame
 * header with Single_Segment set and Frame_Content_Size declared (1 byte for n <= 255, 2 bytes for 256 ..
 * 65536), no dictionary ID, exactly one block with Last_Block set and, with format_opts.checksum, the
 * Content_Checksum flag and the low 32 bits of XXH64 (seed 0) of the chunk behind the block.
 * device_compressed_bytes[i] is the frame's exact length.  ZSTD_decompress, any conforming decoder and
 * hipcompBatchedZstdDecompressAsync return the chunk.
 *
 * Block.  By exact size: an RLE_Block where all n >= 2 bytes are equal; a Compressed_Block where it is strictly
 * smaller than n (which also keeps Block_Size below the frame's Block_Maximum_Size, n here); a Raw_Block
 * otherwise, a tie going to the simpler form.  n = 0 is a Raw_Block of size 0: without checksum the 9 bytes
 * 28 b5 2f fd 20 00 01 00 00.  Inside a compressed block the bytes are this encoder's own: a greedy parse with
 * a minimum match of 4 bytes and offsets up to 65535; literals Raw, RLE or Huffman-coded (at most 11 bits, one
 * stream or four, the tree described directly or FSE-compressed) by exact size; each of the three sequence
 * tables RLE, predefined or described by estimated cost; the first repeat offset used where a sequence with
 * literals repeats the offset before it.
 *
 * Chunk limit.  HIPCOMP_ZSTD_COMPRESS_MAX_CHUNK_BYTES = 65536: every match candidate lies inside the chunk, a
 * 16-bit position is enough and one block suffices.  A max chunk size above it, format_opts.level != 0 or
 * format_opts.checksum outside {0, 1} give hipcompErrorInvalidValue from all three calls; larger inputs are
 * split by the caller, as for the other batched codecs.  A chunk whose device_uncompressed_bytes[i] exceeds the
 * max_uncompressed_chunk_bytes of the call is not compressed: device_compressed_bytes[i] = 0 and nothing is
 * written for it.
 *
 * Output bound.  max_compressed_bytes = n + 14: 4 magic + 1 descriptor + 2 content size + 3 block header + 4
 * checksum.  No frame is longer than its Raw_Block form.  Whatever the input, chunk i reads only its input, at
 * any byte alignment, and writes only [out_i, out_i + max_compressed_bytes(max_uncompressed_chunk_bytes)).
 *
 * Temp space.  Per wave in flight, not per chunk: two record buffers and a literal buffer.
 * hipcompBatchedZstdCompressGetTempSize grows with batch_size up to 3072 waves (what an MI355X holds at once)
 * and is constant beyond (about 193 KiB per wave at the chunk limit).  A temp_bytes smaller than the query's
 * answer, or a device_temp_ptr that is not aligned to 4 bytes, gives hipcompErrorInvalidValue.  Two calls in
 * flight at once need a temp buffer each.
 *
 * Determinism.  A chunk's output bytes depend only on its input bytes and format_opts: not on its place in the
 * batch, its neighbours, the batch size, max_uncompressed_chunk_bytes, the addresses or the run.  Graph replays
 * and repeated calls give identical bytes.  This holds on one device model: which of several equal-hash
 * positions of a parse step stays in the match table is the hardware's rule, so another architecture may choose
 * other (equally valid) matches.
 *
 * Every function returns hipcompErrorInvalidValue for a null required pointer; batch_size == 0 is success and
 * launches nothing.  The calls launch on `stream` and never synchronise, allocate or read the host: they can be
 * captured into a HIP graph.  Input and output may lie at any byte alignment.
 */
#ifndef HIPCOMP_ZSTD_COMPRESS_H
#define HIPCOMP_ZSTD_COMPRESS_H

#include "hipcomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* level: 0 is the only value; checksum: 0 or 1 */
typedef struct
{
  int level;
  int checksum;
} hipcompBatchedZstdOpts_t;

static const hipcompBatchedZstdOpts_t hipcompBatchedZstdDefaultOpts = {0, 0};

#define HIPCOMP_ZSTD_COMPRESS_MAX_CHUNK_BYTES 65536

hipcompStatus_t hipcompBatchedZstdCompressGetTempSize(
    size_t batch_size, size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* temp_bytes);

hipcompStatus_t hipcompBatchedZstdCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* max_compressed_bytes);

hipcompStatus_t hipcompBatchedZstdCompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    hipcompBatchedZstdOpts_t format_opts,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HIPCOMP_ZSTD_COMPRESS_H */
