/*
 * hipcomp/zstd_dict_compress.h -- batched Zstandard (RFC 8878) encoder for frames that use dictionaries, C ABI.
 *
 * The other half of hipcomp/zstd_dict.h, as hipcomp/zstd_compress.h is of hipcomp/zstd.h.  The five entry points
 * live in lib/libhipcomp_zstd_dict_compress.so, a companion of libhipcomp.so.  A dictionary -- raw content or a
 * formatted dictionary (RFC 8878 section 5) -- is digested once on the device into a prepared blob; every chunk of
 * a compress call names its blob or none, and a batch may mix dictionaries.  Everything hipcomp/zstd_compress.h
 * promises holds here too: ownership, null checks, batch_size == 0, asynchrony, graph capture, containment, any
 * byte alignment of input and output, an oversized chunk left alone with size 0, the temp space and its alignment,
 * and determinism on one device model.  What differs:
 *
 * Chunk limit.  HIPCOMP_ZSTD_DICT_COMPRESS_MAX_CHUNK_BYTES = 32768.  The encoder searches the last
 * T = min(content size, 32768) bytes of the dictionary's content; where the content is shorter than 8 bytes T = 0,
 * as libzstd ignores such content.  The history, tail ++ chunk, is therefore at most 65536 bytes: a 16-bit position
 * suffices and every offset is at most 65535.  Larger dictionaries are accepted; only the tail is searched.  A max
 * chunk size above the limit, format_opts.level != 0 (level 0 is the only one) or format_opts.checksum outside
 * {0, 1} give hipcompErrorInvalidValue from the three compress calls.
 *
 * Frame.  As in hipcomp/zstd_compress.h -- Single_Segment, the content size declared, one block with Last_Block,
 * the optional checksum -- plus the dictionary's Dictionary_ID in the smallest field of 1, 2 or 4 bytes where it
 * is not zero.  Raw content has ID 0 and writes no field.  ZSTD_decompress_usingDict with the dictionary's bytes
 * and hipcompBatchedZstdDictDecompressAsync with its decoding blob return the chunk.
 *
 * Block.  The parse of hipcomp/zstd_compress.h over the history: a match may lie in the tail, end at its last
 * byte or begin there and go on into the chunk.  The first sequence's "offset of the sequence before it" is the
 * dictionary's first repeat offset (1 for raw content); repeat offsets 2 and 3 are not used.  With a formatted
 * dictionary the literals have one more form, Treeless under the dictionary's Huffman code, taken by exact size
 * where every literal has a code there (a tie with a tree of the chunk's own goes to Treeless), and each sequence
 * table one more mode, Repeat_Mode under the dictionary's distribution, by estimated cost (at a tie predefined,
 * then Repeat_Mode, then described).
 *
 * Output bound.  max_compressed_bytes = n + 18: the n + 14 of hipcomp/zstd_compress.h and 4 bytes of
 * Dictionary_ID.
 *
 * device_prepared_dicts[i] == NULL.  Chunk i is compressed without a dictionary: its bytes are exactly those
 * that hipcompBatchedZstdCompressAsync writes for the same chunk.
 *
 * An invalid blob.  A chunk that names a blob marked invalid (its prepare status was not hipcompSuccess) is not
 * compressed: device_compressed_bytes[i] = 0 and nothing is written for it.
 *
 * The prepared blob.  It is specific to compression and is not the blob of hipcomp/zstd_dict.h.  It holds no
 * pointers (a copy at another 16-byte aligned address stays valid) and must be 16-byte aligned.  Its size is a
 * function of dict_bytes alone: HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES plus min(dict_bytes, 32768) rounded
 * up to 16.  It is a pure function of the dictionary's bytes: a 64-byte header, the match table primed with the
 * tail, the dictionary's Huffman and FSE encoding tables, the tail.
 *
 * Prepare statuses.  Those of hipcompBatchedZstdDictPrepareAsync: hipcompSuccess; hipcompErrorInvalidValue for a
 * blob pointer that is not 16-byte aligned or a capacity below the size query's answer;
 * hipcompErrorCannotDecompress for a dictionary that is refused.  Both libraries refuse the same dictionaries.
 * A blob that is not prepared has a header marked invalid wherever 64 bytes fit.
 */
#ifndef HIPCOMP_ZSTD_DICT_COMPRESS_H
#define HIPCOMP_ZSTD_DICT_COMPRESS_H

#include "hipcomp/zstd_compress.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPCOMP_ZSTD_DICT_COMPRESS_MAX_CHUNK_BYTES 32768
#define HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES 14080

/* host only; dict_bytes above 2^30 gives hipcompErrorInvalidValue */
hipcompStatus_t hipcompBatchedZstdDictCompressGetPreparedSize(size_t dict_bytes, size_t* prepared_bytes);

hipcompStatus_t hipcompBatchedZstdDictCompressPrepareAsync(
    const void* const* device_dict_ptrs,
    const size_t* device_dict_bytes,
    size_t num_dicts,
    void* const* device_prepared_ptrs,
    const size_t* device_prepared_capacities,
    hipcompStatus_t* device_statuses,
    hipStream_t stream);

hipcompStatus_t hipcompBatchedZstdDictCompressGetTempSize(
    size_t batch_size, size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* temp_bytes);

hipcompStatus_t hipcompBatchedZstdDictCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* max_compressed_bytes);

hipcompStatus_t hipcompBatchedZstdDictCompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    const void* const* device_prepared_dicts,
    hipcompBatchedZstdOpts_t format_opts,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* HIPCOMP_ZSTD_DICT_COMPRESS_H */
