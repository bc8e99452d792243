/*
 * hipcomp/zstd_dict.h -- batched Zstandard (RFC 8878) decoder for frames that use dictionaries, C ABI.
 *
 * The companion of hipcomp/zstd.h for the regime Zstandard has dictionaries for: many small independent
 * chunks (blocks of an LSM store, messages, key-value records) with one dictionary per file or per table.
 * The five entry points live in lib/libhipcomp_zstd_dict.so.  Everything hipcomp/zstd.h says about the chunk
 * format, success, failure, the temp space, the checksum, skippable frames, its three Documented differences
 * and Containment holds here unchanged; this header says what a dictionary adds.  The encoder with
 * dictionaries is hipcomp/zstd_dict_compress.h, in a library of its own with a blob of its own.
 *
 * A dictionary is a buffer of at most 2^30 bytes, RAW CONTENT or FORMATTED (RFC 8878 section 5):
 *   - Raw content: any buffer shorter than 8 bytes or one that does not start with the magic number 0xEC30A437.
 *     Its ID is 0, it has no entropy tables and its repeat offsets are 1, 4, 8.  An empty dictionary is legal and
 *     means "none".
 *   - Formatted: magic, Dictionary_ID, a Huffman tree description for literals, FSE table descriptions in the
 *     order offsets, match lengths, literal lengths, three 4-byte repeat offsets, content.  It is refused where
 *     it is exactly 8 bytes, where a description is refused (maximum symbols and accuracy logs above 31 / 8,
 *     52 / 9, 35 / 9 included), where fewer than 12 bytes are left for the repeat offsets, and where a repeat
 *     offset is 0 or above the content size.
 *
 * The dictionary is digested ONCE, on the device, into a PREPARED BLOB in memory of the caller's: a header, the
 * four decoding tables as the decoder keeps them, and the content.  The blob holds no pointers: it may be copied
 * to any 16-byte aligned address, kept, and used by any number of calls.  Its size is a function of the
 * dictionary's size alone (hipcompBatchedZstdDictGetPreparedSize).
 *
 * A frame against a dictionary:
 *   - Dictionary_ID.  A non-zero Dictionary_ID must equal the ID of the dictionary given; a raw-content
 *     dictionary has ID 0 and so never matches one.  A frame with Dictionary_ID 0 or none is decoded with
 *     whatever dictionary is given.
 *   - History.  The dictionary's content precedes the frame's output: an offset is legal up to (bytes produced
 *     in this frame) + (content size); one more is an error, never a read.  The window is not enforced.
 *   - Every frame of a chunk starts again from the dictionary -- its content, its repeat offsets, its tables;
 *     the previous frame's output is never reachable.
 *   - With a formatted dictionary the first block may use Treeless literals and Repeat_Mode for each of the
 *     three sequence tables; they mean the dictionary's tables.  With raw content or none they are refused.
 *
 * device_prepared_dicts[i] is chunk i's blob; a batch may mix dictionaries.  A NULL entry means no dictionary:
 * that chunk behaves exactly as under hipcomp/zstd.h, the refusal of a non-zero Dictionary_ID included.  A chunk
 * that names a blob marked invalid (see prepare) is refused with hipcompErrorCannotDecompress.  A chunk that
 * names memory that prepare never wrote is the caller's error, like any bad pointer: nothing is promised.
 * Containment: chunk i reads only [comp_i, comp_i + comp_bytes_i) and its blob, and writes only
 * [out_i, out_i + capacity_i) and the temp space.
 *
 * The arbiter is ZSTD_decompress_usingDict of libzstd (1.4.8): what it accepts is decoded to the same bytes, what
 * it refuses is refused, dictionaries included (a Huffman tree of depth 12 is refused in a dictionary as in a
 * block, by both).  The Documented differences are the three of hipcomp/zstd.h; dictionaries add none.
 *
 * Every function returns hipcompErrorInvalidValue for a null required pointer; batch_size == 0 and
 * num_dicts == 0 are success and launch nothing.  The calls launch on `stream` and never synchronise, allocate
 * or read the host: they can be captured into a HIP graph.
 */
#ifndef HIPCOMP_ZSTD_DICT_H
#define HIPCOMP_ZSTD_DICT_H

#include "hipcomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  prepared_bytes = 9280 + round_up(dict_bytes, 16); dict_bytes above 2^30 is
 * hipcompErrorInvalidValue. */
hipcompStatus_t hipcompBatchedZstdDictGetPreparedSize(size_t dict_bytes, size_t* prepared_bytes);

/* Digest num_dicts dictionaries, one wavefront each.  device_statuses (required) gets, per dictionary:
 *   hipcompSuccess                a blob marked valid was written at device_prepared_ptrs[i];
 *   hipcompErrorCannotDecompress  the dictionary is refused (see above) or larger than 2^30 bytes;
 *   hipcompErrorInvalidValue      device_prepared_ptrs[i] is not aligned to 16 bytes, or
 *                                 device_prepared_capacities[i] is below the size query's answer.
 * In the two failing cases a header marked invalid (64 bytes) is written where the pointer is aligned and the
 * capacity holds it, and nothing else.  Dictionary i is read in [dict_i, dict_i + dict_bytes_i) only and
 * nothing but [prepared_i, prepared_i + capacity_i) is written. */
hipcompStatus_t hipcompBatchedZstdDictPrepareAsync(
    const void* const* device_dict_ptrs,
    const size_t* device_dict_bytes,
    size_t num_dicts,
    void* const* device_prepared_ptrs,
    const size_t* device_prepared_capacities,
    hipcompStatus_t* device_statuses,
    hipStream_t stream);

/* The temp size of hipcompBatchedZstdDecompressGetTempSize (the same formula): dictionaries take none. */
hipcompStatus_t hipcompBatchedZstdDictDecompressGetTempSize(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes);

/* As hipcompBatchedZstdGetDecompressSizeAsync.  Where every frame declares its size the headers are walked and
 * the Dictionary_ID rule applied (0 for a chunk it refuses, or whose blob is marked invalid); otherwise the chunk
 * is decoded without stores, with its dictionary. */
hipcompStatus_t hipcompBatchedZstdDictGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const void* const* device_prepared_dicts,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream);

/* As hipcompBatchedZstdDecompressAsync, chunk i decoded with the blob device_prepared_dicts[i] (NULL: none). */
hipcompStatus_t hipcompBatchedZstdDictDecompressAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t* device_actual_uncompressed_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses,
    const void* const* device_prepared_dicts,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif
