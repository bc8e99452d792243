/*
 * hipcomp/zstd.h -- batched Zstandard (RFC 8878) decoder, C ABI.
 *
 * A format of this library's own, like hipcomp/deflate.h: the reference ships no Zstandard.  The three entry
 * points live in lib/libhipcomp_zstd.so, a companion of libhipcomp.so, and follow the decode calls of
 * hipcomp/deflate.h: same argument order, same ownership, every array device-resident, every call asynchronous
 * on `stream`.  There is no encoder.
 *
 * Chunk format.  Chunk i is ZERO OR MORE CONCATENATED ZSTANDARD FRAMES; the decoded chunk is their contents one
 * after the other.  Skippable frames (magic 0x184D2A50 .. 0x184D2A5F) are skipped, before, between and after
 * data frames.  Every block type, literals type and sequence mode of the format is decoded.  There are no
 * dictionaries: a frame with a non-zero Dictionary_ID is refused.  Legacy (pre-0.8) frame formats are not
 * taken, and a frame cannot continue over several calls.  A frame that sets Content_Checksum has its 4
 * trailing bytes verified: the low 32 bits of XXH64, seed 0, of the frame's content.  Input and output may lie
 * at any byte alignment.
 *
 * Success: statuses[i] = hipcompSuccess, actual[i] = the decoded size, exactly that many bytes written at
 * device_uncompressed_ptrs[i].
 * Failure: statuses[i] = hipcompErrorCannotDecompress and actual[i] = 0 -- the input is not legal (a reserved
 * bit or block type, a table description that is refused, a bitstream without its final-bit marker or not
 * exactly consumed, a Block_Size past the bytes left or, for a compressed block, of 128 KiB or more, ...), it
 * ends early, its output exceeds device_uncompressed_bytes[i], a declared Frame_Content_Size differs from what
 * the frame decodes to, the checksum does not match (the same status as the other failures), or a block's
 * literals outgrow the wave's share of the temp space (see the temp size).  The bytes of
 * [out_i, out_i + capacity_i) are then unspecified.  A failing chunk does not disturb its neighbours.
 * Containment: whatever the input, chunk i reads only [comp_i, comp_i + comp_bytes_i) and writes only
 * [out_i, out_i + capacity_i) and the temp space.  An offset that reaches before the start of the FRAME's own
 * output is an error, never a read.
 *
 * The arbiter is ZSTD_decompress of libzstd (1.4.8): what it accepts is decoded to the same bytes, what it
 * refuses is refused.  Documented differences:
 *   1. A sequences bitstream that is read past its start, or whose lowest bits no sequence reads.  libzstd 1.4.8
 *      goes on with the bits its register happens to hold, reads three more states behind the last sequence,
 *      and accepts the block unless bits are left over after that; this decoder refuses both (RFC 8878: the
 *      last sequence's extra bits end the bitstream exactly).
 *   2. FSE-compressed Huffman weights whose bitstream is shorter than its two initial states: libzstd 1.4.8
 *      goes on in the same way; this decoder refuses the block.
 *   3. A Huffman stream that is read past its start by its last symbol.  Where libzstd 1.4.8 decodes two
 *      symbols per lookup it tolerates that; this decoder requires every stream to be consumed exactly.
 * A Huffman tree of depth 12 is refused by both.
 * No legal frame falls under any of them.
 *
 * Every function returns hipcompErrorInvalidValue for a null required pointer; batch_size == 0 is success and
 * launches nothing.  The calls launch on `stream` and never synchronise, allocate or read the host: they can be
 * captured into a HIP graph.
 */
#ifndef HIPCOMP_ZSTD_H
#define HIPCOMP_ZSTD_H

#include "hipcomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The decoder keeps the literals of the block it works on in temp space, one buffer per wave that the launch
 * can have: temp_bytes = min(num_chunks, 3072) * round_up(min(128 KiB, max_uncompressed_chunk_bytes), 256).
 * Calls in flight at the same time need temp space of their own. */
hipcompStatus_t hipcompBatchedZstdDecompressGetTempSize(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes);

/* device_uncompressed_bytes[i] = the decoded size of chunk i, or 0 for a chunk that
 * hipcompBatchedZstdDecompressAsync would refuse for a reason other than capacity, as far as that shows
 * without an output:
 *   - Where every frame of the chunk declares its Frame_Content_Size, the result is the sum of the declared
 *     sizes.  The frame and block headers are walked (0 for a chunk whose headers are refused or that ends
 *     early) and nothing is decoded: for a frame whose declared size is false the query returns the DECLARED
 *     size, and the decompress call then refuses the chunk.
 *   - Otherwise the chunk is decoded without writing, with every check of the decompress call except the
 *     checksum. */
hipcompStatus_t hipcompBatchedZstdGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream);

/* Decompress; device_uncompressed_bytes[i] is the capacity of output i; the actual-bytes and statuses arrays
 * may be NULL.  temp_bytes below what the size query returns for (batch_size, 1) is
 * hipcompErrorInvalidValue.  The temp space is shared out evenly among the launch's waves (in units of 256
 * bytes, at most 128 KiB each): with the size queried for the batch's largest capacity every legal chunk fits. */
hipcompStatus_t hipcompBatchedZstdDecompressAsync(
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
