/*
 * hipcomp/lz4.hpp -- LZ4 manager of the high-level interface (reference
 * include/hipcomp/lz4.hpp:58-70): the input is cut into chunks of uncomp_chunk_size bytes,
 * each compressed as an LZ4 block with elements of data_type (hipcomp/lz4.h).
 */
#ifndef HIPCOMP_LZ4_HPP
#define HIPCOMP_LZ4_HPP

#include "hipcompManager.hpp"

namespace hipcomp
{

struct LZ4FormatSpecHeader
{
  hipcompType_t data_type;
};

/* where compress_frame puts the block index of a seekable frame: nowhere, or in front of the frame */
enum class LZ4FrameIndex
{
  None,
  Leading
};

/* what stands in front of every item of decompress_frames: nothing, or the eight bytes of an Arrow IPC buffer */
enum class LZ4FramePrefix
{
  None,
  ArrowLength
};

/* (test and measurement hook, not a stable interface: see get_frames_stats) what the last decompress_frames /
   get_frames_decompressed_sizes of a manager found (host values, no synchronisation): the items it was given, the data blocks of all of them, the passes they took and the entries
   one pass held */
struct LZ4FramesStats
{
  size_t items;
  size_t blocks;
  size_t passes;
  size_t pass_entries;
};

struct LZ4Manager : hipcompManagerBase
{
  /* uncomp_chunk_size at most 16 MiB (the LZ4 block limit); device_id must be the current device */
  LZ4Manager(size_t uncomp_chunk_size, hipcompType_t data_type, hipStream_t user_stream = 0, const int device_id = 0);
  LZ4Manager(size_t uncomp_chunk_size, hipcompType_t data_type, hipStream_t user_stream, const int device_id,
             ChecksumPolicy checksum_policy);
  ~LZ4Manager() override;
  LZ4Manager(const LZ4Manager&) = delete;
  LZ4Manager& operator=(const LZ4Manager&) = delete;

  CompressionConfig configure_compression(const size_t decomp_buffer_size) override;
  void compress(const uint8_t* decomp_buffer, uint8_t* comp_buffer, const CompressionConfig& comp_config) override;
  DecompressionConfig configure_decompression(const uint8_t* comp_buffer) override;
  DecompressionConfig configure_decompression(const CompressionConfig& comp_config) override;
  void decompress(uint8_t* decomp_buffer, const uint8_t* comp_buffer, const DecompressionConfig& decomp_config) override;
  void set_scratch_buffer(uint8_t* new_scratch_buffer) override;
  size_t get_required_scratch_buffer_size() override;
  size_t get_compressed_output_size(uint8_t* comp_buffer) override;
  /* bytes [first_byte, first_byte + num_bytes) of the uncompressed buffer into out[0, num_bytes): only the chunks
     the range touches are read, decoded and checked (hipcompManager.hpp, "Ranged reads") */
  void decompress_range(uint8_t* out, const uint8_t* comp_buffer, const DecompressionConfig& decomp_config,
                        size_t first_byte, size_t num_bytes);
  /* many ranges in one call, the ranges in device memory: range r into out[off[r], off[r] + num[r]), off the
     exclusive sum of the lengths; every chunk some range touches is decoded and checked once (hipcompManager.hpp,
     "Reading many ranges") */
  void decompress_ranges(uint8_t* out, size_t out_bytes, const uint8_t* comp_buffer, const DecompressionConfig& decomp_config,
                         const size_t* device_first_bytes, const size_t* device_num_bytes, size_t num_ranges,
                         size_t* device_out_offsets);
  size_t get_ranges_pass_chunks() const;
  RangesStats get_ranges_stats() const;

  /* ---- LZ4 frames (magic 0x184D2204: .lz4 files, LZ4F_compressFrame, Arrow IPC buffers) on the device ----
     The frame is the standard layout of what a manager does: one device buffer to one self-describing buffer and
     back.  All buffers are device-accessible and may lie at any byte alignment; all four methods work on the
     manager's stream and only configure_frame_decompression synchronises it; the status goes to
     cfg.get_status(); get_required_scratch_buffer_size() is what it was (a pass takes as many blocks as fit).
     INTEGRATION.md, "LZ4 frames", has the contract in full.  C++ only: there is no C or Python binding.

     Writing: one frame, version 01, B.Indep, C.Size with the content size, no DictID, block maximum the smallest
     of 64 KiB / 256 KiB / 1 MiB / 4 MiB that holds uncomp_chunk_size; one data block per chunk in chunk order,
     each exactly the stream hipcompBatchedLZ4CompressAsync writes for the chunk with this manager's data_type,
     or the chunk itself (stored, bit 31 of the size word) where that stream is not smaller; the EndMark.  Under a
     computing ChecksumPolicy B.Checksum is set and every block is followed by the XXH32 of its stored bytes.
     C.Checksum is never written: XXH32 over the whole content is one serial chain by the construction of the hash.
     cfg.max_compressed_buffer_size = 15 + num_chunks * (uncomp_chunk_size + 4 [+ 4 with block checksums]) + 4
     (the last chunk counted whole); nothing is written at or beyond it.  *frame_bytes (one device-accessible,
     8-byte aligned word, written on the stream) is the exact length.  uncomp_chunk_size > 4 MiB: the
     configuration has hipcompErrorInvalidValue and sizes 0, compress_frame launches nothing but *frame_bytes = 0. */
  CompressionConfig configure_frame_compression(size_t decomp_buffer_size);
  void compress_frame(const uint8_t* decomp_buffer, uint8_t* frame, const CompressionConfig& comp_config,
                      size_t* frame_bytes);
  /* Reading: `frames` holds zero or more frames back to back, skippable frames (0x184D2A50 - 0x184D2A5F) anywhere
     between them, written by anyone: every block maximum, independent and linked blocks, stored blocks, short
     blocks anywhere, content size and either checksum present or not.  A dictionary id and the legacy magic are
     hipcompErrorNotSupported; everything else LZ4F_decompress refuses is hipcompErrorCannotDecompress.  The
     configuration holds the sum of the declared content sizes where every frame declares one (a false declaration
     is refused by decompress_frame), else the sizes found by a parse; num_chunks is the number of data blocks.  A
     refused input configures 0 / 0 with the status set, and decompress_frame then launches nothing.
     Under a verifying policy block checksums and content checksums are checked where a frame carries them
     (hipcompErrorBadChecksum), ComputeAndVerify reports hipcompErrorCannotVerifyChecksums for a frame that carries
     neither; under the other policies they are skipped (LZ4F_decompress always checks what is present).
     Reads stay inside frames[0, frames_bytes), writes inside decomp_buffer[0, decomp_data_size) and the scratch.
     A linked-block frame is decoded by one wavefront, block after block: that is the format's property. */
  DecompressionConfig configure_frame_decompression(const uint8_t* frames, size_t frames_bytes);
  void decompress_frame(uint8_t* decomp_buffer, const uint8_t* frames, size_t frames_bytes,
                        const DecompressionConfig& decomp_config);

  /* ---- Seekable LZ4 frames: a block index in a skippable frame in front of the frame it describes ----
     INTEGRATION.md, "Seekable LZ4 frames", has the layout, the contract and the fallback rule.
     Writing: LZ4FrameIndex::None is the call above, byte for byte.  Leading writes the index -- magic 0x184D2A54,
     "HCLZ4IDX", version, flags, uncomp_chunk_size, the number of blocks, the content size, the size word of every
     block as it stands in the frame, an XXH32: 44 + 4 * num_chunks bytes -- and behind it the very frame the call
     above writes for the same input.  Every reader of the format skips the index, the result is still a plain
     .lz4 file.  max_compressed_buffer_size is the bound above plus 44 + 4 * num_chunks, *frame_bytes counts the
     index, the call stays asynchronous and get_required_scratch_buffer_size() what it is.
     Reading: configure_frame_decompression and decompress_frame find the index themselves.  Where `frames` is
     indexed frames of the form written here and nothing else but skippable frames of other magics between them,
     the blocks are found by a scan of the index and not by following the chain of size words, and no block is
     parsed twice.  The index is untrusted: it is used only where every word of it is found in its place in the
     frame and every compressed block decodes to exactly its share of the content; in every other case the call
     carries on as if the index were any skippable frame, with the status, size and bytes it has without it. */
  CompressionConfig configure_frame_compression(size_t decomp_buffer_size, LZ4FrameIndex index);
  void compress_frame(const uint8_t* decomp_buffer, uint8_t* frame, const CompressionConfig& comp_config,
                      size_t* frame_bytes, LZ4FrameIndex index);
  /* Bytes [first_byte, first_byte + num_bytes) of the content decompress_frame would produce for `frames` into
     out[0, num_bytes): only the blocks the range touches are read, decoded (stored ones copied) and, under a
     verifying policy, checked against their block checksums.  `frames` has to be indexed frames as written with
     LZ4FrameIndex::Leading -- several of them, skippable frames of other magics between them -- and every index
     has to be found in its frame, size word for size word: anything else is hipcompErrorNotSupported with nothing
     written to out.  A range that ends beyond decomp_config.decomp_data_size is hipcompErrorInvalidValue;
     num_bytes == 0 succeeds and launches nothing.  A touched block that does not decode to its share of the
     content is hipcompErrorCannotDecompress, a wrong block checksum hipcompErrorBadChecksum; blocks the range
     does not touch are not looked at.  Reads stay inside frames[0, frames_bytes), writes inside out[0, num_bytes)
     and the scratch.  The call synchronises the stream once: the host reads the table of frames the device made. */
  void decompress_frame_range(uint8_t* out, const uint8_t* frames, size_t frames_bytes,
                              const DecompressionConfig& decomp_config, size_t first_byte, size_t num_bytes);
  /* the data blocks the last decompress_frame found by following the chain: 0 where the index served, num_chunks
     where it did not.  Synchronises the stream; meant for tests and for telling why a read was slow. */
  size_t get_frame_walked_blocks();

  /* ---- A batch of LZ4 frames in one call: the buffers of an Arrow IPC record batch, the files of a directory ----
     INTEGRATION.md, "Batches of LZ4 frames", has the contract in full and a worked Arrow body.
     Item i is device_item_ptrs[i][0, device_item_bytes[i]), decoded into device_out_ptrs[i][0,
     device_out_capacities[i]); all six arrays are in device memory, buffers may lie at any byte alignment.
     LZ4FramePrefix::None: an item is exactly what decompress_frame accepts as `frames` (an index in front of a
     frame is skipped like any skippable frame: the batch has no index fast path).
     LZ4FramePrefix::ArrowLength: an item of 0 bytes is an empty buffer (success, size 0); otherwise its first eight
     bytes are a little-endian int64 p: -1, the remaining bytes are the buffer itself and are copied; p >= 0, the
     remaining bytes are read as under None and have to decode to exactly p bytes (a p above the capacity is refused
     before a byte is written); 1 to 7 bytes or p < -1, hipcompErrorCannotDecompress.
     device_statuses[i] is what decompress_frame says for the item's bytes under this manager's ChecksumPolicy
     (hipcompErrorBadChecksum before the walk's refusal before hipcompErrorCannotDecompress before
     hipcompErrorCannotVerifyChecksums -- which an item stored whole gets too under ComputeAndVerify -- before
     success); device_actual_bytes[i] is the decoded size, 0 for an item that failed (CannotVerifyChecksums is no
     failure: the bytes are there).  No item's status, size or bytes depend on any other item.  Reads stay inside the
     items, writes inside each item's capacity and the scratch.
     get_frames_decompressed_sizes: under ArrowLength the prefix (bytes - 8 for -1) with nothing parsed; under None the
     sum of the declared content sizes where every frame of the item declares one (a false declaration is returned as
     declared and refused by the decode), else the size found by a parse -- what configure_frame_decompression
     gives as decomp_data_size, which is not yet a promise that the item decodes; 0 for an item the walk refuses
     (a header, a size word or a length that does not fit: what configure_frame_decompression refuses).
     num_items == 0 launches nothing; more than 2^20 items or a null array throws.  Each call works on the manager's
     stream and synchronises it once (the host reads how many data blocks the device found); the size query under
     ArrowLength does not synchronise.  get_required_scratch_buffer_size() is what it was: a pass takes as many blocks
     as fit, whatever items they belong to.  The manager's own scratch is grown to hold the items' state (160 bytes
     each); a caller's scratch that cannot hold that and two blocks' entries throws. */
  void decompress_frames(const uint8_t* const* device_item_ptrs, const size_t* device_item_bytes,
                         uint8_t* const* device_out_ptrs, const size_t* device_out_capacities, size_t* device_actual_bytes,
                         hipcompStatus_t* device_statuses, size_t num_items, LZ4FramePrefix prefix);
  void get_frames_decompressed_sizes(const uint8_t* const* device_item_ptrs, const size_t* device_item_bytes,
                                     size_t* device_decompressed_bytes, size_t num_items, LZ4FramePrefix prefix);
  /* TEST AND MEASUREMENT HOOKS, NOT A STABLE INTERFACE: they exist because a caller's scratch buffer has no size
     argument through which a test could make a pass small, and may change or go in any release; production code has
     no use for either.  set_frames_pass_entries: at most `entries` block entries per pass of the two calls above
     (0, the default: as many as the scratch holds).  get_frames_stats: what the last of the two calls found (a call
     that threw: all zero). */
  void set_frames_pass_entries(size_t entries);
  LZ4FramesStats get_frames_stats() const;

private:
  struct Impl;
  std::unique_ptr<Impl> impl;
};

} // namespace hipcomp

#endif
