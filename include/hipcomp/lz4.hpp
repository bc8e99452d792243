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

private:
  struct Impl;
  std::unique_ptr<Impl> impl;
};

} // namespace hipcomp

#endif
