/*
 * hipcomp/snappy.hpp -- Snappy manager of the high-level interface (reference
 * include/hipcomp/snappy.hpp:58-69): the input is cut into chunks of uncomp_chunk_size
 * bytes, each compressed as a raw Snappy block (hipcomp/snappy.h).
 */
#ifndef HIPCOMP_SNAPPY_HPP
#define HIPCOMP_SNAPPY_HPP

#include "hipcompManager.hpp"

namespace hipcomp
{

struct SnappyFormatSpecHeader
{
  /* empty, as in the reference: one byte of the container */
};

/* where compress_frame puts the chunk index of a seekable framed stream: nowhere, or behind the stream identifier */
enum class SnappyFrameIndex
{
  None,
  Leading
};

/* the codec of a Parquet column, from the file's footer (the caller has it) */
enum class ParquetCodec
{
  Uncompressed,
  Snappy
};

/* one listed page of a column chunk, written on the device by decompress_parquet_pages (72 bytes) */
struct ParquetPageInfo
{
  uint64_t header_offset, body_offset;                  /* in the column chunk */
  uint64_t out_offset;                                  /* of the page's decoded body in the chunk's output */
  uint32_t compressed_page_size, uncompressed_page_size;
  uint32_t kind;                                        /* 0 DATA_PAGE, 2 DICTIONARY_PAGE, 3 DATA_PAGE_V2 */
  uint32_t num_values, encoding;
  uint32_t rep_levels_bytes, def_levels_bytes;          /* V2; 0 otherwise */
  uint32_t num_nulls, num_rows;                         /* V2; 0 otherwise */
  uint32_t crc, flags;                                  /* flags: 1 has_crc, 2 values are stored (not compressed) */
  uint32_t pad;
};

/* (test and measurement hook, not a stable interface: see get_parquet_pages_stats) what the last
   decompress_parquet_pages of a manager found (host values): the items it was given, the listed pages of those that
   went to the passes, the passes they took and the pages a pass holds */
struct ParquetPagesStats
{
  size_t items, pages, passes, pass_pages;
};

struct SnappyManager : hipcompManagerBase
{
  /* device_id must be the current device */
  SnappyManager(size_t uncomp_chunk_size, hipStream_t user_stream = 0, int device_id = 0);
  SnappyManager(size_t uncomp_chunk_size, hipStream_t user_stream, int device_id, ChecksumPolicy checksum_policy);
  ~SnappyManager() override;
  SnappyManager(const SnappyManager&) = delete;
  SnappyManager& operator=(const SnappyManager&) = delete;

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

  /* ---- Snappy framed streams (magic ff 06 00 00 "sNaPpY": .sz files, Go's snappy.Writer / Reader, snzip,
     python-snappy's stream classes) on the device ----
     All buffers are device-accessible and may lie at any byte alignment; all four methods work on the manager's
     stream and only configure_frame_decompression synchronises it; the status goes to cfg.get_status();
     get_required_scratch_buffer_size() is what it was (a pass takes as many chunks as fit).  INTEGRATION.md,
     "Snappy framed streams in the Snappy manager", has the contract in full.  C++ only: no C or Python binding.

     Writing: one stream: the identifier, then one data chunk per manager chunk in chunk order -- type 0x00 with
     exactly the block hipcompBatchedSnappyCompressAsync writes for the chunk where that is strictly shorter than
     the chunk, else type 0x01 with the chunk itself.  Every data chunk carries the masked CRC-32C of its
     uncompressed bytes, computed on the device under every ChecksumPolicy: it is part of the format.  0 bytes give
     the 10-byte identifier alone.  cfg.max_compressed_buffer_size = 10 + num_chunks * (uncomp_chunk_size + 8) (the
     last chunk counted whole); nothing is written at or beyond it.  *frame_bytes (one device-accessible, 8-byte
     aligned word, written on the stream) is the exact length.  uncomp_chunk_size > 65536, the most a data chunk
     holds: the configuration has hipcompErrorInvalidValue and sizes 0, compress_frame launches nothing but
     *frame_bytes = 0. */
  CompressionConfig configure_frame_compression(size_t decomp_buffer_size);
  void compress_frame(const uint8_t* decomp_buffer, uint8_t* frame, const CompressionConfig& comp_config,
                      size_t* frame_bytes);
  /* Reading: `frames` holds zero or more streams back to back, written by anyone: compressed and uncompressed data
     chunks of up to 65536 bytes of content, repeated identifiers, padding (0xfe) and reserved skippable chunks
     (0x80 - 0xfd) anywhere.  The configuration holds the sum of the stored lengths and of the compressed chunks'
     length preambles, and the number of data chunks.  hipcompErrorCannotDecompress: a first chunk that is not the
     identifier, an identifier of another length or body, a reserved unskippable type (0x02 - 0x7f), a header or body
     that runs past frames_bytes, a data chunk without room for its CRC, a compressed chunk without payload, a
     preamble that is no complete varint of at most 5 bytes or exceeds 65536, an uncompressed chunk of more than
     65536 bytes -- these configure 0 / 0 with the status set, and decompress_frame then launches nothing -- and,
     from decompress_frame, a block the batched decoder refuses or that decodes to another size than its preamble.
     Under a verifying policy a data chunk whose masked CRC does not fit gives hipcompErrorBadChecksum (it wins over
     CannotDecompress; the CRC of a chunk whose decode failed is not looked at); under the other policies the CRCs
     are not looked at -- readers elsewhere always check.  Every data chunk carries a CRC, so ComputeAndVerify never
     reports hipcompErrorCannotVerifyChecksums here.
     Reads stay inside frames[0, frames_bytes), writes inside decomp_buffer[0, decomp_data_size) and the scratch.
     The chunk chain is followed by one lane: the format has no index. */
  DecompressionConfig configure_frame_decompression(const uint8_t* frames, size_t frames_bytes);
  void decompress_frame(uint8_t* decomp_buffer, const uint8_t* frames, size_t frames_bytes,
                        const DecompressionConfig& decomp_config);

  /* ---- Seekable Snappy framed streams: a chunk index in a reserved skippable chunk behind the identifier ----
     INTEGRATION.md, "Seekable Snappy framed streams", has the layout, the contract and the fallback rule.
     Writing: SnappyFrameIndex::None is the call above, byte for byte.  Leading writes, behind the identifier, one
     chunk of the reserved skippable type 0xa5 -- "HCSNPIDX", version, flags, uncomp_chunk_size, num_chunks, the
     content size, the first four bytes of every data chunk as they stand in the stream, a masked CRC-32C: 40 +
     4 * num_chunks bytes -- and behind it the very data chunks the call above writes.  Readers elsewhere step over
     the chunk: the result is still a plain .sz file.  max_compressed_buffer_size is the bound above plus 40 +
     4 * num_chunks, *frame_bytes counts the index.  More than 4 194 294 chunks do not fit the chunk's length
     field: hipcompErrorInvalidValue and sizes 0, like uncomp_chunk_size > 65536.
     Reading: configure_frame_decompression and decompress_frame find the index themselves.  Where `frames` is
     streams of the form written here and nothing else but padding and skippable chunks between them, the data
     chunks are found by a scan of the index, not by following the chain.  The index is not trusted: it is used
     only where every word is found at its scanned place in the stream, with a type, length and preamble that fit
     the chunk's share of the content, and every compressed chunk decodes to exactly that share; in every other
     case the call carries on as if the index were any skippable chunk, with the status, size and bytes it has
     without it. */
  CompressionConfig configure_frame_compression(size_t decomp_buffer_size, SnappyFrameIndex index);
  void compress_frame(const uint8_t* decomp_buffer, uint8_t* frame, const CompressionConfig& comp_config,
                      size_t* frame_bytes, SnappyFrameIndex index);
  /* Bytes [first_byte, first_byte + num_bytes) of the content decompress_frame would produce for `frames` into
     out[0, num_bytes): only the data chunks the range touches are read, decoded or copied and, under a verifying
     policy, checked -- each of them whole -- against their CRCs.  `frames` has to be streams as written with
     SnappyFrameIndex::Leading -- up to 32 of them, padding and skippable chunks between them -- and every index has
     to be found in its stream, word for word: anything else is hipcompErrorNotSupported with nothing written to
     out, as is an index of chunks so large that two of them do not fit this manager's scratch space.  A range that
     ends beyond decomp_data_size: hipcompErrorInvalidValue; num_bytes == 0 succeeds and launches nothing.  A
     touched chunk that does not decode to its share: hipcompErrorCannotDecompress, a CRC that does not fit:
     hipcompErrorBadChecksum; chunks the range does not touch are not looked at.  Reads stay inside
     frames[0, frames_bytes), writes inside out[0, num_bytes) and the scratch.  The call synchronises the stream
     once: the host reads the table of streams the device made. */
  void decompress_frame_range(uint8_t* out, const uint8_t* frames, size_t frames_bytes,
                              const DecompressionConfig& decomp_config, size_t first_byte, size_t num_bytes);
  /* the data chunks the last decompress_frame found by following the chain: 0 where the index served, num_chunks
     where there was none or it was refused (synchronises the stream) */
  size_t get_frame_walked_chunks();

  /* ---- The pages of Parquet column chunks, a batch of chunks in one call ----
     INTEGRATION.md, "Parquet column chunks in the Snappy manager", has the contract in full and a worked example.
     Item i is one column chunk as it lies in the file: the bytes [first page header, + total_compressed_size), a
     chain of Thrift compact-protocol PageHeaders with their bodies; `codec` is the column's, from the footer.  The
     item's output is the decoded bodies of its listed pages -- data pages V1 and V2 and dictionary pages; index pages
     and pages of unknown kinds are stepped over -- back to back in page order, without the headers; the levels of a
     V2 page are copied, its values decoded behind them.  device_actual_bytes[i] is the sum of the pages'
     uncompressed_page_size, device_num_pages[i] the number of listed pages; both are 0 for an item that failed.
     device_page_ptrs: nullptr, or per item a table of device_page_capacities[i] rows that takes one ParquetPageInfo
     per listed page; an item with more pages than rows is hipcompErrorInvalidValue and nothing of it is written.
     hipcompErrorCannotDecompress: a header the Thrift reader or the page rules refuse, a body that runs past the
     chunk, bytes behind the last page that are no page, an output that does not hold the pages (nothing of the item
     is written then), a block the batched decoder refuses or that decodes to another size than its header says.
     Page CRCs (the gzip CRC-32 of the stored body) follow the manager's ChecksumPolicy: compared under a verifying
     policy -- hipcompErrorBadChecksum, which wins over CannotDecompress --; under ComputeAndVerify an item with a
     page without one is hipcompErrorCannotVerifyChecksums with its bytes and size in place.
     All arrays are in device memory; chunks and outputs may lie at any byte alignment (a page table at a
     ParquetPageInfo's).  No item's status, size, bytes or table depend on any other item.  Reads stay inside the
     items, writes inside each item's capacity, its table's capacity and the scratch.  get_parquet_pages_sizes is
     the walk alone and does not synchronise; decompress_parquet_pages synchronises the stream once, to read the
     number of listed pages of the batch and the size of its largest stored part.  get_required_scratch_buffer_size()
     is what it was: a pass takes as many pages as fit; a caller's scratch that does not hold the items' states and
     two pages' entries throws before anything is launched.  At most 2^20 items.  C++ only. */
  void get_parquet_pages_sizes(const uint8_t* const* device_chunk_ptrs, const size_t* device_chunk_bytes,
                               size_t* device_num_pages, size_t* device_decompressed_bytes,
                               hipcompStatus_t* device_statuses, size_t num_chunks, ParquetCodec codec);
  void decompress_parquet_pages(const uint8_t* const* device_chunk_ptrs, const size_t* device_chunk_bytes,
                                uint8_t* const* device_out_ptrs, const size_t* device_out_capacities,
                                size_t* device_actual_bytes, hipcompStatus_t* device_statuses,
                                ParquetPageInfo* const* device_page_ptrs, const size_t* device_page_capacities,
                                size_t* device_num_pages, size_t num_chunks, ParquetCodec codec);
  /* Test and measurement hooks, not a stable interface.  set_parquet_pass_pages: at most `pages` pages per pass of
     decompress_parquet_pages (0, the default: as many as the scratch holds).  get_parquet_pages_stats: what the last
     decompress_parquet_pages found (a call that threw counts nothing). */
  void set_parquet_pass_pages(size_t pages);
  ParquetPagesStats get_parquet_pages_stats() const;

private:
  struct Impl;
  std::unique_ptr<Impl> impl;
};

} // namespace hipcomp

#endif
