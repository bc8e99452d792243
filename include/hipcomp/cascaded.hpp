/*
 * hipcomp/cascaded.hpp -- Cascaded manager of the high-level interface (reference
 * include/hipcomp/cascaded.hpp:55-68): the input is cut into chunks of options.chunk_size
 * bytes (the CONTAINER's chunk size; 4096 by default), each compressed as one partition of
 * the batched Cascaded codec with options.{type, num_RLEs, num_deltas, use_bp}
 * (hipcomp/cascaded.h).  The input buffer has to be aligned like its elements.
 */
#ifndef HIPCOMP_CASCADED_HPP
#define HIPCOMP_CASCADED_HPP

#include "cascaded.h"
#include "hipcompManager.hpp"

namespace hipcomp
{

struct CascadedFormatSpecHeader
{
  hipcompBatchedCascadedOpts_t options;
};

/* what stands in front of the runs of an item of decode_parquet_hybrid */
enum class ParquetHybridForm
{
  Bare,           /* the runs alone: the levels of a V2 data page (their length comes from the page table) */
  LengthPrefixed, /* a 4-byte little-endian byte count, then the runs: the levels of a V1 data page */
  WidthPrefixed   /* 1 byte bit width, then the runs to the end of the item: dictionary indices */
};

/* what an item of decode_parquet_delta writes */
enum class ParquetDeltaOutput
{
  Values, /* the decoded integers */
  Offsets /* the stream holds the lengths of a DELTA_LENGTH_BYTE_ARRAY page: n + 1 Arrow offsets, 0 first */
};

/* how the fixed-width values of an item of place_parquet_values lie in its source */
enum class ParquetValueLayout
{
  Plain,          /* value k at k * value_bytes: a PLAIN page body, or a decoded array */
  ByteStreamSplit /* byte b of value k at b * num_values + k: a BYTE_STREAM_SPLIT page body */
};

/* where the bytes of value k of an item of place_parquet_strings lie, off being its offsets */
enum class ParquetStringLayout
{
  LengthPrefixed, /* at 4 * (k + 1) + off[k]: a PLAIN BYTE_ARRAY body, off from index_parquet_dictionary */
  Packed          /* at off[k]: DELTA_LENGTH_BYTE_ARRAY, off from decode_parquet_delta(..., Offsets) */
};

struct CascadedManager : hipcompManagerBase
{
  /* device_id must be the current device */
  CascadedManager(
      const hipcompBatchedCascadedOpts_t& options = hipcompBatchedCascadedDefaultOpts, hipStream_t user_stream = 0,
      int device_id = 0);
  CascadedManager(const hipcompBatchedCascadedOpts_t& options, hipStream_t user_stream, int device_id,
                  ChecksumPolicy checksum_policy);
  ~CascadedManager() override;
  CascadedManager(const CascadedManager&) = delete;
  CascadedManager& operator=(const CascadedManager&) = delete;

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
     "Reading many ranges").  A first or a length that is not whole elements refuses the call. */
  void decompress_ranges(uint8_t* out, size_t out_bytes, const uint8_t* comp_buffer, const DecompressionConfig& decomp_config,
                         const size_t* device_first_bytes, const size_t* device_num_bytes, size_t num_ranges,
                         size_t* device_out_offsets);
  size_t get_ranges_pass_chunks() const;
  RangesStats get_ranges_stats() const;
  /* A batch of Parquet RLE / bit-packed hybrid streams -- repetition and definition levels, dictionary indices --
     decoded to UCHAR, USHORT or UINT elements (out_type); every array in device memory.  One launch on the manager's
     stream: no scratch, no synchronisation, so the arrays may be what an earlier call on the stream leaves behind
     (a definition-level call's match counts as the num_values of the index call).  Item i writes
     device_num_values[i] elements; device_consumed_bytes[i] says where the next section of the page begins;
     device_match_counts[i] counts the decoded values equal to device_match_values[i].  An item the rules refuse is
     hipcompErrorCannotDecompress with 0 consumed bytes, 0 matches and no byte of its output written; no item's
     result depends on another's.  Throws before anything is launched: more than 2^20 items, a null mandatory array,
     one match array without the other, an out_type outside the three.  The contract, rule by rule: INTEGRATION.md,
     "Parquet levels and dictionary indices in the Cascaded manager". */
  void decode_parquet_hybrid(const uint8_t* const* device_stream_ptrs, const size_t* device_stream_bytes,
                             const uint32_t* device_bit_widths, /* per item; ignored (may be null) for WidthPrefixed */
                             const size_t* device_num_values,   /* values wanted per item */
                             void* const* device_out_ptrs, const size_t* device_out_capacities, /* in elements */
                             size_t* device_consumed_bytes,                                     /* may be null */
                             const uint32_t* device_match_values, size_t* device_match_counts,  /* both null or both set */
                             hipcompStatus_t* device_statuses, size_t num_items, ParquetHybridForm form, hipcompType_t out_type);
  /* A batch of Parquet DELTA_BINARY_PACKED streams -- the values of integer and timestamp pages, or the lengths in
     front of a DELTA_LENGTH_BYTE_ARRAY page's string bytes -- decoded to INT (Parquet INT32, 32-bit wrapping sums) or
     LONGLONG (INT64, 64-bit) elements (out_type); every array in device memory.  One launch on the manager's stream:
     no scratch, no synchronisation, so device_num_values may be the match counts a decode_parquet_hybrid call on the
     stream leaves behind (the non-null count of the page's definition levels).  Values: item i writes the stream's
     total count of elements.  Offsets: it writes total + 1 running sums of the lengths, 0 first, and
     device_consumed_bytes[i] is where the string bytes begin: stream + consumed and the offsets are the Arrow string
     array.  An item the rules refuse is hipcompErrorCannotDecompress with 0 consumed bytes, a count of 0 and no byte
     of its output written; no item's result depends on another's.  Throws before anything is launched: more than
     2^20 items, a null mandatory array, an out_type outside the two, an unknown ParquetDeltaOutput.  The contract,
     rule by rule: INTEGRATION.md, "Parquet DELTA_BINARY_PACKED values and string offsets in the Cascaded manager". */
  void decode_parquet_delta(const uint8_t* const* device_stream_ptrs, const size_t* device_stream_bytes,
                            const size_t* device_num_values, /* may be null: every item decodes its header's count */
                            void* const* device_out_ptrs, const size_t* device_out_capacities, /* in elements */
                            size_t* device_value_counts,     /* may be null: the values decoded per item */
                            size_t* device_consumed_bytes,   /* may be null */
                            hipcompStatus_t* device_statuses, size_t num_items, ParquetDeltaOutput output, hipcompType_t out_type);
  /* The three calls that turn a dictionary-encoded Parquet column's decoded parts -- the dictionary page's body, the
     UINT indices and the UCHAR definition levels of decode_parquet_hybrid -- into an Arrow-shaped array: values, or
     offsets and bytes, and a validity bitmap.  Every array in device memory; each call one launch on the manager's
     stream, no scratch, no synchronisation, so the counts may be what an earlier call on the stream leaves behind
     (the levels' match counts as device_num_indices, call 1's entry counts as device_dict_entries).  An item the
     rules refuse is hipcompErrorCannotDecompress, every count it reports 0 and no byte of its outputs written; no
     item's result depends on another's.  Each throws before anything is launched: more than 2^20 items, a null
     mandatory array, a parameter outside its range.  Flat columns, one dictionary per item (many items may name
     the same one).  The contract, rule by rule: INTEGRATION.md, "Parquet dictionary entries gathered to rows in the
     Cascaded manager". */
  /* 1. The Arrow offsets of a PLAIN BYTE_ARRAY dictionary page body (len32 bytes len32 bytes ...): entries + 1
     of them, 0 first; entry k's bytes lie at dict + 4 * (k + 1) + off[k].  Refused: entries + 1 above the capacity,
     a body that ends in a length word, a length that runs past the body, a sum above 2^31 - 1. */
  void index_parquet_dictionary(const uint8_t* const* device_dict_ptrs, const size_t* device_dict_bytes,
                                const size_t* device_num_entries, /* the dictionary page's num_values */
                                int32_t* const* device_offset_ptrs, const size_t* device_offset_capacities, /* in elements */
                                size_t* device_entry_counts, /* may be null: the entries, 0 of a refused item */
                                hipcompStatus_t* device_statuses, size_t num_dicts);
  /* 2. Fixed-width entries (INT32, INT64, FLOAT, DOUBLE, INT96, FIXED_LEN_BYTE_ARRAY) of entry_bytes (1 to 64) each:
     entry k lies at dict + k * entry_bytes, at any byte address.  Dense (the three arrays of the levels null): row r
     gets dict[index[r]].  With levels: row r is valid where level[r] == max_level; the j-th valid row gets
     dict[index[j]], every other row entry_bytes zero bytes.  The validity bitmap is Arrow's, bit r & 7 of byte
     r >> 3, the unused bits 0; it may lie at any byte address.  The output lies at the alignment of the largest power
     of two that divides entry_bytes, at most 8.  Refused: rows above the capacity, dict_entries * entry_bytes above
     dict_bytes, an index at or above dict_entries, a level above max_level, valid rows that are not num_indices. */
  void gather_parquet_dictionary(const uint8_t* const* device_dict_ptrs, const size_t* device_dict_bytes,
                                 const size_t* device_dict_entries, const uint32_t* const* device_index_ptrs,
                                 const size_t* device_num_indices, const uint8_t* const* device_level_ptrs,
                                 const size_t* device_num_rows,
                                 const uint32_t* device_max_levels, /* these three: all null (dense) or all set */
                                 void* const* device_out_ptrs, const size_t* device_out_capacities, /* in entries (rows) */
                                 uint8_t* const* device_validity_ptrs, /* may be null; (rows + 7) / 8 bytes per item */
                                 hipcompStatus_t* device_statuses, size_t num_items, uint32_t entry_bytes);
  /* 3. BYTE_ARRAY entries to an Arrow string array: rows + 1 offsets, 0 first, a row that is not valid adding 0, and
     the valid rows' bytes back to back.  device_dict_offsets is what call 1 wrote and is not trusted: an entry an
     item uses needs 0 <= off[k] <= off[k + 1] and 4 * (k + 1) + off[k + 1] <= dict_bytes.  Refused besides, and
     besides what call 2 refuses of the rows: rows + 1 above the offset capacity, a byte total above the byte capacity
     or above 2^31 - 1. */
  void gather_parquet_dictionary_strings(const uint8_t* const* device_dict_ptrs, const size_t* device_dict_bytes,
                                         const size_t* device_dict_entries, const int32_t* const* device_dict_offsets,
                                         const uint32_t* const* device_index_ptrs, const size_t* device_num_indices,
                                         const uint8_t* const* device_level_ptrs, const size_t* device_num_rows,
                                         const uint32_t* device_max_levels, /* these three: all null (dense) or all set */
                                         int32_t* const* device_out_offsets, const size_t* device_offset_capacities, /* elements */
                                         uint8_t* const* device_out_bytes, const size_t* device_byte_capacities,
                                         size_t* device_out_byte_counts, /* may be null: the bytes, 0 of a refused item */
                                         uint8_t* const* device_validity_ptrs, /* may be null */
                                         hipcompStatus_t* device_statuses, size_t num_items);
  /* The three calls that put the dense values of a page that is not dictionary-encoded -- a PLAIN or BYTE_STREAM_SPLIT
     page body, or the array a decode_parquet_delta or decode_parquet_hybrid call wrote -- into their rows with the nulls
     placed: an Arrow-shaped array of values, of bits, or of offsets and bytes, and a validity bitmap.  The contract is
     the dictionary calls' above wherever it applies: every array in device memory; each call one launch on the
     manager's stream, no scratch, no synchronisation; at most 2^20 items; an item the rules refuse is
     hipcompErrorCannotDecompress, every count it reports 0 and no byte of its outputs written; no item's result depends
     on another's.  Each throws before anything is launched: more than 2^20 items, a null mandatory array, a parameter
     outside its range, one or two of the levels' three arrays without the rest, an unknown enum value.  Dense (the
     three arrays of the levels null): rows = num_values.  With levels (UCHAR): row r is valid where level[r] ==
     max_level, the j-th valid row gets value j; a level above max_level and valid rows that are not num_values refuse
     the item.  The validity bitmap is Arrow's and optional, at any byte address.  device_value_starts may be null (every
     start 0): the item's source begins start[i] bytes behind its pointer, the byte count being that of the whole buffer
     from the pointer; a start above it refuses the item (the consumed bytes of a V1 page's definition levels, or of a
     decode_parquet_delta(..., Offsets) call, go here as they are).  An item's inputs and outputs must not overlap; this
     is not checked.  The contract, rule by rule: INTEGRATION.md, "PLAIN Parquet values placed in rows in the Cascaded
     manager". */
  /* 1. Fixed-width values of value_bytes (1 to 64) each.  Plain: value k lies at src + k * value_bytes, at any byte
     address.  ByteStreamSplit: byte b of value k lies at src + b * num_values + k.  rows values are written, value_bytes
     zero bytes where the row is not valid; the output lies at the alignment of the largest power of two that divides
     value_bytes, at most 8.  Refused: rows above the capacity, num_values * value_bytes above the bytes behind the
     start, and what the levels refuse. */
  void place_parquet_values(const uint8_t* const* device_value_ptrs, const size_t* device_value_bytes,
                            const size_t* device_value_starts, /* may be null */
                            const size_t* device_num_values, const uint8_t* const* device_level_ptrs, const size_t* device_num_rows,
                            const uint32_t* device_max_levels, /* these three: all null (dense) or all set */
                            void* const* device_out_ptrs, const size_t* device_out_capacities, /* in values (rows) */
                            uint8_t* const* device_validity_ptrs, /* may be null; (rows + 7) / 8 bytes per item */
                            hipcompStatus_t* device_statuses, size_t num_items, uint32_t value_bytes, ParquetValueLayout layout);
  /* 2. PLAIN BOOLEAN: value k is bit k & 7 of byte k >> 3.  The output is an Arrow boolean array's values bitmap,
     (rows + 7) / 8 bytes at any byte address: bit r is the j-th source bit where row r is the j-th valid row, 0 where the
     row is not valid, the unused bits 0.  Refused: (num_values + 7) / 8 above the bytes behind the start, rows above
     the capacity, and what the levels refuse.  Bits behind num_values are not looked at. */
  void place_parquet_booleans(const uint8_t* const* device_value_ptrs, const size_t* device_value_bytes,
                              const size_t* device_value_starts, /* may be null */
                              const size_t* device_num_values, const uint8_t* const* device_level_ptrs, const size_t* device_num_rows,
                              const uint32_t* device_max_levels, /* these three: all null (dense) or all set */
                              uint8_t* const* device_out_ptrs, const size_t* device_out_capacities, /* in rows (bits) */
                              uint8_t* const* device_validity_ptrs, /* may be null */
                              hipcompStatus_t* device_statuses, size_t num_items);
  /* 3. BYTE_ARRAY values to an Arrow string array: rows + 1 offsets, 0 first, a row that is not valid adding 0, and the
     valid rows' bytes back to back.  device_value_offsets are num_values + 1 INT offsets, not trusted.  LengthPrefixed:
     a PLAIN body (len32 bytes len32 bytes ...) with the offsets index_parquet_dictionary writes for it; value k's
     bytes lie at body + 4 * (k + 1) + off[k].  Packed: DELTA_LENGTH_BYTE_ARRAY with the offsets of
     decode_parquet_delta(..., Offsets); value k's bytes lie at body + off[k].  Every value needs 0 <= off[k] <=
     off[k + 1] and its end -- 4 * (k + 1) + off[k + 1], or off[k + 1] -- at most the bytes behind the start.  Refused
     besides: rows + 1 above the offset capacity, a byte total above the byte capacity or above 2^31 - 1, and what the
     levels refuse.  num_values may be the counts an earlier call leaves: a refused earlier item has 0 and refuses
     every item with a valid row. */
  void place_parquet_strings(const uint8_t* const* device_body_ptrs, const size_t* device_body_bytes,
                             const size_t* device_value_starts, /* may be null */
                             const int32_t* const* device_value_offsets, const size_t* device_num_values,
                             const uint8_t* const* device_level_ptrs, const size_t* device_num_rows,
                             const uint32_t* device_max_levels, /* these three: all null (dense) or all set */
                             int32_t* const* device_out_offsets, const size_t* device_offset_capacities, /* elements */
                             uint8_t* const* device_out_bytes, const size_t* device_byte_capacities,
                             size_t* device_out_byte_counts, /* may be null: the bytes, 0 of a refused item */
                             uint8_t* const* device_validity_ptrs, /* may be null */
                             hipcompStatus_t* device_statuses, size_t num_items, ParquetStringLayout layout);

private:
  struct Impl;
  std::unique_ptr<Impl> impl;
};

} // namespace hipcomp

#endif
