// parquet_plain_plan.hpp -- the arithmetic of the three calls that put the dense values of a Parquet page that is not
// dictionary-encoded into their rows, the nulls placed (hipcomp/cascaded.hpp: place_parquet_values,
// place_parquet_booleans and place_parquet_strings; the kernels: parquet_plain_kernels.hip): where a value's bytes lie
// under each layout, the rules of a start, of a source that has to hold its values and of an untrusted offset, the
// rules that refuse an item, and each call's whole work on one thread.  INTEGRATION.md, "PLAIN Parquet values placed in
// rows in the Cascaded manager", has the contract.
//
// The rules these calls share with the dictionary calls -- a row's level, the shape of the rows against a capacity, the
// validity bitmap, the output's alignment, the largest offset, the byte total -- are parquet_dict_plan.hpp's, used
// from there and not restated.
//
// constexpr functions over standard headers only, no HIP, no state.  The host and the kernels include this one copy.
// tests/test_parquet_plain_plan_cpu.py compiles it with g++ alone under the address and undefined-behaviour sanitizers
// (tests/parquet_plain_plan_driver.cpp prints it) and compares it with tests/parquet_plaingen.py.
#pragma once

#include <cstddef>
#include <cstdint>

#include "parquet_dict_plan.hpp"

namespace hcamd {
namespace pqv {

using pqg::bitmap_bytes;
using pqg::kMaxItems;
using pqg::kMaxOffset;
using pqg::kStep;
using pqg::level_refused;
using pqg::level_valid;
using pqg::output_alignment;
using pqg::row_valid;
using pqg::Rows; // (its indices stay null here: the j-th valid row gets value j)
using pqg::Shape;
using pqg::shape_of;
using pqg::store_validity;
using pqg::Strings;
using pqg::total_refused;

constexpr uint32_t kMaxValueBytes = 64; // of a fixed-width value

// hipcomp::ParquetValueLayout and hipcomp::ParquetStringLayout (hlif.hip asserts it)
enum ValueLayout : uint32_t { kPlain = 0, kByteStreamSplit = 1 };
enum StringLayout : uint32_t { kLengthPrefixed = 0, kPacked = 1 };
constexpr bool value_layout_known(uint32_t layout) { return layout <= kByteStreamSplit; }
constexpr bool string_layout_known(uint32_t layout) { return layout <= kPacked; }

// ---- 1. the source ------------------------------------------------------------------------------------------------------
// An item's source begins `start` bytes behind its pointer; `bytes` is the whole buffer's.  Refused: a start above it.
constexpr bool start_refused(uint64_t start, uint64_t bytes) { return start > bytes; }
// Refused: num_values * value_bytes above the bytes behind the start (value_bytes >= 1)
constexpr bool values_fit(uint64_t num_values, uint32_t value_bytes, uint64_t behind) { return num_values <= behind / value_bytes; }
// byte b of value k, from the start
constexpr uint64_t value_byte_at(uint32_t layout, uint64_t k, uint32_t b, uint32_t value_bytes, uint64_t num_values)
{
  return layout == kByteStreamSplit ? (uint64_t)b * num_values + k : k * value_bytes + b;
}
// PLAIN BOOLEAN: bit k & 7 of byte k >> 3.  Refused: (num_values + 7) / 8 above the bytes behind the start.
constexpr bool bits_fit(uint64_t num_values, uint64_t behind) { return num_values / 8 + (num_values % 8 ? 1 : 0) <= behind; }

// ---- 2. an untrusted offset of a BYTE_ARRAY value -------------------------------------------------------------------------
// Value k through offsets someone else wrote: a = off[k], b = off[k + 1].  Refused: a < 0, a > b, the value's end above
// the bytes behind the start -- 4 * (k + 1) + b under kLengthPrefixed (the dictionary calls' rule as it is), b under
// kPacked.  An accepted value's bytes, [string_at(k, a), string_at(k, a) + b - a), lie in the source.
constexpr bool string_refused(uint32_t layout, uint64_t k, int32_t a, int32_t b, uint64_t behind)
{
  return layout == kLengthPrefixed ? pqg::entry_refused(k, a, b, behind) : (a < 0 || a > b || (uint64_t)b > behind);
}
constexpr uint64_t string_at(uint32_t layout, uint64_t k, uint64_t a) { return layout == kLengthPrefixed ? pqg::entry_at(k, a) : a; }

// ---- 3. the rows ----------------------------------------------------------------------------------------------------------
// The levels of the first walk: none above the maximum, and the valid rows are the values.  Dense: nothing to ask.
constexpr bool levels_accepted(const Rows& r, uint64_t rows)
{
  bool ok = true;
  if (r.levels) {
    uint64_t valid = 0;
    for (uint64_t i = 0; ok && i < rows; ++i) {
      ok = !level_refused(r.levels[i], r.max_level);
      valid += level_valid(r.levels[i], r.max_level) ? 1 : 0;
    }
    ok = ok && valid == r.num_indices;
  }
  return ok;
}
constexpr Rows rows_of(uint64_t num_values, const uint8_t* levels, uint64_t num_rows, uint32_t max_level)
{
  return Rows{nullptr, num_values, levels, num_rows, max_level};
}

// ---- each call's whole work on one thread ----------------------------------------------------------------------------------
// An item is walked without storing, then worked, so that a refused item has nothing written.  What the host path of
// a measurement runs, and what the tests hold the kernels to.  `r` is rows_of(...); levels == nullptr: dense.

// place_parquet_values: rows values of value_bytes into out[0, capacity * value_bytes); validity may be null
constexpr bool place_values_item(const uint8_t* src, uint64_t src_bytes, uint64_t start, const Rows& r, uint64_t capacity,
                                 uint32_t value_bytes, uint32_t layout, uint8_t* out, uint8_t* validity)
{
  const Shape s = shape_of(r.levels != nullptr, r.num_indices, r.num_rows, capacity, 0);
  const bool ok = s.ok && !start_refused(start, src_bytes) && values_fit(r.num_indices, value_bytes, src_bytes - start)
                  && levels_accepted(r, s.rows);
  if (ok) {
    uint64_t j = 0;
    for (uint64_t i = 0; i < s.rows; ++i) {
      const bool valid = row_valid(r, i);
      for (uint32_t b = 0; b < value_bytes; ++b)
        out[i * value_bytes + b] = valid ? src[start + value_byte_at(layout, j, b, value_bytes, r.num_indices)] : (uint8_t)0;
      j += valid ? 1 : 0;
    }
    if (validity)
      store_validity(r, s.rows, validity);
  }
  return ok;
}

// place_parquet_booleans: rows bits into out[0, (capacity + 7) / 8): (rows + 7) / 8 bytes are written
constexpr bool place_booleans_item(const uint8_t* src, uint64_t src_bytes, uint64_t start, const Rows& r, uint64_t capacity, uint8_t* out,
                                   uint8_t* validity)
{
  const Shape s = shape_of(r.levels != nullptr, r.num_indices, r.num_rows, capacity, 0);
  const bool ok = s.ok && !start_refused(start, src_bytes) && bits_fit(r.num_indices, src_bytes - start) && levels_accepted(r, s.rows);
  if (ok) {
    uint64_t j = 0;
    for (uint64_t at = 0; at < bitmap_bytes(s.rows); ++at) {
      uint32_t bits = 0;
      for (uint64_t i = 8 * at; i < s.rows && i < 8 * at + 8; ++i) {
        if (row_valid(r, i)) {
          bits |= ((uint32_t)(src[start + (j >> 3)] >> (j & 7)) & 1u) << (i & 7);
          ++j;
        }
      }
      out[at] = (uint8_t)bits;
    }
    if (validity)
      store_validity(r, s.rows, validity);
  }
  return ok;
}

// place_parquet_strings: rows + 1 offsets into out_offsets[0, offset_capacity) and the values' bytes, back to back,
// into out_bytes[0, byte_capacity); `offsets` has num_values + 1 entries and is not trusted.  No byte of the body is
// read before the item is accepted.
constexpr Strings place_strings_item(const uint8_t* body, uint64_t body_bytes, uint64_t start, const int32_t* offsets, const Rows& r,
                                     uint32_t layout, uint64_t offset_capacity, uint64_t byte_capacity, int32_t* out_offsets,
                                     uint8_t* out_bytes, uint8_t* validity)
{
  Strings v;
  const Shape s = shape_of(r.levels != nullptr, r.num_indices, r.num_rows, offset_capacity, 1);
  bool ok = s.ok && !start_refused(start, body_bytes) && levels_accepted(r, s.rows);
  uint64_t total = 0;
  for (uint64_t k = 0; ok && k < r.num_indices; ++k) {
    ok = !string_refused(layout, k, offsets[k], offsets[k + 1], body_bytes - start);
    if (ok) {
      total += (uint64_t)(uint32_t)(offsets[k + 1] - offsets[k]);
      ok = !total_refused(total, byte_capacity);
    }
  }
  if (ok) {
    uint64_t j = 0, at = 0;
    out_offsets[0] = 0;
    for (uint64_t i = 0; i < s.rows; ++i) {
      if (row_valid(r, i)) {
        const uint64_t length = (uint64_t)(offsets[j + 1] - offsets[j]);
        const uint8_t* const from = body + start + string_at(layout, j, (uint64_t)offsets[j]);
        for (uint64_t b = 0; b < length; ++b)
          out_bytes[at + b] = from[b];
        at += length;
        ++j;
      }
      out_offsets[i + 1] = (int32_t)at;
    }
    if (validity)
      store_validity(r, s.rows, validity);
    v.ok = true;
    v.bytes = total;
  }
  return v;
}

} // namespace pqv
} // namespace hcamd
