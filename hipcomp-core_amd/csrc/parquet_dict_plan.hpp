// parquet_dict_plan.hpp -- the arithmetic of the three calls that turn a Parquet dictionary-encoded column's decoded
// parts into rows (hipcomp/cascaded.hpp: index_parquet_dictionary, gather_parquet_dictionary and
// gather_parquet_dictionary_strings; the kernels: parquet_dict_kernels.hip): the chain of a PLAIN BYTE_ARRAY
// dictionary page's lengths, the place of a fixed-width entry, the rules of a row's level and index, the rules of an
// untrusted dictionary offset, the validity bitmap, the rules that refuse an item, and each call's whole work on one
// thread.  INTEGRATION.md, "Parquet dictionary entries gathered to rows in the Cascaded manager", has the contract.
//
// constexpr functions over standard headers only, no HIP, no state.  The chain is templated over the byte source:
// `Src` has `uint32_t at(uint64_t pos)`, asked only for pos inside the item.  The host and the kernels include this one
// copy.  tests/test_parquet_dict_plan_cpu.py compiles it with g++ alone under the address and undefined-behaviour
// sanitizers (tests/parquet_dict_plan_driver.cpp prints it) and compares it with tests/parquet_dictgen.py.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace pqg {

constexpr uint64_t kMaxItems = uint64_t(1) << 20;
constexpr uint32_t kStep = 64;          // the rows of a gathering step: a wavefront's lanes
constexpr uint32_t kMaxEntryBytes = 64; // of a fixed-width entry
constexpr uint64_t kMaxOffset = 0x7FFFFFFFu; // the largest Arrow offset of 32 bits

// ---- 1. the chain of a BYTE_ARRAY dictionary page: len32 bytes len32 bytes ... ---------------------------------------
// The length word of entry k stands at 4 * k + off[k], its bytes at 4 * (k + 1) + off[k].
constexpr uint64_t length_word_at(uint64_t k, uint64_t off) { return 4 * k + off; }
constexpr uint64_t entry_at(uint64_t k, uint64_t off) { return 4 * (k + 1) + off; }
// entries + 1 offsets have to fit
constexpr bool offsets_fit(uint64_t entries, uint64_t capacity) { return entries < capacity; }

template <class Src>
constexpr uint32_t read_le32(Src& s, uint64_t pos)
{
  return (s.at(pos) & 0xFFu) | ((s.at(pos + 1) & 0xFFu) << 8) | ((s.at(pos + 2) & 0xFFu) << 16) | ((s.at(pos + 3) & 0xFFu) << 24);
}
// `Sink` has `void take(uint64_t k, uint64_t off)`: off[k + 1] is `off`.  Refused: the body ending inside a length
// word; a length that runs past the body (one of 2^31 or more among them: the sum rule below bounds the body that
// could hold it); a sum above 2^31 - 1.  Nothing behind the last entry is looked at.  One exit.
struct NoSink
{
  constexpr void take(uint64_t, uint64_t) {}
};
template <class Src, class Sink>
constexpr bool walk_chain(Src& s, uint64_t n, uint64_t entries, Sink& sink)
{
  bool ok = true;
  uint64_t off = 0;
  for (uint64_t k = 0; ok && k < entries; ++k) {
    const uint64_t pos = length_word_at(k, off); // (<= n: every step below keeps it so)
    if (n - pos < 4) {
      ok = false;
    } else {
      const uint64_t length = read_le32(s, pos);
      if (length > n - pos - 4 || off + length > kMaxOffset) {
        ok = false;
      } else {
        off += length;
        sink.take(k, off);
      }
    }
  }
  return ok;
}

// ---- 2. the rows ---------------------------------------------------------------------------------------------------------
// What the call's own arrays say of an item, before a level or an index is read.
struct Shape
{
  bool ok = false;
  uint64_t rows = 0;
};
// Refused: rows (+ `extra`: the strings' offsets are one more) above the capacity.
constexpr Shape shape_of(bool has_levels, uint64_t num_indices, uint64_t num_rows, uint64_t capacity, uint64_t extra)
{
  Shape s;
  s.rows = has_levels ? num_rows : num_indices;
  s.ok = s.rows <= capacity && capacity - s.rows >= extra;
  return s;
}
// Refused: dict_entries * entry_bytes above dict_bytes (entry_bytes >= 1)
constexpr bool dictionary_fits(uint64_t dict_entries, uint64_t dict_bytes, uint32_t entry_bytes)
{
  return dict_entries <= dict_bytes / entry_bytes;
}
// a row's level: refused above the maximum, valid at it
constexpr bool level_refused(uint32_t level, uint32_t max_level) { return level > max_level; }
constexpr bool level_valid(uint32_t level, uint32_t max_level) { return level == max_level; }
constexpr bool index_refused(uint32_t index, uint64_t dict_entries) { return (uint64_t)index >= dict_entries; }
// the bitmap: bit r & 7 of byte r >> 3
constexpr uint64_t bitmap_bytes(uint64_t rows) { return (rows + 7) / 8; }
// the alignment a fixed-width output has: the largest power of two that divides entry_bytes, at most 8
constexpr uint32_t output_alignment(uint32_t entry_bytes)
{
  return (entry_bytes & 1) ? 1 : (entry_bytes & 2) ? 2 : (entry_bytes & 4) ? 4 : 8;
}

// ---- 3. an untrusted dictionary offset ------------------------------------------------------------------------------------
// Entry k of a BYTE_ARRAY dictionary through offsets someone else wrote: a = off[k], b = off[k + 1].  Refused: a > b, a
// < 0, 4 * (k + 1) + b above dict_bytes.  An accepted entry's bytes, [entry_at(k, a), entry_at(k, a) + b - a), lie in
// the dictionary.
constexpr bool entry_refused(uint64_t k, int32_t a, int32_t b, uint64_t dict_bytes)
{
  return a < 0 || a > b || 4 * (k + 1) > dict_bytes || (uint64_t)b > dict_bytes - 4 * (k + 1);
}
// Refused: a byte total above the capacity or above 2^31 - 1
constexpr bool total_refused(uint64_t total, uint64_t byte_capacity) { return total > byte_capacity || total > kMaxOffset; }

// ---- each call's whole work on one thread ----------------------------------------------------------------------------------
// An item is walked without storing, then worked, so that a refused item has nothing written.  What the host path of
// a measurement runs, and what the tests hold the kernels to.
struct Bytes
{
  const uint8_t* p;
  constexpr uint32_t at(uint64_t pos) const { return p[pos]; }
};
struct StoreSink
{
  int32_t* out;
  constexpr void take(uint64_t k, uint64_t off) { out[k + 1] = (int32_t)off; }
};
// index_parquet_dictionary: entries + 1 offsets into off[0, capacity); true: accepted
constexpr bool index_item(const uint8_t* dict, uint64_t n, uint64_t entries, uint64_t capacity, int32_t* off)
{
  Bytes src{dict};
  NoSink none;
  const bool ok = offsets_fit(entries, capacity) && walk_chain(src, n, entries, none);
  if (ok) {
    StoreSink sink{off};
    off[0] = 0;
    (void)walk_chain(src, n, entries, sink);
  }
  return ok;
}

// the inputs of a gathering item; levels == nullptr: dense
struct Rows
{
  const uint32_t* indices;
  uint64_t num_indices;
  const uint8_t* levels;
  uint64_t num_rows;
  uint32_t max_level;
};
// The first walk of both gathers: every level, the count of the valid rows, every index.  `Entry` has `bool
// refused(uint32_t index)`, asked for an index below dict_entries.
template <class Entry>
constexpr bool rows_accepted(const Rows& r, uint64_t rows, uint64_t dict_entries, Entry& entry)
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
  for (uint64_t j = 0; ok && j < r.num_indices; ++j)
    ok = !index_refused(r.indices[j], dict_entries) && !entry.refused(r.indices[j]);
  return ok;
}
constexpr bool row_valid(const Rows& r, uint64_t i) { return !r.levels || level_valid(r.levels[i], r.max_level); }
constexpr void store_validity(const Rows& r, uint64_t rows, uint8_t* validity)
{
  for (uint64_t b = 0; b < bitmap_bytes(rows); ++b) {
    uint32_t bits = 0;
    for (uint64_t i = 8 * b; i < rows && i < 8 * b + 8; ++i)
      bits |= (row_valid(r, i) ? 1u : 0u) << (i & 7);
    validity[b] = (uint8_t)bits;
  }
}

struct AnyEntry
{
  constexpr bool refused(uint32_t) const { return false; }
};
// gather_parquet_dictionary: rows entries of entry_bytes into out[0, capacity * entry_bytes); validity may be null
constexpr bool gather_item(const uint8_t* dict, uint64_t dict_bytes, uint64_t dict_entries, const Rows& r, uint64_t capacity,
                           uint32_t entry_bytes, uint8_t* out, uint8_t* validity)
{
  const Shape s = shape_of(r.levels != nullptr, r.num_indices, r.num_rows, capacity, 0);
  AnyEntry any;
  const bool ok = s.ok && dictionary_fits(dict_entries, dict_bytes, entry_bytes) && rows_accepted(r, s.rows, dict_entries, any);
  if (ok) {
    uint64_t j = 0;
    for (uint64_t i = 0; i < s.rows; ++i) {
      const bool valid = row_valid(r, i);
      const uint8_t* const from = dict + (valid ? (uint64_t)r.indices[j] * entry_bytes : 0);
      for (uint32_t b = 0; b < entry_bytes; ++b)
        out[i * entry_bytes + b] = valid ? from[b] : (uint8_t)0;
      j += valid ? 1 : 0;
    }
    if (validity)
      store_validity(r, s.rows, validity);
  }
  return ok;
}

// what the strings' call says of an item; a refused one has 0
struct Strings
{
  bool ok = false;
  uint64_t bytes = 0;
};
struct OffsetEntry
{
  const int32_t* off;
  uint64_t dict_bytes;
  constexpr bool refused(uint32_t k) const { return entry_refused(k, off[k], off[(uint64_t)k + 1], dict_bytes); }
};
// gather_parquet_dictionary_strings: rows + 1 offsets into out_offsets[0, offset_capacity) and the entries' bytes, back
// to back, into out_bytes[0, byte_capacity)
constexpr Strings gather_strings_item(const uint8_t* dict, uint64_t dict_bytes, uint64_t dict_entries, const int32_t* dict_offsets,
                                      const Rows& r, uint64_t offset_capacity, uint64_t byte_capacity, int32_t* out_offsets,
                                      uint8_t* out_bytes, uint8_t* validity)
{
  Strings v;
  const Shape s = shape_of(r.levels != nullptr, r.num_indices, r.num_rows, offset_capacity, 1);
  OffsetEntry entry{dict_offsets, dict_bytes};
  bool ok = s.ok && rows_accepted(r, s.rows, dict_entries, entry);
  uint64_t total = 0;
  for (uint64_t j = 0; ok && j < r.num_indices; ++j) {
    const uint64_t k = r.indices[j];
    total += (uint64_t)(dict_offsets[k + 1] - dict_offsets[k]);
    ok = !total_refused(total, byte_capacity);
  }
  if (ok) {
    uint64_t j = 0, at = 0;
    out_offsets[0] = 0;
    for (uint64_t i = 0; i < s.rows; ++i) {
      if (row_valid(r, i)) {
        const uint64_t k = r.indices[j++];
        const uint64_t length = (uint64_t)(dict_offsets[k + 1] - dict_offsets[k]);
        const uint8_t* const from = dict + entry_at(k, (uint64_t)dict_offsets[k]);
        for (uint64_t b = 0; b < length; ++b)
          out_bytes[at + b] = from[b];
        at += length;
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

} // namespace pqg
} // namespace hcamd
