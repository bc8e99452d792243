// parquet_pages_plan.hpp -- the arithmetic of a read of the pages of a batch of Parquet column chunks in one call
// (hipcomp/snappy.hpp, decompress_parquet_pages and get_parquet_pages_sizes; the kernels: parquet_pages_kernels.hip):
// a reader of Thrift compact-protocol structs, the rules that turn the bytes at an offset of a column chunk into a
// page record or a refusal, the walk along a chunk's page chain, how the scratch space is laid out and how the listed
// pages of all items -- numbered through the batch in item order -- fall into passes.
//
// constexpr functions over standard headers only, no HIP, no state, templated over the byte source: `Src` has
// `uint32_t at(uint64_t pos)`, asked only for pos inside the chunk.  The host and the kernels include this one copy.
// tests/test_parquet_pages_plan_cpu.py compiles it with g++ alone under the address and undefined-behaviour
// sanitizers (tests/parquet_pages_plan_driver.cpp prints it) and compares it with tests/parquet_pagegen.py.
// The codec of the compressed parts is not this file's business: a part is stored or it is compressed.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace pqp {

constexpr uint64_t kMaxItems = uint64_t(1) << 20;
constexpr uint32_t kMaxDepth = 8; // containers open at once, the page header itself being the first

// ---- the page record (hipcomp/snappy.hpp, ParquetPageInfo: the same fields in the same order) -------------------
struct Page
{
  uint64_t header_offset = 0, body_offset = 0;
  uint64_t out_offset = 0;
  uint32_t compressed_page_size = 0, uncompressed_page_size = 0;
  uint32_t kind = 0;
  uint32_t num_values = 0, encoding = 0;
  uint32_t rep_levels_bytes = 0, def_levels_bytes = 0;
  uint32_t num_nulls = 0, num_rows = 0;
  uint32_t crc = 0, flags = 0;
  uint32_t pad = 0;
};
enum Kind : uint32_t { kDataPage = 0, kIndexPage = 1, kDictionaryPage = 2, kDataPageV2 = 3 };
enum Flags : uint32_t { kHasCrc = 1, kValuesStored = 2 };
enum Codec : uint32_t { kStoredColumn = 0, kCompressedColumn = 1 };

// The parts of a listed page.  The levels of a V2 page lie stored in front of its values; where the values are
// stored too, the body is one stored part.
constexpr uint64_t levels_bytes(const Page& p) { return (uint64_t)p.rep_levels_bytes + p.def_levels_bytes; }
constexpr uint64_t stored_bytes(const Page& p) { return (p.flags & kValuesStored) ? p.compressed_page_size : levels_bytes(p); }
// the compressed part [body_offset + levels, body_offset + compressed_page_size) decodes to this many bytes behind
// the levels; 0: nothing is decoded
constexpr uint64_t decoded_bytes(const Page& p)
{
  return (p.flags & kValuesStored) ? 0 : p.uncompressed_page_size - levels_bytes(p);
}
constexpr uint64_t compressed_bytes(const Page& p)
{
  return (p.flags & kValuesStored) ? 0 : p.compressed_page_size - levels_bytes(p);
}

// ---- Thrift compact protocol --------------------------------------------------------------------------------
// A failed read clears `ok`, returns 0 and leaves the position where it is; every loop below ends on !ok.
enum Wire : uint32_t {
  kStop = 0, kTrue = 1, kFalse = 2, kByte = 3, kI16 = 4, kI32 = 5, kI64 = 6, kDouble = 7, kBinary = 8, kList = 9, kSet = 10,
  kMap = 11, kStruct = 12
};

template <class Src>
constexpr uint32_t read_byte(Src& s, uint64_t& pos, uint64_t end, bool& ok)
{
  if (!ok || pos >= end) {
    ok = false;
    return 0;
  }
  return s.at(pos++) & 0xFFu;
}
constexpr void skip_bytes(uint64_t& pos, uint64_t end, uint64_t n, bool& ok)
{
  if (!ok || n > end - pos)
    ok = false;
  else
    pos += n;
}
// a varint of at most `most` bytes (5: i16 and i32, sizes; 10: i64)
template <class Src>
constexpr uint64_t read_varint(Src& s, uint64_t& pos, uint64_t end, uint32_t most, bool& ok)
{
  uint64_t v = 0;
  uint32_t n = 0;
  bool more = true;
  while (more && ok) {
    if (n == most) {
      ok = false;
    } else {
      const uint32_t b = read_byte(s, pos, end, ok);
      v |= (uint64_t)(b & 0x7Fu) << (7 * n);
      ++n;
      more = (b & 0x80u) != 0;
    }
  }
  return ok ? v : 0;
}
// an i32: the low 32 bits of the varint, zigzag
template <class Src>
constexpr int32_t read_i32(Src& s, uint64_t& pos, uint64_t end, bool& ok)
{
  const uint32_t u = (uint32_t)read_varint(s, pos, end, 5, ok);
  return (int32_t)((u >> 1) ^ (0u - (u & 1u)));
}
// a size (binary, list, set, map): the low 32 bits of the varint; one with the top bit set is negative: refused
template <class Src>
constexpr uint32_t read_size(Src& s, uint64_t& pos, uint64_t end, bool& ok)
{
  const uint32_t u = (uint32_t)read_varint(s, pos, end, 5, ok);
  if (u >> 31)
    ok = false;
  return ok ? u : 0;
}
// A field header: false at the stop byte or on !ok.  The id comes by delta or, delta 0, as a zigzag i16 (kept in 32
// unsigned bits: an id that fits no i16 names no field anyone wants).
template <class Src>
constexpr bool read_field(Src& s, uint64_t& pos, uint64_t end, uint32_t& id, uint32_t& type, bool& ok)
{
  const uint32_t h = read_byte(s, pos, end, ok);
  if (!ok || h == 0)
    return false;
  type = h & 15u;
  if ((h >> 4) == 0)
    id = (uint32_t)read_i32(s, pos, end, ok);
  else
    id += h >> 4;
  if (type == kStop || type > kStruct)
    ok = false;
  return ok;
}

// The open containers of a skip: a word each.  Bits 0-1 what it is, 4-7 and 8-11 the element types (a map's key
// and value), bit 12 set where a map's value comes next, 32-63 the elements (a map's pairs) still to come.
// (get and set by a loop over constant indices: in a kernel the words stay in registers.)
struct Open
{
  uint64_t w[kMaxDepth] = {};
};
constexpr uint64_t open_get(const Open& o, uint32_t i)
{
  uint64_t v = 0;
  for (uint32_t k = 0; k < kMaxDepth; ++k)
    if (k == i)
      v = o.w[k];
  return v;
}
constexpr void open_set(Open& o, uint32_t i, uint64_t v)
{
  for (uint32_t k = 0; k < kMaxDepth; ++k)
    if (k == i)
      o.w[k] = v;
}
constexpr uint64_t kOpenStruct = 0, kOpenList = 1, kOpenMap = 2;
// bytes of an element of a list, set or map with this type where they are the same for every element, else 0
constexpr uint32_t element_bytes(uint32_t t) { return t == kTrue || t == kFalse || t == kByte ? 1u : t == kDouble ? 8u : 0u; }

// Steps over a value of wire type `type`, a field's value (a bool then has no bytes) or an element (one byte);
// `depth` containers are open around it.  Binaries and lists of fixed-size elements are stepped over by arithmetic.
template <class Src>
constexpr void skip_value(Src& s, uint64_t& pos, uint64_t end, uint32_t type, bool field, uint32_t depth, bool& ok)
{
  Open open;
  uint32_t sp = 0, t = type;
  bool have = true;
  while (have && ok) {
    if (t == kStop || t > kStruct) {
      ok = false;
    } else if (t == kTrue || t == kFalse) {
      skip_bytes(pos, end, field ? 0 : 1, ok);
    } else if (t == kByte) {
      skip_bytes(pos, end, 1, ok);
    } else if (t == kI16 || t == kI32) {
      (void)read_varint(s, pos, end, 5, ok);
    } else if (t == kI64) {
      (void)read_varint(s, pos, end, 10, ok);
    } else if (t == kDouble) {
      skip_bytes(pos, end, 8, ok);
    } else if (t == kBinary) {
      const uint32_t n = read_size(s, pos, end, ok);
      skip_bytes(pos, end, n, ok);
    } else if (depth + sp >= kMaxDepth) {
      ok = false;
    } else if (t == kStruct) {
      open_set(open, sp++, kOpenStruct);
    } else if (t == kList || t == kSet) {
      const uint32_t h = read_byte(s, pos, end, ok);
      const uint32_t et = h & 15u;
      uint32_t n = h >> 4;
      if (n == 15)
        n = read_size(s, pos, end, ok);
      if (et == kStop || et > kStruct)
        ok = false;
      if (element_bytes(et))
        skip_bytes(pos, end, (uint64_t)n * element_bytes(et), ok);
      else if (ok)
        open_set(open, sp++, kOpenList | ((uint64_t)et << 4) | ((uint64_t)n << 32));
    } else { // kMap
      const uint32_t n = read_size(s, pos, end, ok);
      if (ok && n != 0) {
        const uint32_t kv = read_byte(s, pos, end, ok);
        const uint32_t kt = kv >> 4, vt = kv & 15u;
        if (kt == kStop || kt > kStruct || vt == kStop || vt > kStruct)
          ok = false;
        if (ok)
          open_set(open, sp++, kOpenMap | ((uint64_t)kt << 4) | ((uint64_t)vt << 8) | ((uint64_t)n << 32));
      }
    }
    // the next value: from the innermost open container that still has one
    have = false;
    while (!have && sp > 0 && ok) {
      const uint64_t f = open_get(open, sp - 1);
      const uint64_t what = f & 3u, left = f >> 32;
      if (what == kOpenStruct) {
        uint32_t id = 0, ft = 0;
        if (read_field(s, pos, end, id, ft, ok)) {
          t = ft;
          field = true;
          have = true;
        } else {
          --sp; // (the stop byte, or !ok)
        }
      } else if (left == 0) {
        --sp;
      } else if (what == kOpenList) {
        open_set(open, sp - 1, f - (uint64_t(1) << 32));
        t = (uint32_t)(f >> 4) & 15u;
        field = false;
        have = true;
      } else if (!(f & (1u << 12))) { // a map's key
        open_set(open, sp - 1, f | (1u << 12));
        t = (uint32_t)(f >> 4) & 15u;
        field = false;
        have = true;
      } else { // a map's value
        open_set(open, sp - 1, (f & ~(uint64_t)(1u << 12)) - (uint64_t(1) << 32));
        t = (uint32_t)(f >> 8) & 15u;
        field = false;
        have = true;
      }
    }
  }
}

// The i32 fields 1..7 of a struct and its bool field 7; everything else in it is stepped over.
struct Ints
{
  int32_t v[8] = {};
  bool flag7 = true; // (DataPageHeaderV2.is_compressed: true where the field is missing)
  bool present = false;
};
constexpr int32_t ints_get(const Ints& a, uint32_t i)
{
  int32_t v = 0;
  for (uint32_t k = 1; k < 8; ++k)
    if (k == i)
      v = a.v[k];
  return v;
}
template <class Src>
constexpr Ints read_ints(Src& s, uint64_t& pos, uint64_t end, uint32_t depth, bool& ok)
{
  Ints a;
  a.present = true;
  uint32_t id = 0, type = 0;
  while (read_field(s, pos, end, id, type, ok)) {
    if (type == kI32 && id >= 1 && id <= 7) {
      const int32_t v = read_i32(s, pos, end, ok);
      for (uint32_t k = 1; k < 8; ++k)
        if (k == id)
          a.v[k] = v;
    } else if ((type == kTrue || type == kFalse) && id == 7) {
      a.flag7 = type == kTrue;
    } else {
      skip_value(s, pos, end, type, true, depth, ok);
    }
  }
  return a;
}

// ---- the page rules -----------------------------------------------------------------------------------------
enum Verdict : uint32_t { kListed = 0, kSteppedOver = 1, kRefused = 2 };
struct Parsed
{
  Page page;
  uint64_t next = 0; // where the page behind this one starts
  uint32_t verdict = kRefused;
};
// A wanted field counts where it has the wire type the format gives it; with another it is stepped over like an
// unknown one (and is then missing).  A field that comes twice: the last one stands.
template <class Src>
constexpr Parsed parse_page(Src& s, uint64_t at, uint64_t end, uint32_t codec)
{
  Parsed r;
  bool ok = true;
  uint64_t pos = at;
  uint32_t id = 0, type = 0, have = 0;
  int32_t kind = 0, usize = 0, csize = 0, crc = 0;
  Ints data, dict, v2;
  while (read_field(s, pos, end, id, type, ok)) {
    if (type == kI32 && id >= 1 && id <= 4) {
      const int32_t v = read_i32(s, pos, end, ok);
      have |= 1u << id;
      kind = id == 1 ? v : kind;
      usize = id == 2 ? v : usize;
      csize = id == 3 ? v : csize;
      crc = id == 4 ? v : crc;
    } else if (type == kStruct && (id == 5 || id == 7 || id == 8)) {
      const Ints a = read_ints(s, pos, end, 2, ok); // (kMaxDepth >= 2: the struct itself may be open)
      if (id == 5)
        data = a;
      else if (id == 7)
        dict = a;
      else
        v2 = a;
    } else {
      skip_value(s, pos, end, type, true, 1, ok);
    }
  }
  if (!ok || (have & 0xEu) != 0xEu || usize < 0 || csize < 0)
    return r;
  if ((uint64_t)csize > end - pos)
    return r;
  Page& p = r.page;
  p.header_offset = at;
  p.body_offset = pos;
  p.compressed_page_size = (uint32_t)csize;
  p.uncompressed_page_size = (uint32_t)usize;
  p.kind = (uint32_t)kind;
  r.next = pos + (uint64_t)csize;
  if (p.kind == kIndexPage || p.kind > kDataPageV2) {
    r.verdict = kSteppedOver;
    return r;
  }
  const Ints& mine = p.kind == kDataPage ? data : p.kind == kDictionaryPage ? dict : v2;
  if (!mine.present)
    return r;
  bool stored = codec == kStoredColumn;
  int32_t num_values = ints_get(mine, 1), encoding = 0, rep = 0, def = 0, nulls = 0, rows = 0;
  if (p.kind == kDataPageV2) {
    nulls = ints_get(mine, 2);
    rows = ints_get(mine, 3);
    encoding = ints_get(mine, 4);
    def = ints_get(mine, 5);
    rep = ints_get(mine, 6);
    stored = stored || !mine.flag7;
  } else {
    encoding = ints_get(mine, 2);
  }
  if (num_values < 0 || nulls < 0 || rows < 0 || rep < 0 || def < 0)
    return r;
  const uint64_t levels = (uint64_t)rep + (uint64_t)def;
  if (levels > (uint64_t)csize || levels > (uint64_t)usize)
    return r;
  if (stored && csize != usize)
    return r;
  p.num_values = (uint32_t)num_values;
  p.encoding = (uint32_t)encoding;
  p.rep_levels_bytes = (uint32_t)rep;
  p.def_levels_bytes = (uint32_t)def;
  p.num_nulls = (uint32_t)nulls;
  p.num_rows = (uint32_t)rows;
  p.crc = (have & (1u << 4)) ? (uint32_t)crc : 0;
  p.flags = ((have & (1u << 4)) ? kHasCrc : 0u) | (stored ? kValuesStored : 0u);
  r.verdict = kListed;
  return r;
}

// ---- the walk -----------------------------------------------------------------------------------------------
// Where a walk along a chunk stands and what it found so far.  It is taken up where it stopped: the counting walk
// runs to the end of the chunk, a listing walk until it has listed as many pages as the pass gives it.
struct Walk
{
  uint64_t pos = 0;        // of the next page header in the chunk
  uint64_t out = 0;        // bytes the listed pages so far decode to
  uint64_t pages = 0;      // listed pages so far
  uint64_t largest = 0;    // the most bytes a stored part of them has
  uint32_t bare = 0;       // listed pages without a crc
  uint32_t ok = 1;         // 0: refused (pos is where)
};
// `sink.page(j, page)` is told every listed page, j counting from the walk's first.  One loop, one exit.
template <class Src, class Sink>
constexpr Walk walk_pages(Src& s, uint64_t bytes, uint32_t codec, Walk w, uint64_t most, Sink& sink)
{
  const uint64_t first = w.pages;
  bool go = w.ok && w.pos < bytes && most > 0;
  while (go) {
    Parsed r = parse_page(s, w.pos, bytes, codec);
    if (r.verdict == kRefused) {
      w.ok = 0;
      go = false;
    } else {
      if (r.verdict == kListed) {
        r.page.out_offset = w.out;
        sink.page(w.pages - first, r.page);
        w.out += r.page.uncompressed_page_size;
        w.pages += 1;
        w.largest = stored_bytes(r.page) > w.largest ? stored_bytes(r.page) : w.largest;
        w.bare += (r.page.flags & kHasCrc) ? 0u : 1u;
      }
      w.pos = r.next;
      go = w.pos < bytes && w.pages - first < most;
    }
  }
  return w;
}
struct NoSink
{
  constexpr void page(uint64_t, const Page&) {}
};

// What the counting walk makes of an item.  The order: a refusal of the walk; a page table too small for the listed
// pages; an output too small for them.
enum Fate : uint32_t { kFine = 0, kCannotDecompress = 1, kInvalidValue = 2 };
constexpr uint32_t fate_of(const Walk& w, bool table, uint64_t table_capacity, uint64_t capacity)
{
  if (!w.ok)
    return kCannotDecompress;
  if (table && w.pages > table_capacity)
    return kInvalidValue;
  return w.out > capacity ? kCannotDecompress : kFine;
}

// ---- the scratch space --------------------------------------------------------------------------------------
//   item states   kItemBytes each
//   totals        64 bytes: what the host reads after the scan of the items
//   page lists    kEntryBytes per page of a pass: kLists8 lists of 8-byte words, then kLists4 of 4-byte words
// every part 16-byte aligned.
constexpr uint64_t kItemBytes = 128;
constexpr uint64_t kLists8 = 10, kLists4 = 5;
constexpr uint64_t kEntryBytes = kLists8 * 8 + kLists4 * 4;
constexpr uint64_t kTotalsBytes = 64;

constexpr uint64_t items_bytes(uint64_t items) { return items * kItemBytes; }
constexpr uint64_t totals_at(uint64_t items) { return items_bytes(items); }
constexpr uint64_t lists_at(uint64_t items) { return totals_at(items) + kTotalsBytes; }
constexpr uint64_t list8_at(uint64_t items, uint64_t P, uint64_t j) { return lists_at(items) + 8 * P * j; }
constexpr uint64_t list4_at(uint64_t items, uint64_t P, uint64_t j) { return lists_at(items) + 8 * P * kLists8 + 4 * P * j; }
constexpr uint64_t scratch_bytes(uint64_t items, uint64_t P) { return lists_at(items) + kEntryBytes * P; }
// the least a scratch space has to hold: the states and two pages' entries
constexpr uint64_t min_scratch_bytes(uint64_t items) { return scratch_bytes(items, 2); }
// pages of a pass in `room` bytes, at most `most`; 0: not even min_scratch_bytes
constexpr uint64_t pass_entries(uint64_t room, uint64_t items, uint64_t most)
{
  if (room < min_scratch_bytes(items))
    return 0;
  const uint64_t P = (room - lists_at(items)) / kEntryBytes;
  return P < most ? P : most;
}

// ---- the passes ---------------------------------------------------------------------------------------------
// Item i contributes pages [first_i, first_i + pages_i) to the numbering, first_i the exclusive sum of the counts
// before it; pass k takes pages [k * P, (k + 1) * P).  An item's pages may span passes, a pass may hold the pages
// of many items, an item of no pages is in no pass.
constexpr uint64_t passes_of(uint64_t total_pages, uint64_t P) { return (total_pages + P - 1) / P; }
constexpr uint64_t pass_count(uint64_t total_pages, uint64_t P, uint64_t k)
{
  return total_pages - k * P < P ? total_pages - k * P : P;
}
// the entries of pass k that are item i's: [at, at + count) of the pass's lists
struct Slice
{
  uint64_t at = 0, count = 0;
};
constexpr Slice item_slice(uint64_t first, uint64_t pages, uint64_t P, uint64_t k)
{
  Slice s;
  const uint64_t lo = k * P, hi = lo + P, end = first + pages;
  const uint64_t a = first > lo ? first : lo, b = end < hi ? end : hi;
  if (a < b) {
    s.at = a - lo;
    s.count = b - a;
  }
  return s;
}

} // namespace pqp
} // namespace hcamd
