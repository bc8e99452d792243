// parquet_hybrid_plan.hpp -- the arithmetic of a decode of a batch of Parquet RLE / bit-packed hybrid streams
// (hipcomp/cascaded.hpp, decode_parquet_hybrid; the kernels: parquet_hybrid_kernels.hip): the reader of a run
// header, the rules that turn the bytes at a position of a stream into a run or a refusal, the walk along a
// stream's runs, the extraction of value k of a bit-packed run, and what the three forms of an item put in front of
// the runs.  INTEGRATION.md, "Parquet levels and dictionary indices in the Cascaded manager", has the contract.
//
// constexpr functions over standard headers only, no HIP, no state, templated over the byte source: `Src` has
// `uint32_t at(uint64_t pos)`, asked only for pos inside the item.  The host and the kernels include this one copy.
// tests/test_parquet_hybrid_plan_cpu.py compiles it with g++ alone under the address and undefined-behaviour
// sanitizers (tests/parquet_hybrid_plan_driver.cpp prints it) and compares it with tests/parquet_hybridgen.py.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace pqh {

constexpr uint64_t kMaxItems = uint64_t(1) << 20;
constexpr uint32_t kMaxBitWidth = 32;

// hipcomp/cascaded.hpp, ParquetHybridForm: the same values in the same order
enum Form : uint32_t { kBare = 0, kLengthPrefixed = 1, kWidthPrefixed = 2 };

// ---- a run -----------------------------------------------------------------------------------------------------
struct Run
{
  bool ok = false;
  bool packed = false;
  uint32_t value = 0; // an RLE run's, as read
  uint64_t take = 0;  // the values of it that are wanted: the run's own count, clipped
  uint64_t data = 0;  // where a bit-packed run's bytes begin
  uint64_t next = 0;  // where the run ends: behind its bytes, or at the end of the stream where they are cut short
};

// The header: a ULEB128 of at most 5 bytes whose value fits 32 bits.  A failed read clears `ok` and returns 0.
template <class Src>
constexpr uint32_t read_header(Src& s, uint64_t& pos, uint64_t end, bool& ok)
{
  uint64_t v = 0;
  uint32_t n = 0;
  bool more = true;
  while (more && ok) {
    if (n == 5 || pos >= end) {
      ok = false;
    } else {
      const uint32_t b = s.at(pos++) & 0xFFu;
      v |= (uint64_t)(b & 0x7Fu) << (7 * n);
      ++n;
      more = (b & 0x80u) != 0;
    }
  }
  if (v >> 32)
    ok = false;
  return ok ? (uint32_t)v : 0;
}

constexpr uint32_t value_bytes(uint32_t bit_width) { return (bit_width + 7) / 8; }
// the bytes that hold the first `values` values of a bit-packed run
constexpr uint64_t packed_bytes(uint64_t values, uint32_t bit_width) { return (values * bit_width + 7) / 8; }

// The run at `pos` of a stream that ends at `end`, `wanted` (> 0) values still to come.  Refused: a header that is
// cut, too long or too large; 0 values or 0 groups; an RLE value that runs past the stream; a bit-packed run whose
// bytes -- those of the values wanted, no more -- run past the stream.
template <class Src>
constexpr Run next_run(Src& s, uint64_t pos, uint64_t end, uint32_t bit_width, uint64_t wanted)
{
  Run r;
  bool ok = true;
  const uint32_t h = read_header(s, pos, end, ok);
  const uint64_t count = h >> 1; // values of an RLE run, groups of 8 of a bit-packed one
  if (!ok || count == 0)
    return r;
  const uint64_t room = end - pos;
  if (h & 1u) {
    const uint64_t values = count * 8, bytes = count * bit_width;
    r.packed = true;
    r.take = values < wanted ? values : wanted;
    if (packed_bytes(r.take, bit_width) > room)
      return r;
    r.data = pos;
    r.next = pos + (bytes < room ? bytes : room);
  } else {
    const uint32_t vb = value_bytes(bit_width);
    if (vb > room)
      return r;
    for (uint32_t j = 0; j < vb; ++j)
      r.value |= (s.at(pos + j) & 0xFFu) << (8 * j);
    r.take = count < wanted ? count : wanted;
    r.next = pos + vb;
  }
  r.ok = true;
  return r;
}

// ---- value k of a bit-packed run ---------------------------------------------------------------------------------
// It begins `shift` bits into the byte at `byte` of the run and lies in the at most 5 bytes from there.
struct Where
{
  uint64_t byte;
  uint32_t shift, bytes;
};
constexpr Where where_of(uint64_t k, uint32_t bit_width)
{
  const uint64_t bit = k * bit_width;
  const uint32_t shift = (uint32_t)(bit & 7u);
  return Where{bit >> 3, shift, (shift + bit_width + 7) / 8};
}
// from the 8 bytes (little-endian; those behind the value's own may hold anything) at its first byte
constexpr uint32_t value_of(uint64_t bytes8, uint32_t shift, uint32_t bit_width)
{
  const uint64_t mask = (uint64_t(1) << bit_width) - 1; // (bit_width <= 32)
  return (uint32_t)((bytes8 >> shift) & mask);
}
// by single bytes: reads the value's own bytes and no other
template <class Src>
constexpr uint32_t extract(Src& s, uint64_t data, uint64_t k, uint32_t bit_width)
{
  const Where w = where_of(k, bit_width);
  uint64_t v = 0;
  for (uint32_t j = 0; j < w.bytes; ++j)
    v |= (uint64_t)(s.at(data + w.byte + j) & 0xFFu) << (8 * j);
  return value_of(v, w.shift, bit_width);
}

// ---- the walk ----------------------------------------------------------------------------------------------------
// `Sink` has rle(first, count, value) and packed(first, count, data, bit_width): values [first, first + count) of
// the output.  Every loop has one exit.
struct Walk
{
  bool ok = true;
  uint64_t pos = 0;  // behind the last run used
  uint64_t done = 0; // values so far
};
struct NoSink
{
  constexpr void rle(uint64_t, uint64_t, uint32_t) {}
  constexpr void packed(uint64_t, uint64_t, uint64_t, uint32_t) {}
};
template <class Src, class Sink>
constexpr Walk walk_runs(Src& s, uint64_t pos, uint64_t end, uint32_t bit_width, uint64_t wanted, Sink& sink)
{
  Walk w;
  w.pos = pos;
  while (w.ok && w.done < wanted) {
    const Run r = next_run(s, w.pos, end, bit_width, wanted - w.done);
    if (!r.ok) {
      w.ok = false;
    } else {
      if (r.packed)
        sink.packed(w.done, r.take, r.data, bit_width);
      else
        sink.rle(w.done, r.take, r.value);
      w.done += r.take;
      w.pos = r.next;
    }
  }
  return w;
}

// ---- an item -------------------------------------------------------------------------------------------------------
// What stands in front of the runs.  Refused: more values than the capacity; a width above 32 or above the
// element's bits; a length prefix that is cut or runs past the item; a WidthPrefixed item without its byte that
// wants values.  (The prefix and the width byte are read and held to these rules whether values are wanted or not;
// a WidthPrefixed item of 0 bytes that wants none is the one item that has neither.)
struct Frame
{
  bool ok = false;
  uint64_t pos = 0, end = 0; // the runs
  uint32_t bit_width = 0;
};
template <class Src>
constexpr Frame frame_of(Src& s, uint64_t n, uint32_t form, uint32_t bit_width, uint64_t wanted, uint64_t capacity,
                         uint32_t element_bits)
{
  Frame f;
  f.end = n;
  f.bit_width = bit_width;
  if (wanted > capacity)
    return f;
  if (form == kLengthPrefixed) {
    if (n < 4)
      return f;
    uint64_t len = 0;
    for (uint32_t j = 0; j < 4; ++j)
      len |= (uint64_t)(s.at(j) & 0xFFu) << (8 * j);
    if (len > n - 4)
      return f;
    f.pos = 4;
    f.end = 4 + len;
  } else if (form == kWidthPrefixed) {
    if (n == 0) {
      f.bit_width = 0;
      f.ok = wanted == 0;
      return f;
    }
    f.bit_width = s.at(0) & 0xFFu;
    f.pos = 1;
  }
  f.ok = f.bit_width <= kMaxBitWidth && f.bit_width <= element_bits;
  return f;
}

// What the call says of an item.  A refused item has 0 and 0.
struct Verdict
{
  bool ok = false;
  uint64_t consumed = 0;
};
constexpr Verdict verdict_of(const Frame& f, const Walk& w, uint32_t form)
{
  Verdict v;
  v.ok = f.ok && w.ok;
  if (v.ok)
    v.consumed = form == kLengthPrefixed ? f.end : w.pos;
  return v;
}

// The whole of it on one thread: the headers are walked without storing, then the values are decoded, so that a
// refused item has nothing written.  `out`: wanted elements of T.  What the host path of a measurement runs, and
// what the tests hold the kernel to.
template <class T>
struct StoreSink
{
  const uint8_t* bytes;
  T* out;
  uint32_t match;
  uint64_t matches = 0;
  struct Bytes
  {
    const uint8_t* p;
    constexpr uint32_t at(uint64_t pos) const { return p[pos]; }
  };
  constexpr void rle(uint64_t first, uint64_t count, uint32_t value)
  {
    const T v = (T)value;
    for (uint64_t i = 0; i < count; ++i)
      out[first + i] = v;
    if ((uint32_t)v == match)
      matches += count;
  }
  constexpr void packed(uint64_t first, uint64_t count, uint64_t data, uint32_t bit_width)
  {
    Bytes b{bytes};
    for (uint64_t k = 0; k < count; ++k) {
      const T v = (T)extract(b, data, k, bit_width);
      out[first + k] = v;
      matches += (uint32_t)v == match;
    }
  }
};
template <class T>
constexpr Verdict decode_item(const uint8_t* bytes, uint64_t n, uint32_t form, uint32_t bit_width, uint64_t wanted,
                              uint64_t capacity, T* out, uint32_t match, uint64_t& matches)
{
  typename StoreSink<T>::Bytes src{bytes};
  matches = 0;
  const Frame f = frame_of(src, n, form, bit_width, wanted, capacity, (uint32_t)(8 * sizeof(T)));
  Walk w;
  if (f.ok) {
    NoSink none;
    w = walk_runs(src, f.pos, f.end, f.bit_width, wanted, none);
    if (w.ok) {
      StoreSink<T> sink{bytes, out, match};
      w = walk_runs(src, f.pos, f.end, f.bit_width, wanted, sink);
      matches = sink.matches;
    }
  }
  return verdict_of(f, w, form);
}

} // namespace pqh
} // namespace hcamd
