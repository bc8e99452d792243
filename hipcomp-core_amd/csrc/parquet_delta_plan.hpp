// parquet_delta_plan.hpp -- the arithmetic of a decode of a batch of Parquet DELTA_BINARY_PACKED streams
// (hipcomp/cascaded.hpp, decode_parquet_delta; the kernels: parquet_delta_kernels.hip): the varint reader, the parse of
// the stream's header and of a block's header, the bytes of a miniblock from its width, the walk along a stream's
// blocks in steps of 64 values, the extraction of a packed delta of up to 64 bits, the rules that refuse an item, and
// the whole decode on one thread.  INTEGRATION.md, "Parquet DELTA_BINARY_PACKED values and string offsets in the
// Cascaded manager", has the contract.
//
// constexpr functions over standard headers only, no HIP, no state, templated over the byte source: `Src` has
// `uint32_t at(uint64_t pos)`, asked only for pos inside the item.  The host and the kernels include this one copy.
// tests/test_parquet_delta_plan_cpu.py compiles it with g++ alone under the address and undefined-behaviour
// sanitizers (tests/parquet_delta_plan_driver.cpp prints it) and compares it with tests/parquet_deltagen.py.
#pragma once

#include <cstddef>
#include <cstdint>

#include "parquet_hybrid_plan.hpp" // where_of: the place of value k of a bit-packed run

namespace hcamd {
namespace pqd {

using pqh::Where;
using pqh::where_of;

constexpr uint64_t kMaxItems = uint64_t(1) << 20;
constexpr uint32_t kStep = 64; // the values of a decoding step: a wavefront's lanes

// hipcomp/cascaded.hpp, ParquetDeltaOutput: the same values in the same order
enum Output : uint32_t { kValues = 0, kOffsets = 1 };

// ---- varints -------------------------------------------------------------------------------------------------------
// A ULEB128 of at most 10 bytes, the tenth 0 or 1: 64 bits.  A failed read clears `ok` and returns 0.
template <class Src>
constexpr uint64_t read_varint(Src& s, uint64_t& pos, uint64_t end, bool& ok)
{
  uint64_t v = 0;
  uint32_t n = 0;
  bool more = true;
  while (more && ok) {
    if (n == 10 || pos >= end) {
      ok = false;
    } else {
      const uint32_t b = s.at(pos++) & 0xFFu;
      if (n == 9 && b > 1) {
        ok = false;
      } else {
        v |= (uint64_t)(b & 0x7Fu) << (7 * n);
        ++n;
        more = (b & 0x80u) != 0;
      }
    }
  }
  return ok ? v : 0;
}
constexpr uint64_t unzigzag(uint64_t u) { return (u >> 1) ^ (0 - (u & 1)); }

// ---- the header ------------------------------------------------------------------------------------------------------
struct Header
{
  bool ok = false;
  uint32_t block = 0, miniblocks = 0, per_miniblock = 0;
  uint64_t total = 0;
  uint64_t first = 0; // the first value, 64 bits of it
  uint64_t pos = 0;   // behind the header
};
// Refused: a varint that is cut, too long or too large; a block size, a miniblock count or a total that does not fit 32
// bits; a block size of 0 or no multiple of 128; 0 miniblocks, or a count that does not divide the block size; values
// per miniblock that are no multiple of 32.
template <class Src>
constexpr Header parse_header(Src& s, uint64_t n)
{
  Header h;
  bool ok = true;
  uint64_t pos = 0;
  const uint64_t block = read_varint(s, pos, n, ok);
  const uint64_t miniblocks = read_varint(s, pos, n, ok);
  const uint64_t total = read_varint(s, pos, n, ok);
  const uint64_t first = unzigzag(read_varint(s, pos, n, ok));
  if (!ok || (block >> 32) || (miniblocks >> 32) || (total >> 32))
    return h;
  if (block == 0 || block % 128 != 0 || miniblocks == 0 || block % miniblocks != 0 || (block / miniblocks) % 32 != 0)
    return h;
  h.block = (uint32_t)block;
  h.miniblocks = (uint32_t)miniblocks;
  h.per_miniblock = (uint32_t)(block / miniblocks);
  h.total = total;
  h.first = first;
  h.pos = pos;
  h.ok = true;
  return h;
}
// the elements an accepted item writes
constexpr uint64_t elements_of(uint64_t total, uint32_t output) { return output == kOffsets ? total + 1 : total; }
// What the call's own arrays refuse: more elements than the capacity; a total that is not the count the caller holds.
constexpr bool fits(const Header& h, bool has_wanted, uint64_t wanted, uint64_t capacity, uint32_t output)
{
  return h.ok && elements_of(h.total, output) <= capacity && (!has_wanted || wanted == h.total);
}

// ---- a miniblock -----------------------------------------------------------------------------------------------------
struct Piece
{
  uint64_t data = 0; // where its bytes begin
  uint32_t width = 0;
};
// (values per miniblock are a multiple of 32: whole bytes)
constexpr uint64_t miniblock_bytes(uint32_t per_miniblock, uint32_t width) { return (uint64_t)(per_miniblock / 8) * width; }
// the bytes of a block's first `needed` miniblocks, their widths read at `widths`
template <class Src>
constexpr uint64_t block_bytes(Src& s, uint64_t widths, uint32_t needed, uint32_t per_miniblock)
{
  uint64_t bytes = 0;
  for (uint32_t m = 0; m < needed; ++m)
    bytes += miniblock_bytes(per_miniblock, s.at(widths + m) & 0xFFu);
  return bytes;
}
// Miniblock `m` of a block, a needed one, its bytes at `data`.  Refused: a width above the limit; bytes, padded to the
// miniblock's full length, that run past the stream.
template <class Src>
constexpr Piece enter(Src& s, uint64_t widths, uint64_t m, uint64_t data, uint64_t end, uint32_t per_miniblock, uint32_t limit,
                      bool& ok)
{
  Piece p;
  p.data = data;
  p.width = s.at(widths + m) & 0xFFu;
  if (p.width > limit || miniblock_bytes(per_miniblock, p.width) > end - data)
    ok = false;
  return p;
}

// ---- a packed delta ----------------------------------------------------------------------------------------------------
// Value k of a miniblock begins `shift` bits into the byte at `byte` of it (where_of) and lies in the at most 9 bytes
// from there: `lo` the first 8 of them, little-endian, `hi` the ninth (bytes behind the value's own may hold anything).
constexpr uint64_t value_of64(uint64_t lo, uint32_t hi, uint32_t shift, uint32_t width)
{
  uint64_t v = lo >> shift;
  if (shift)
    v |= (uint64_t)hi << (64 - shift);
  return width < 64 ? v & ((uint64_t(1) << width) - 1) : v;
}
// by single bytes: reads the value's own bytes and no other
template <class Src>
constexpr uint64_t extract64(Src& s, uint64_t data, uint64_t k, uint32_t width)
{
  const Where w = where_of(k, width);
  uint64_t lo = 0;
  uint32_t hi = 0;
  for (uint32_t j = 0; j < w.bytes; ++j) {
    const uint32_t b = s.at(data + w.byte + j) & 0xFFu;
    if (j < 8)
      lo |= (uint64_t)b << (8 * j);
    else
      hi = b;
  }
  return value_of64(lo, hi, w.shift, width);
}

// ---- the walk ----------------------------------------------------------------------------------------------------
// `Sink` has `bool step(first, count, min_delta, a, k0, split, b)`: values [first, first + count) of the stream, count
// <= 64, are the block's minimum delta plus the packed deltas k0, k0 + 1, ... of miniblock `a` -- `split` of them --
// and then 0, 1, ... of miniblock `b`.  A step begins at a multiple of 64 of its block, and the values per miniblock
// are a multiple of 32, so it never touches a third miniblock.  `false` refuses the item.  Every loop has one exit.
struct Walk
{
  bool ok = true;
  uint64_t pos = 0; // behind the last needed miniblock, or behind the header
};
struct NoSink
{
  constexpr bool step(uint64_t, uint32_t, uint64_t, const Piece&, uint32_t, uint32_t, const Piece&) { return true; }
};
// Refused: a minimum delta that is cut, too long or too large; width bytes that run past the stream; what `enter`
// refuses of a miniblock that holds a wanted value; what the sink refuses.  The width bytes of the other miniblocks
// are stepped over unread, and nothing behind the last needed miniblock is looked at.
template <class Src, class Sink>
constexpr Walk walk_blocks(Src& s, const Header& h, uint64_t end, uint32_t limit, Sink& sink)
{
  Walk w;
  w.pos = h.pos;
  uint64_t first = 1;                           // the value the next block begins with
  uint64_t left = h.total ? h.total - 1 : 0;    // deltas still to come
  while (w.ok && left > 0) {
    uint64_t pos = w.pos;
    bool ok = true;
    const uint64_t min_delta = unzigzag(read_varint(s, pos, end, ok));
    if (!ok || end - pos < h.miniblocks) {
      w.ok = false;
    } else {
      const uint64_t widths = pos;
      const uint32_t in_block = left < h.block ? (uint32_t)left : h.block;
      uint64_t m = 0;                            // the miniblock that holds value `at` of the block
      uint64_t m_end = h.per_miniblock;          // the first value of the block behind it
      Piece cur = enter(s, widths, m, pos + h.miniblocks, end, h.per_miniblock, limit, ok);
      for (uint64_t at = 0; ok && at < in_block; at += kStep) {
        const uint32_t count = in_block - at < kStep ? (uint32_t)(in_block - at) : kStep;
        const uint32_t k0 = (uint32_t)(at + h.per_miniblock - m_end);
        const uint32_t room = h.per_miniblock - k0;
        const uint32_t split = count < room ? count : room;
        Piece next = cur;
        if (split < count)
          next = enter(s, widths, m + 1, cur.data + miniblock_bytes(h.per_miniblock, cur.width), end, h.per_miniblock, limit, ok);
        if (ok)
          ok = sink.step(first + at, count, min_delta, cur, k0, split, next);
        if (ok && split < count) {
          cur = next;
          ++m;
          m_end += h.per_miniblock;
        }
        if (ok && at + kStep < in_block && at + kStep == m_end) { // the next step begins a miniblock
          cur = enter(s, widths, m + 1, cur.data + miniblock_bytes(h.per_miniblock, cur.width), end, h.per_miniblock, limit, ok);
          ++m;
          m_end += h.per_miniblock;
        }
      }
      w.ok = ok;
      w.pos = cur.data + miniblock_bytes(h.per_miniblock, cur.width);
      first += in_block;
      left -= in_block;
    }
  }
  return w;
}

// ---- offsets -----------------------------------------------------------------------------------------------------------
// The lengths of a DELTA_LENGTH_BYTE_ARRAY page: the delta layer in 32 bits, their sum in 64.  Refused: a negative
// length (the sink's step says so), a sum above 2^31 - 1 where the offsets are 32-bit, a sum above the bytes of the
// item behind the lengths.
constexpr bool negative_length(uint32_t length) { return (length >> 31) != 0; }
constexpr bool offsets_fit(uint64_t sum, uint64_t n, uint64_t consumed, uint32_t element_bits)
{
  return (element_bits > 32 || sum <= 0x7FFFFFFFu) && sum <= n - consumed;
}

// What the call says of an item.  A refused item has 0 and 0.
struct Verdict
{
  bool ok = false;
  uint64_t consumed = 0;
  uint64_t count = 0;
};
constexpr Verdict verdict_of(bool ok, const Header& h, const Walk& w)
{
  Verdict v;
  v.ok = ok;
  if (ok) {
    v.consumed = w.pos;
    v.count = h.total;
  }
  return v;
}

// ---- the whole of it on one thread ---------------------------------------------------------------------------------------
// The stream is walked without storing, then decoded, so that a refused item has nothing written.  T: uint32_t (Parquet
// INT32, HIPCOMP_TYPE_INT) or uint64_t (INT64, HIPCOMP_TYPE_LONGLONG); unsigned, so that the sums wrap.  What the host
// path of a measurement runs, and what the tests hold the kernel to.
struct Bytes
{
  const uint8_t* p;
  constexpr uint32_t at(uint64_t pos) const { return p[pos]; }
};
template <class T>
struct ValuesSink
{
  const uint8_t* bytes;
  T* out;
  T last;
  constexpr bool step(uint64_t first, uint32_t count, uint64_t min_delta, const Piece& a, uint32_t k0, uint32_t split, const Piece& b)
  {
    Bytes src{bytes};
    for (uint32_t k = 0; k < count; ++k) {
      const uint64_t packed = k < split ? extract64(src, a.data, k0 + k, a.width) : extract64(src, b.data, k - split, b.width);
      last = (T)(last + (T)min_delta + (T)packed);
      out[first + k] = last;
    }
    return true;
  }
};
template <class T, bool kStore>
struct OffsetsSink
{
  const uint8_t* bytes;
  T* out;
  uint32_t last; // a length
  uint64_t sum;
  constexpr bool take(uint64_t index) // value `index` is `last`
  {
    if (negative_length(last))
      return false;
    sum += last;
    if (kStore)
      out[index + 1] = (T)sum;
    return true;
  }
  constexpr bool step(uint64_t first, uint32_t count, uint64_t min_delta, const Piece& a, uint32_t k0, uint32_t split, const Piece& b)
  {
    Bytes src{bytes};
    bool ok = true;
    for (uint32_t k = 0; ok && k < count; ++k) {
      const uint64_t packed = k < split ? extract64(src, a.data, k0 + k, a.width) : extract64(src, b.data, k - split, b.width);
      last = last + (uint32_t)min_delta + (uint32_t)packed;
      ok = take(first + k);
    }
    return ok;
  }
};
template <class T>
constexpr Verdict decode_item(const uint8_t* bytes, uint64_t n, bool has_wanted, uint64_t wanted, uint64_t capacity, uint32_t output,
                              T* out)
{
  Bytes src{bytes};
  const uint32_t bits = (uint32_t)(8 * sizeof(T));
  const Header h = parse_header(src, n);
  Walk w;
  bool ok = fits(h, has_wanted, wanted, capacity, output);
  if (ok && output == kOffsets) {
    OffsetsSink<T, false> dry{bytes, out, (uint32_t)h.first, 0};
    ok = h.total == 0 || dry.take(0);
    if (ok) {
      w = walk_blocks(src, h, n, bits, dry);
      ok = w.ok && offsets_fit(dry.sum, n, w.pos, bits);
    }
    if (ok) {
      OffsetsSink<T, true> sink{bytes, out, (uint32_t)h.first, 0};
      out[0] = 0;
      if (h.total)
        (void)sink.take(0);
      w = walk_blocks(src, h, n, bits, sink);
    }
  } else if (ok) {
    NoSink none;
    w = walk_blocks(src, h, n, bits, none);
    ok = w.ok;
    if (ok && h.total) {
      ValuesSink<T> sink{bytes, out, (T)h.first};
      out[0] = (T)h.first;
      w = walk_blocks(src, h, n, bits, sink);
    }
  }
  return verdict_of(ok, h, w);
}

} // namespace pqd
} // namespace hcamd
