// gather_plan.hpp -- the arithmetic of a read of many byte ranges of a container in one call (hlif.hip,
// decompress_ranges; the kernels: gather_kernels.hip): whether range r = [first, first + num) of the uncompressed
// buffer is valid, the chunks [c0, c1] it touches, the piece chunk c gives to it and where that piece lands, how
// the touched chunks -- numbered by their RANK, the count of touched chunks below them -- fall into passes and
// scratch slots, and how many slots a scratch space holds.
//
// Pure arithmetic in constexpr functions: standard headers only, no HIP, no state.  The host and the kernels
// include this one copy.  tests/test_gather_plan_cpu.py compiles it with g++ alone (tests/gather_plan_driver.cpp
// prints it) and compares it with a restatement.  Sizes up to 2^63 do not overflow.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace gather {

// false: the range is refused (hipcompErrorInvalidValue), as range::range_plan refuses it -- first + num overflows
// or reaches past decomp_bytes, or either is not a multiple of `elem` (>= 1; 1: any)
constexpr bool range_valid(uint64_t decomp_bytes, uint64_t first, uint64_t num, uint32_t elem)
{
  if (elem == 0)
    return false;
  if (first > decomp_bytes || num > decomp_bytes - first) // (first + num may wrap)
    return false;
  return first % elem == 0 && num % elem == 0;
}

// a + b, or 2^64 - 1 where that is too large: the sum of the lengths of many valid ranges may pass 2^64, and a
// saturated total is above every out_bytes the call accepts (associative, so a scan may use it)
constexpr uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~uint64_t(0) : a + b; }
// the whole call is refused: the total does not fit out_bytes (or is not known exactly)
constexpr bool total_refused(uint64_t total, uint64_t out_bytes) { return total > out_bytes || total == ~uint64_t(0); }

// the chunks a valid range of num > 0 bytes touches: [c0, c1]
struct Interval
{
  uint64_t c0 = 0, c1 = 0;
};
constexpr Interval range_chunks(uint64_t chunk_bytes, uint64_t first, uint64_t num)
{
  Interval i;
  i.c0 = first / chunk_bytes;
  i.c1 = (first + num - 1) / chunk_bytes;
  return i;
}

// what chunk c (one of [c0, c1]) gives to the range: `bytes` bytes from src_at of the decoded chunk to dst_at of
// the range's place in out (0 < bytes <= the chunk's own length; the last chunk of a buffer may be short)
struct Piece
{
  uint64_t src_at = 0, bytes = 0, dst_at = 0;
};
constexpr uint64_t chunk_cap(uint64_t decomp_bytes, uint64_t chunk_bytes, uint64_t c)
{
  const uint64_t start = c * chunk_bytes;
  return decomp_bytes - start < chunk_bytes ? decomp_bytes - start : chunk_bytes;
}
constexpr Piece range_piece(uint64_t decomp_bytes, uint64_t chunk_bytes, uint64_t first, uint64_t num, uint64_t c)
{
  Piece p;
  const uint64_t start = c * chunk_bytes, chunk_end = start + chunk_cap(decomp_bytes, chunk_bytes, c);
  const uint64_t from = start > first ? start : first;
  const uint64_t range_end = first + num; // <= decomp_bytes
  const uint64_t to = chunk_end < range_end ? chunk_end : range_end;
  p.src_at = from - start;
  p.dst_at = from - first;
  p.bytes = to - from;
  return p;
}

// ---- ranks, passes, slots: a pass decodes S touched chunks, rank k in pass k / S into slot k % S ----
constexpr uint64_t pass_of(uint64_t rank, uint64_t S) { return rank / S; }
constexpr uint64_t slot_of(uint64_t rank, uint64_t S) { return rank % S; }
constexpr uint64_t passes_of(uint64_t touched, uint64_t S) { return (touched + S - 1) / S; }
// chunks of pass p (the last one may be shorter)
constexpr uint64_t pass_count(uint64_t touched, uint64_t S, uint64_t p)
{
  const uint64_t left = touched - p * S;
  return left < S ? left : S;
}
// every chunk of [c0, c1] is touched, so their ranks are consecutive: the rank of c from the rank of c0
constexpr uint64_t rank_in_range(uint64_t rank_c0, uint64_t c0, uint64_t c) { return rank_c0 + (c - c0); }
// the chunks of a range (ranks [rank_c0, rank_c0 + c1 - c0]) that pass p decodes: chunks [lo, hi), lo >= hi: none
struct InPass
{
  uint64_t lo = 0, hi = 0;
};
constexpr InPass range_in_pass(uint64_t rank_c0, uint64_t c0, uint64_t c1, uint64_t S, uint64_t p)
{
  InPass r;
  const uint64_t first_rank = p * S, end_rank = first_rank + S; // ranks of the pass: [first_rank, end_rank)
  const uint64_t rank_end = rank_c0 + (c1 - c0) + 1;
  const uint64_t a = rank_c0 > first_rank ? rank_c0 : first_rank, b = rank_end < end_rank ? rank_end : end_rank;
  if (a >= b)
    return r;
  r.lo = c0 + (a - rank_c0);
  r.hi = c0 + (b - rank_c0);
  return r;
}
// the rank of chunk c from the bitmap of touched chunks (bit c & 31 of word c >> 5) and the number of set bits in
// front of its word: rank(c) = in front of the word + popcount(word & below(c & 31))
constexpr uint32_t below(uint32_t bit) { return (uint32_t(1) << bit) - 1; } // bit < 32
constexpr uint32_t bits_below(uint32_t word, uint32_t bit)
{
  uint32_t v = word & below(bit), n = 0;
  for (; v; v &= v - 1)
    ++n;
  return n;
}

// ---- the scratch space: [fixed] [tables] [S slots, the lists of S chunks] ----
constexpr uint64_t round16(uint64_t x) { return (x + 15) & ~uint64_t(15); }
// bytes of the lists per chunk of a pass: comp_ptr, comp_size, cap, out_ptr, actual (8 each), status, two stored
// checksums (4 each)
constexpr uint64_t kListBytes = 5 * 8 + 3 * 4;
// alignment in front, the head (the words the host fetches), the LZ4 decoder's ticket words, the CrcState, the
// alignment of the lists
constexpr uint64_t kFixedBytes = 16 + 64 + 64 + 64 + 16;
constexpr uint64_t bitmap_words(uint64_t num_chunks) { return (num_chunks + 31) / 32; }
constexpr uint64_t kRankGroup = 1024; // words of the bitmap per group of the rank sum
// the tables of a call: out offsets (u64 x ranges + 1), the list of long ranges (u32 x ranges), the bitmap, the
// rank in front of each word inside its group and in front of each group (u32 each); each 16-byte aligned
constexpr uint64_t table_bytes(uint64_t ranges, uint64_t num_chunks)
{
  const uint64_t w = bitmap_words(num_chunks);
  return round16(8 * (ranges + 1)) + round16(4 * ranges) + 2 * round16(4 * w) + round16(4 * ((w + kRankGroup - 1) / kRankGroup));
}
// S: the slots (and list entries) that fit `room` bytes behind the fixed part and the tables, at most `cap`;
// 0: not even one
constexpr uint64_t slots_of(uint64_t room, uint64_t stride, uint64_t tables, uint64_t cap)
{
  if (room < kFixedBytes || room - kFixedBytes < tables)
    return 0;
  const uint64_t s = (room - kFixedBytes - tables) / (stride + kListBytes);
  return s < cap ? s : cap;
}
// the room that holds S slots
constexpr uint64_t room_of(uint64_t S, uint64_t stride, uint64_t tables) { return kFixedBytes + tables + S * (stride + kListBytes); }

} // namespace gather
} // namespace hcamd
