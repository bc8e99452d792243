// deflate_tables.hpp -- the canonical-Huffman logic of the Deflate decoder (RFC 1951), free of HIP.
//
// Everything here is constexpr and plain C++17: the kernel (deflate_kernels.hip) and the CPU driver
// (tests/deflate_tables_driver.cpp) include this one file, so what the tests prove about it on the CPU is what
// the GPU runs.  It holds the constant tables of the format, the verdict on a set of code lengths (the same
// accept / reject as zlib's inflate, see verdict_counts) and the decode table with its two lookups:
//
//   count[l]   number of codes of length l (1..15)
//   sorted[]   the symbols in canonical order (by length, then by symbol)
//   fast[]     indexed by the next FASTBITS bits of the stream: (symbol << 4) | length for every code of at
//              most FASTBITS bits, 0 where the bits start a longer code or no code at all
//
// A code longer than FASTBITS is found by canon_decode(), the count/offset walk over `count` and `sorted`
// (one step per bit).  The same walk fills `fast`: entry e is canon_decode(e) cut off at FASTBITS bits, so the
// table can be filled in parallel over its entries -- the kernel does that with 64 lanes, build_table() below
// does it in a loop.
#pragma once

#include <cstdint>

namespace hcamd {
namespace deflate {

constexpr int kMaxBits = 15;
constexpr int kFixedLitLen = 288, kFixedDist = 32;   // the fixed block codes 288 + 32 symbols,
constexpr int kMaxLitLen = 286, kMaxDist = 30;       // of which these many may be used (and HLIT / HDIST name)
constexpr int kNumCodeLen = 19;
constexpr int kEndOfBlock = 256;
constexpr int kLitFastBits = 10, kDistFastBits = 8, kCodeLenFastBits = 7;

// length symbols 257..285 and distance symbols 0..29 (RFC 1951 3.2.5)
constexpr uint16_t kLengthBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                      31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                    193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
// the order in which the code lengths of the code-length alphabet are stored (3.2.7)
constexpr uint8_t kCodeLenOrder[kNumCodeLen] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// The same four tables as arithmetic (the kernel computes them on the scalar unit instead of loading them);
// `i` is the symbol less 257 for lengths.
constexpr uint32_t length_extra(uint32_t i) { return i < 8 || i == 28 ? 0u : (i - 4u) >> 2; }
constexpr uint32_t length_base(uint32_t i) { return i < 8 ? 3u + i : i == 28 ? 258u : 3u + ((4u + (i & 3u)) << length_extra(i)); }
constexpr uint32_t dist_extra(uint32_t s) { return s < 4 ? 0u : (s >> 1) - 1u; }
constexpr uint32_t dist_base(uint32_t s) { return s < 4 ? 1u + s : 1u + ((2u + (s & 1u)) << dist_extra(s)); }

constexpr bool arithmetic_matches_tables()
{
  for (uint32_t i = 0; i < 29; ++i)
    if (length_base(i) != kLengthBase[i] || length_extra(i) != kLengthExtra[i])
      return false;
  for (uint32_t s = 0; s < 30; ++s)
    if (dist_base(s) != kDistBase[s] || dist_extra(s) != kDistExtra[s])
      return false;
  return true;
}
static_assert(arithmetic_matches_tables(), "length_base / dist_base disagree with RFC 1951's tables");

// code lengths of the fixed block (3.2.6): literal/length symbol i, every distance symbol 5 bits
constexpr uint32_t fixed_litlen_length(uint32_t i) { return i < 144 ? 8u : i < 256 ? 9u : i < 280 ? 7u : 8u; }
constexpr uint32_t kFixedDistLength = 5;

enum Kind { kCodeLen = 0, kLitLen = 1, kDist = 2 };

enum Verdict {
  kOk = 0,
  kOverSubscribed,
  kIncomplete,
  kNoEndOfBlock,            // literal/length set without code 256
  kTooManySymbols,          // HLIT > 286 or HDIST > 30
  kRepeatWithoutPrevious,   // code-length symbol 16 first
  kRepeatPastEnd,           // a run that passes HLIT + HDIST
  kBadSymbol,               // bits that are no code of the set
  kTruncated,
};

constexpr const char* verdict_name(Verdict v)
{
  switch (v) {
  case kOk: return "ok";
  case kOverSubscribed: return "oversubscribed";
  case kIncomplete: return "incomplete";
  case kNoEndOfBlock: return "no-end-of-block";
  case kTooManySymbols: return "too-many-symbols";
  case kRepeatWithoutPrevious: return "repeat-without-previous";
  case kRepeatPastEnd: return "repeat-past-end";
  case kBadSymbol: return "bad-symbol";
  default: return "truncated";
  }
}

constexpr Verdict verdict_header(uint32_t hlit, uint32_t hdist)
{
  return hlit > (uint32_t)kMaxLitLen || hdist > (uint32_t)kMaxDist ? kTooManySymbols : kOk;
}

// The verdict on a set of code lengths, given as count[1..15].  It is zlib's (inftrees.c): an over-subscribed
// set is refused; an incomplete one is refused except where its longest code has one bit -- that is a single
// code of length 1, which inflate accepts in the literal/length and the distance alphabet (the other 1-bit
// pattern is then no code, and an error only where the stream uses it) -- and except a distance alphabet
// without any code (an error only where the block has a match).  The code-length alphabet has to be complete.
template <class C>
constexpr Verdict verdict_counts(const C& count, Kind kind)
{
  int max = 0;
  for (int l = 1; l <= kMaxBits; ++l)
    if (count[l] != 0)
      max = l;
  if (max == 0)
    return kind == kDist ? kOk : kIncomplete;
  int left = 1;
  for (int l = 1; l <= kMaxBits; ++l) {
    left = (left << 1) - (int)count[l];
    if (left < 0)
      return kOverSubscribed;
  }
  if (left > 0 && (kind == kCodeLen || max != 1))
    return kIncomplete;
  return kOk;
}

// One symbol of the code-length stream (3.2.7): `sym` with the value of its extra bits, `have` lengths written
// so far of `total` = HLIT + HDIST, `prev` the last length written.  -> `count` lengths of value `value` follow.
constexpr uint32_t code_len_extra_bits(uint32_t sym) { return sym < 16 ? 0u : sym == 16 ? 2u : sym == 17 ? 3u : 7u; }
constexpr Verdict code_len_run(uint32_t sym, uint32_t extra, uint32_t have, uint32_t total, uint32_t prev, uint32_t& value,
                               uint32_t& count)
{
  if (sym < 16) {
    value = sym;
    count = 1;
  } else if (sym == 16) {
    if (have == 0)
      return kRepeatWithoutPrevious;
    value = prev;
    count = 3 + extra;
  } else {
    value = 0;
    count = (sym == 17 ? 3u : 11u) + extra;
  }
  return have + count > total ? kRepeatPastEnd : kOk;
}

// The count/offset walk: `bits` holds the stream's next bits, first bit lowest.  -> (symbol << 4) | length of the
// code they start with if it has at most `maxlen` bits, else 0.  (Codes are stored first bit first, so the
// code is assembled one bit at a time; `first` is the first code of the current length, `index` its place in
// `sorted`.)
template <class C, class S>
constexpr uint32_t canon_decode(const C& count, const S& sorted, uint32_t bits, int maxlen)
{
  uint32_t code = 0, first = 0, index = 0;
  for (int len = 1; len <= maxlen; ++len) {
    code |= bits & 1u;
    bits >>= 1;
    const uint32_t c = count[len];
    if (code < first + c)
      return ((uint32_t)sorted[index + (code - first)] << 4) | (uint32_t)len;
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0;
}

template <int N, int FASTBITS>
struct Table
{
  uint16_t count[kMaxBits + 1];
  uint16_t sorted[N];
  uint16_t fast[1 << FASTBITS];
};

// lengths[0, n) -> table and verdict (the table is filled whatever the verdict, except for an over-subscribed
// set, whose walk would leave `sorted`)
template <int N, int FASTBITS>
constexpr Verdict build_table(const uint8_t* lengths, int n, Kind kind, Table<N, FASTBITS>& t)
{
  for (int l = 0; l <= kMaxBits; ++l)
    t.count[l] = 0;
  for (int i = 0; i < n; ++i)
    ++t.count[lengths[i]];
  t.count[0] = 0;
  if (kind == kLitLen && (n <= kEndOfBlock || lengths[kEndOfBlock] == 0))
    return kNoEndOfBlock;
  const Verdict v = verdict_counts(t.count, kind);
  if (v == kOverSubscribed)
    return v;
  uint16_t offs[kMaxBits + 2] = {};
  for (int l = 1; l <= kMaxBits; ++l)
    offs[l + 1] = (uint16_t)(offs[l] + t.count[l]);
  for (int i = 0; i < N; ++i)
    t.sorted[i] = 0;
  for (int i = 0; i < n; ++i)
    if (lengths[i] != 0)
      t.sorted[offs[lengths[i]]++] = (uint16_t)i;
  for (uint32_t e = 0; e < (1u << FASTBITS); ++e)
    t.fast[e] = (uint16_t)canon_decode(t.count, t.sorted, e, FASTBITS);
  return v;
}

// what the kernel does per symbol: the fast table, then the walk
template <int N, int FASTBITS>
constexpr uint32_t lookup(const Table<N, FASTBITS>& t, uint32_t bits)
{
  const uint32_t e = t.fast[bits & ((1u << FASTBITS) - 1u)];
  return e != 0 ? e : canon_decode(t.count, t.sorted, bits, kMaxBits);
}

} // namespace deflate
} // namespace hcamd
