// deflate_codes.hpp -- the code-building logic of the Deflate encoder (RFC 1951), free of HIP.
//
// Everything here is constexpr and plain C++17, as deflate_tables.hpp is for the decoder: the kernel
// (deflate_compress_kernels.hip) and the CPU driver (tests/deflate_codes_driver.cpp) include this one file, so
// what the tests prove about it on the CPU is what the GPU runs.  It holds
//
//   length_symbol / dist_symbol   match length and distance -> symbol (deflate_tables.hpp has the inverse)
//   rank_of, build_lengths        histogram -> code lengths of at most `maxbits` bits
//   assign_codes                  lengths -> canonical codes, bit-reversed (the stream takes codes first bit first,
//                                 everything else lowest bit first)
//   code_length_stream            the two sets of lengths -> the run-length symbols 0..18 and their histogram
//   trimmed_hlit / _hdist / _hclen
//   dynamic_cost / fixed_cost / stored_cost   exact bit lengths of a chunk as one block of each kind
//   put_dynamic_header            the header of a dynamic block through a caller's put(bits, count)
//
// Code lengths.  The used symbols are sorted by (frequency, symbol) -- rank_of() gives a symbol's place, so the
// sort runs in parallel over the symbols where there are lanes for it -- and merged by the two-queue method
// (leaves before inner nodes of equal weight, which keeps the tree as shallow as an optimal tree can be).  Only
// the number of leaves per depth is kept: handing the longest lengths to the rarest symbols costs exactly what
// the tree costs.  Leaves deeper than `maxbits` are cut to it, and the excess of the Kraft sum -- an integer in
// units of 2^-maxbits -- is taken back one unit at a time: a leaf of the deepest level above the limit moves one
// level down and takes a leaf of the limit level as its sibling (zlib's gen_bitlen does the same).
#pragma once

#include <cstdint>

#include "deflate_tables.hpp"

namespace hcamd {
namespace deflate {

constexpr int kCodeLenMaxBits = 7;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDistance = 32768;
constexpr uint32_t kStoredBlockMax = 65535;

constexpr uint32_t floor_log2(uint32_t v) // v >= 1
{
  uint32_t r = 0;
  while (v >>= 1)
    ++r;
  return r;
}

// match length 3..258 -> symbol 257..285
constexpr uint32_t length_symbol(uint32_t len)
{
  const uint32_t v = len - 3u;
  if (v < 8u)
    return 257u + v;
  if (len == kMaxMatch)
    return 285u;
  const uint32_t e = floor_log2(v) - 2u;
  return 261u + 4u * e + ((v >> e) & 3u);
}

// distance 1..32768 -> symbol 0..29
constexpr uint32_t dist_symbol(uint32_t dist)
{
  const uint32_t v = dist - 1u;
  if (v < 4u)
    return v;
  const uint32_t m = floor_log2(v);
  return 2u * m + ((v >> (m - 1u)) & 1u);
}

constexpr bool symbols_invert_the_tables()
{
  for (uint32_t len = 3; len <= kMaxMatch; ++len) {
    const uint32_t i = length_symbol(len) - 257u;
    if (i >= 29u || len < length_base(i) || len - length_base(i) >= (1u << length_extra(i)))
      return false;
  }
  // (both ends of every distance symbol's range; dist_symbol never falls as the distance grows)
  for (uint32_t s = 0; s < 30u; ++s)
    if (dist_symbol(dist_base(s)) != s || dist_symbol(dist_base(s) + (1u << dist_extra(s)) - 1u) != s)
      return false;
  return true;
}
static_assert(symbols_invert_the_tables(), "length_symbol / dist_symbol disagree with RFC 1951's tables");

constexpr uint32_t reverse_bits(uint32_t code, uint32_t len)
{
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i)
    r |= ((code >> i) & 1u) << (len - 1u - i);
  return r;
}

// ---- histogram -> code lengths ---------------------------------------------------------------------------------
constexpr int kMaxSymbols = kFixedLitLen; // the largest alphabet

struct HuffWork
{
  uint16_t order[kMaxSymbols];  // the used symbols by (frequency, symbol)
  uint32_t weight[kMaxSymbols]; // inner node k: its weight, later its depth
  uint16_t parent[kMaxSymbols]; // inner node k: the inner node it hangs from
  uint8_t leaves[kMaxSymbols];  // inner node k: how many of its two children are leaves
  uint16_t count[kMaxBits + 1]; // leaves per code length
  uint16_t next[kMaxBits + 1];  // assign_codes: next code per length
};

// the place of symbol i among the used symbols of freq[0, n), sorted by (frequency, symbol); i is a used one
template <class F>
constexpr uint32_t rank_of(const F& freq, int n, int i)
{
  const uint32_t f = freq[i];
  uint32_t r = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t g = freq[j];
    r += (g != 0u && (g < f || (g == f && j < i))) ? 1u : 0u;
  }
  return r;
}

// -> number of used symbols; w.order filled
template <class F>
constexpr int sort_symbols(const F& freq, int n, HuffWork& w)
{
  int used = 0;
  for (int i = 0; i < n; ++i)
    if (freq[i] != 0u) {
      w.order[rank_of(freq, n, i)] = (uint16_t)i;
      ++used;
    }
  return used;
}

// freq[0, n) with w.order sorted (`used` symbols) -> lens[0, n): 0 for an unused symbol, else 1..maxbits.  A
// single used symbol gets one bit (the decoder takes such a set in the literal/length and the distance alphabet);
// with `complete` -- the code-length alphabet, whose code has to be complete -- it gets a partner of one bit, the
// first other symbol.  This is the one function both the CPU path (build_lengths) and the kernel go through.
template <class F, class L>
constexpr void lengths_from_sorted(const F& freq, int n, int used, int maxbits, HuffWork& w, L& lens, bool complete = false)
{
  for (int i = 0; i < n; ++i)
    lens[i] = 0;
  if (used == 0)
    return;
  if (used == 1) {
    lens[w.order[0]] = 1;
    if (complete)
      lens[w.order[0] == 0 ? 1 : 0] = 1;
    return;
  }
  // two queues: the sorted leaves, and the inner nodes in the order they are made (their weights never fall)
  int leaf = 0, node = 0;
  for (int made = 0; made < used - 1; ++made) {
    uint32_t sum = 0, from_leaves = 0;
    for (int c = 0; c < 2; ++c) {
      const bool take_leaf = leaf < used && (node >= made || freq[w.order[leaf]] <= w.weight[node]);
      if (take_leaf) {
        sum += freq[w.order[leaf]];
        ++leaf;
        ++from_leaves;
      } else {
        sum += w.weight[node];
        w.parent[node] = (uint16_t)made;
        ++node;
      }
    }
    w.weight[made] = sum;
    w.leaves[made] = (uint8_t)from_leaves;
  }
  for (int l = 0; l <= kMaxBits; ++l)
    w.count[l] = 0;
  // depths from the root down (a parent is made after its children), leaves counted per depth, cut to maxbits
  const int root = used - 2;
  uint32_t kraft = 0; // in units of 2^-maxbits
  for (int k = root; k >= 0; --k) {
    const uint32_t depth = k == root ? 0u : w.weight[w.parent[k]] + 1u;
    w.weight[k] = depth;
    const uint32_t d = depth + 1u > (uint32_t)maxbits ? (uint32_t)maxbits : depth + 1u;
    w.count[d] = (uint16_t)(w.count[d] + w.leaves[k]);
    kraft += (uint32_t)w.leaves[k] << ((uint32_t)maxbits - d);
  }
  for (uint32_t excess = kraft - (1u << maxbits); excess > 0; --excess) {
    int bits = maxbits - 1;
    while (w.count[bits] == 0)
      --bits;
    --w.count[bits];
    w.count[bits + 1] = (uint16_t)(w.count[bits + 1] + 2);
    --w.count[maxbits];
  }
  int at = 0;
  for (int bits = maxbits; bits >= 1; --bits)
    for (int c = 0; c < (int)w.count[bits]; ++c)
      lens[w.order[at++]] = (uint8_t)bits;
}

template <class F, class L>
constexpr void build_lengths(const F& freq, int n, int maxbits, HuffWork& w, L& lens, bool complete = false)
{
  const int used = sort_symbols(freq, n, w);
  lengths_from_sorted(freq, n, used, maxbits, w, lens, complete);
}

// lens[0, n) -> codes[0, n), each reversed so that its first bit is the lowest
template <class L, class C>
constexpr void assign_codes(const L& lens, int n, HuffWork& w, C& codes)
{
  for (int l = 0; l <= kMaxBits; ++l)
    w.count[l] = 0;
  for (int i = 0; i < n; ++i)
    ++w.count[lens[i]];
  w.count[0] = 0;
  uint32_t code = 0;
  w.next[0] = 0;
  for (int l = 1; l <= kMaxBits; ++l) {
    code = (code + w.count[l - 1]) << 1;
    w.next[l] = (uint16_t)code;
  }
  for (int i = 0; i < n; ++i) {
    const uint32_t l = lens[i];
    codes[i] = (uint16_t)(l != 0u ? reverse_bits(w.next[l]++, l) : 0u);
  }
}

// ---- the header of a dynamic block -------------------------------------------------------------------------------
template <class L>
constexpr int trimmed_hlit(const L& lit_lens)
{
  int n = kMaxLitLen;
  while (n > 257 && lit_lens[n - 1] == 0)
    --n;
  return n;
}
template <class L>
constexpr int trimmed_hdist(const L& dist_lens)
{
  int n = kMaxDist;
  while (n > 1 && dist_lens[n - 1] == 0)
    --n;
  return n;
}
template <class L>
constexpr int trimmed_hclen(const L& cl_lens)
{
  int n = kNumCodeLen;
  while (n > 4 && cl_lens[kCodeLenOrder[n - 1]] == 0)
    --n;
  return n;
}

// lit_lens[0, hlit) followed by dist_lens[0, hdist) as run-length symbols: syms[k] = symbol | value of its extra
// bits << 8; cl_freq[0, 19) counts them.  -> number of symbols (at most hlit + hdist)
template <class L, class D, class S, class F>
constexpr int code_length_stream(const L& lit_lens, int hlit, const D& dist_lens, int hdist, S& syms, F& cl_freq)
{
  for (int s = 0; s < kNumCodeLen; ++s)
    cl_freq[s] = 0;
  const int total = hlit + hdist;
  int out = 0, i = 0;
  while (i < total) {
    const uint32_t v = i < hlit ? lit_lens[i] : dist_lens[i - hlit];
    int run = 1;
    while (i + run < total && (i + run < hlit ? lit_lens[i + run] : dist_lens[i + run - hlit]) == v)
      ++run;
    i += run;
    if (v != 0u) { // the length itself, then repeats of it
      syms[out++] = (uint16_t)v;
      ++cl_freq[v];
      --run;
    }
    while (run >= 3) {
      const int most = v != 0u ? 6 : 138;
      const int take = run < most ? run : most;
      const uint32_t sym = v != 0u ? 16u : take <= 10 ? 17u : 18u;
      syms[out++] = (uint16_t)(sym | (uint32_t)(take - (sym == 18u ? 11 : 3)) << 8);
      ++cl_freq[sym];
      run -= take;
    }
    for (; run > 0; --run) {
      syms[out++] = (uint16_t)v;
      ++cl_freq[v];
    }
  }
  return out;
}

// The code of the code-length alphabet has to be complete: a lone symbol gets a partner of one bit.
template <class F, class L>
constexpr void build_code_length_lengths(const F& cl_freq, HuffWork& w, L& cl_lens)
{
  build_lengths(cl_freq, kNumCodeLen, kCodeLenMaxBits, w, cl_lens, true);
}

// ---- exact costs in bits, the block's 3 header bits included -----------------------------------------------------
template <class F, class D, class L, class M>
constexpr uint32_t symbols_cost(const F& lit_freq, const D& dist_freq, const L& lit_len_of, const M& dist_len_of)
{
  uint32_t bits = 0;
  for (uint32_t s = 0; s < (uint32_t)kMaxLitLen; ++s)
    bits += lit_freq[s] * (lit_len_of(s) + (s > 256u ? length_extra(s - 257u) : 0u));
  for (uint32_t s = 0; s < (uint32_t)kMaxDist; ++s)
    bits += dist_freq[s] * (dist_len_of(s) + dist_extra(s));
  return bits;
}

template <class F, class D, class L, class M, class CF, class CL>
constexpr uint32_t dynamic_cost(const F& lit_freq, const D& dist_freq, const L& lit_lens, const M& dist_lens,
                                const CF& cl_freq, const CL& cl_lens, int hclen)
{
  uint32_t bits = 3u + 5u + 5u + 4u + 3u * (uint32_t)hclen;
  for (uint32_t s = 0; s < (uint32_t)kNumCodeLen; ++s)
    bits += cl_freq[s] * (cl_lens[s] + code_len_extra_bits(s));
  return bits + symbols_cost(lit_freq, dist_freq, [&](uint32_t s) { return (uint32_t)lit_lens[s]; },
                             [&](uint32_t s) { return (uint32_t)dist_lens[s]; });
}

template <class F, class D>
constexpr uint32_t fixed_cost(const F& lit_freq, const D& dist_freq)
{
  return 3u + symbols_cost(lit_freq, dist_freq, [](uint32_t s) { return fixed_litlen_length(s); },
                           [](uint32_t) { return kFixedDistLength; });
}

// n bytes as stored blocks of at most 65535 bytes: 3 header bits, padding to the byte, LEN and NLEN per block
constexpr uint32_t stored_blocks(uint32_t n) { return n == 0u ? 1u : (n + kStoredBlockMax - 1u) / kStoredBlockMax; }
constexpr uint32_t stored_bytes(uint32_t n) { return n + 5u * stored_blocks(n); }
constexpr uint32_t stored_cost(uint32_t n) { return 8u * stored_bytes(n); }

enum BlockKind { kStored = 0, kFixed = 1, kDynamic = 2 };

// the smallest; a tie goes to the simpler kind
constexpr BlockKind choose_block(uint32_t stored_bits, uint32_t fixed_bits, uint32_t dynamic_bits)
{
  if (stored_bits <= fixed_bits && stored_bits <= dynamic_bits)
    return kStored;
  return fixed_bits <= dynamic_bits ? kFixed : kDynamic;
}

// BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN and the lengths of the code-length code; put(bits, count), count <= 16
template <class Put, class CL>
constexpr void put_dynamic_header(Put&& put, int hlit, int hdist, int hclen, const CL& cl_lens)
{
  put(1u | (2u << 1), 3u);
  put((uint32_t)(hlit - 257), 5u);
  put((uint32_t)(hdist - 1), 5u);
  put((uint32_t)(hclen - 4), 4u);
  for (int k = 0; k < hclen; ++k)
    put((uint32_t)cl_lens[kCodeLenOrder[k]], 3u);
}

} // namespace deflate
} // namespace hcamd
