// zstd_codes.hpp -- the format logic of the Zstandard encoder (RFC 8878), free of HIP.
//
// Everything here is constexpr and plain C++17, as zstd_tables.hpp is for the decoder: the kernel
// (zstd_compress_kernels.hip) and the CPU driver (tests/zstd_codes_driver.cpp) include this one file, so what the
// tests prove about it on the CPU is what the GPU runs.  It holds
//
//   ll_code / ml_code / of_code, offset_value   lengths and offsets -> codes and extra bits (the inverse of kLLBase /
//                                               kMLBase of zstd_tables.hpp, held to them by a static_assert)
//   pick_log, normalize_counts                  histogram -> accuracy log and normalised counts
//   write_ncount                                the table description, the inverse of read_ncount
//   fse_build_ctable, fse_init, fse_encode      the encoding table (the spread of fse_build) and one state step
//   log2_fix8, fse_cost_fix8                    the estimated cost of a histogram under a distribution
//   plan_table                                  one of LL / OF / ML: RLE, predefined or described, table and header
//   huf_weights_of, huf_codes_of                Huffman lengths -> weights -> canonical codes in the format's order
//   write_weights_direct / write_weights_fse    the two descriptions of a tree
//   plan_huffman, choose_literals               the tree of a literal histogram and the literals section's form
//   write_literals_header, write_seq_count, write_block_header, write_frame_header
//   encode_frame                                all of it composed into a scalar encoder of a token list (the
//                                               driver's; the kernel walks the same steps 64 lanes wide)
//
// Byte sinks and tables are templates (anything indexable), so the kernel passes LDS and the driver plain arrays.
// No function here keeps an array of its own: work areas come from the caller (on the GPU they are LDS).
//
// Rules that the format leaves to an encoder, as this one sets them:
//   * Accuracy log (pick_log): two less than the bits of the symbol count, so that a table has about a quarter as
//     many states as there are symbols to code; not below 5 nor below one more than the bits of the number of used
//     symbols (every used symbol needs a state, and the rest of the states make the shares unequal); not above the
//     format's limit (9 / 8 / 9, 6 for weights).
//   * Normalisation (normalize_counts): every used symbol gets floor(count * 2^log / total), at least 1; what is
//     missing to 2^log goes to the most frequent symbol, what is too much is taken one at a time from the largest
//     share.  The "less than 1" probability is not used.
//   * Mode per table (plan_table): RLE where one code is used; otherwise the described table where its estimated
//     cost plus its description's exact bits is below the predefined table's estimated cost.
//   * Sequence count: one byte below 128, two bytes otherwise.  The three-byte form starts at 32512 sequences; a
//     chunk of at most 65536 bytes with matches of at least 4 bytes has at most 16384, so it cannot occur.
//   * Repeat_Mode and treeless literals need a block before this one in the frame; there is none.
#pragma once

#include <cstdint>

#include "deflate_codes.hpp"
#include "zstd_tables.hpp"

namespace hcamd {
namespace zstd {

constexpr uint32_t kEncMinMatch = 4;
constexpr uint32_t kEncMaxChunk = 65536;
constexpr uint32_t kEncMaxSequences = kEncMaxChunk / kEncMinMatch;
constexpr uint32_t kFrameOverhead = 14; // 4 magic + 1 descriptor + 2 content size + 3 block header + 4 checksum
constexpr uint32_t kWeightSymbols = 13; // weights 0 .. 12
constexpr uint32_t kWeightsDescMax = 127;
constexpr uint32_t kCostNever = 0xFFFFFFFFu;

constexpr uint32_t frame_bound(uint32_t n) { return n + kFrameOverhead; }

// ---- lengths and offsets -> codes ---------------------------------------------------------------------------------
constexpr uint32_t ll_code(uint32_t v)
{
  if (v < 16u)
    return v;
  if (v < 24u)
    return 16u + ((v - 16u) >> 1);
  if (v < 32u)
    return 20u + ((v - 24u) >> 2);
  if (v < 48u)
    return 22u + ((v - 32u) >> 3);
  if (v < 64u)
    return 24u;
  return highbit(v) + 19u;
}

constexpr uint32_t ml_code(uint32_t v) // v >= 3
{
  if (v < 35u)
    return v - 3u;
  if (v < 43u)
    return 32u + ((v - 35u) >> 1);
  if (v < 51u)
    return 36u + ((v - 43u) >> 2);
  if (v < 67u)
    return 38u + ((v - 51u) >> 3);
  if (v < 99u)
    return 40u + ((v - 67u) >> 4);
  if (v < 131u)
    return 42u;
  return highbit(v - 3u) + 36u;
}

constexpr bool codes_invert_the_tables()
{
  for (uint32_t c = 0; c < 36u; ++c)
    if (ll_code(kLLBase[c]) != c || ll_code(kLLBase[c] + (1u << kLLBits[c]) - 1u) != c)
      return false;
  for (uint32_t c = 0; c < 53u; ++c)
    if (ml_code(kMLBase[c]) != c || ml_code(kMLBase[c] + (1u << kMLBits[c]) - 1u) != c)
      return false;
  return true;
}
static_assert(codes_invert_the_tables(), "ll_code / ml_code disagree with kLLBase / kMLBase");

// Offset_Value of a sequence: 1 -- the first repeat offset -- where the sequence has literals and uses the offset
// of the sequence before it (prev_off: 0 for the first sequence), offset + 3 otherwise.  After any sequence coded
// so, the offset it used is the first repeat offset, whichever of the two it was.
constexpr uint32_t offset_value(uint32_t off, uint32_t prev_off, uint32_t ll, bool repeat_codes = true)
{
  return repeat_codes && ll != 0u && off == prev_off ? 1u : off + 3u;
}
// its code is its highest bit, the extra bits are the bits below it
constexpr uint32_t of_code(uint32_t value) { return highbit(value); }

// ---- sinks ---------------------------------------------------------------------------------------------------------
struct NullSink
{
  constexpr void operator()(uint32_t, uint8_t) const {}
};
template <class P>
struct ByteSink
{
  P p;
  constexpr void operator()(uint32_t at, uint8_t b) const { p[at] = b; }
};

// bits appended lowest first, bytes leave through sink(at, byte)
template <class S>
struct BitAppender
{
  S sink;
  uint32_t at;  // next byte
  uint64_t acc;
  uint32_t n;   // bits in acc, < 8 between calls

  constexpr void add(uint32_t v, uint32_t nbits) // nbits <= 32
  {
    acc |= (uint64_t)v << n;
    n += nbits;
    while (n >= 8u) {
      sink(at++, (uint8_t)acc);
      acc >>= 8;
      n -= 8u;
    }
  }
  constexpr uint32_t bits() const { return 8u * at + n; }
  constexpr uint32_t close_forward() // a forward stream: pad to the byte
  {
    if (n)
      sink(at++, (uint8_t)acc);
    acc = 0;
    n = 0;
    return at;
  }
  constexpr uint32_t close_backward() // a backward stream: the final-bit marker, then pad
  {
    add(1u, 1u);
    return close_forward();
  }
};

// ---- accuracy log and normalisation ---------------------------------------------------------------------------------
constexpr uint32_t ceil_log2(uint32_t v) { return v <= 1u ? 0u : highbit(v - 1u) + 1u; }

constexpr uint32_t pick_log(uint32_t total, uint32_t nused, uint32_t max_log)
{
  const uint32_t bits = ceil_log2(total);
  uint32_t log = bits > 2u ? bits - 2u : 0u;
  uint32_t lo = ceil_log2(nused) + 1u;
  lo = lo < 5u ? 5u : lo;
  lo = lo > max_log ? max_log : lo;
  log = log < lo ? lo : log;
  return log > max_log ? max_log : log;
}

// hist[0, nsym) with sum `total` and at most 2^log used symbols -> norm[0, nsym) with sum 2^log, every used
// symbol >= 1.  -> the number of used symbols
template <class H, class N>
constexpr uint32_t normalize_counts(const H& hist, uint32_t nsym, uint32_t total, uint32_t log, N& norm)
{
  const uint32_t size = 1u << log;
  uint32_t used = 0, sum = 0, big = 0, big_count = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const uint32_t h = hist[s];
    uint32_t c = 0;
    if (h) {
      c = (h << log) / total; // (h <= 2^14 and log <= 9)
      c = c ? c : 1u;
      ++used;
      if (h > big_count) {
        big_count = h;
        big = s;
      }
    }
    norm[s] = (int16_t)c;
    sum += c;
  }
  if (sum <= size) {
    norm[big] = (int16_t)(norm[big] + (int32_t)(size - sum));
    return used;
  }
  for (; sum > size; --sum) { // too many shares of 1: take from the largest, the lowest symbol among equals
    uint32_t at = 0;
    for (uint32_t s = 1; s < nsym; ++s)
      if (norm[s] > norm[at])
        at = s;
    norm[at] = (int16_t)(norm[at] - 1);
  }
  return used;
}

// ---- the table description (4.1.1), the mirror of read_ncount -------------------------------------------------------
// norm[0, nsym) with sum 2^log (a -1 counts 1) -> the description's bits; bytes through sink(at0 + k, byte)
template <class N, class S>
constexpr uint32_t write_ncount(const N& norm, uint32_t log, S sink, uint32_t at0)
{
  BitAppender<S> w{sink, at0, 0, 0};
  w.add(log - 5u, 4u);
  int32_t remaining = (1 << log) + 1, threshold = 1 << log;
  uint32_t nb = log + 1u, sym = 0;
  bool prev0 = false;
  while (remaining > 1) {
    if (prev0) {
      uint32_t run = 0;
      while (norm[sym + run] == 0)
        ++run;
      sym += run;
      for (; run >= 3u; run -= 3u)
        w.add(3u, 2u);
      w.add(run, 2u);
    }
    const int32_t count = norm[sym++];
    const int32_t mx = (2 * threshold - 1) - remaining;
    remaining -= count < 0 ? -count : count;
    int32_t v = count + 1;
    if (v >= threshold)
      v += mx;
    w.add((uint32_t)v, nb - (v < mx ? 1u : 0u));
    prev0 = count == 0;
    while (remaining < threshold) {
      nb -= 1u;
      threshold >>= 1;
    }
  }
  const uint32_t bits = w.bits() - 8u * at0;
  w.close_forward();
  return bits;
}

// ---- the FSE encoding table -------------------------------------------------------------------------------------------
struct FseSym
{
  uint32_t delta_nbits;
  int32_t delta_state;
};

// norm[0, nsym) -> symtt[0, nsym), states[0, 2^log): states[] lists, symbol by symbol, the table positions (plus
// 2^log) of that symbol in rising order.  The spread is fse_build's.  spread (bytes, 2^log) and cumul (16-bit,
// nsym + 1) are scratch.
template <class N, class Y, class T, class B, class C>
constexpr void fse_build_ctable(const N& norm, uint32_t nsym, uint32_t log, Y& symtt, T& states, B& spread, C& cumul)
{
  const uint32_t size = 1u << log, mask = size - 1u;
  uint32_t high = size - 1u;
  cumul[0] = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    if (norm[s] == -1) {
      cumul[s + 1u] = (uint16_t)(cumul[s] + 1u);
      spread[high--] = (uint8_t)s;
    } else {
      cumul[s + 1u] = (uint16_t)(cumul[s] + (uint32_t)norm[s]);
    }
  }
  const uint32_t step = (size >> 1) + (size >> 3) + 3u;
  uint32_t pos = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const int32_t c = norm[s];
    for (int32_t i = 0; i < c; ++i) {
      spread[pos] = (uint8_t)s;
      do
        pos = (pos + step) & mask;
      while (pos > high);
    }
  }
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t s = spread[u];
    states[cumul[s]] = (uint16_t)(size + u);
    cumul[s] = (uint16_t)(cumul[s] + 1u);
  }
  uint32_t total = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const int32_t c = norm[s];
    if (c == 0) {
      symtt[s].delta_nbits = ((log + 1u) << 16) - size;
      symtt[s].delta_state = 0;
    } else if (c == -1 || c == 1) {
      symtt[s].delta_nbits = (log << 16) - size;
      symtt[s].delta_state = (int32_t)total - 1;
      total += 1u;
    } else {
      const uint32_t max_bits = log - highbit((uint32_t)c - 1u);
      symtt[s].delta_nbits = (max_bits << 16) - ((uint32_t)c << max_bits);
      symtt[s].delta_state = (int32_t)total - c;
      total += (uint32_t)c;
    }
  }
}

// an RLE table: one symbol, no state bits (fse_init and fse_encode then leave state 0 and ask for 0 bits)
template <class Y, class T>
constexpr void fse_build_ctable_rle(Y& symtt, T& states, uint32_t sym)
{
  symtt[sym].delta_nbits = 0;
  symtt[sym].delta_state = 0;
  states[0] = 0;
}

// the state that codes `sym` as the last symbol of a chain: the one that leaves the decoder the most bits to read
template <class Y, class T>
constexpr uint32_t fse_init(const Y& symtt, const T& states, uint32_t sym)
{
  const uint32_t d = symtt[sym].delta_nbits;
  const uint32_t nb = (d + (1u << 15)) >> 16;
  const uint32_t value = (nb << 16) - d;
  return states[(int32_t)(value >> nb) + symtt[sym].delta_state];
}

// one step: -> (bits | count << 16), the state moves on
template <class Y, class T>
constexpr uint32_t fse_encode(const Y& symtt, const T& states, uint32_t& state, uint32_t sym)
{
  const uint32_t nb = (state + symtt[sym].delta_nbits) >> 16;
  const uint32_t out = (state & ((1u << nb) - 1u)) | (nb << 16);
  state = states[(int32_t)(state >> nb) + symtt[sym].delta_state];
  return out;
}

// ---- the cost estimate --------------------------------------------------------------------------------------------------
// floor(256 * log2(x)) by repeated squaring, x >= 1
constexpr uint32_t log2_fix8(uint32_t x)
{
  const uint32_t h = highbit(x);
  uint64_t m = ((uint64_t)x << 16) >> h; // [1, 2) in 16.16
  uint32_t r = h << 8;
  for (int b = 7; b >= 0; --b) {
    m = (m * m) >> 16;
    if (m >= (2ull << 16)) {
      m >>= 1;
      r |= 1u << b;
    }
  }
  return r;
}

// sum of hist[s] * (log - log2 norm[s]) in 1/256 bit; kCostNever where a used symbol has no share
template <class H, class N>
constexpr uint32_t fse_cost_fix8(const H& hist, uint32_t nsym, const N& norm, uint32_t norm_syms, uint32_t log)
{
  uint32_t cost = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const uint32_t h = hist[s];
    if (!h)
      continue;
    const int32_t c = s < norm_syms ? (int32_t)norm[s] : 0;
    if (c == 0)
      return kCostNever;
    cost += h * ((log << 8) - log2_fix8(c < 0 ? 1u : (uint32_t)c));
  }
  return cost;
}

constexpr uint32_t default_cost_fix8_probe() // (a fixed figure the tests restate)
{
  uint32_t hist[36] = {};
  for (uint32_t s = 0; s < 36u; ++s)
    hist[s] = s + 1u;
  return fse_cost_fix8(hist, 36u, kLLDefault, 36u, kLLDefaultLog);
}

// ---- one of the three tables -----------------------------------------------------------------------------------------------
enum TableKind { kLLTable = 0, kOFTable = 1, kMLTable = 2 };
constexpr uint32_t kTableSyms[3] = {36, 32, 53};
constexpr uint32_t kTableMaxLog[3] = {kLLLogMax, kOFLogMax, kMLLogMax};
constexpr uint32_t kTableDefaultLog[3] = {kLLDefaultLog, kOFDefaultLog, kMLDefaultLog};
constexpr uint32_t kTableDefaultSyms[3] = {36, 29, 53};
constexpr uint32_t kMaxTableSyms = 53, kMaxTableStates = 512;

struct FseScratch
{
  int16_t norm[64];
  uint16_t cumul[64];
  uint8_t spread[kMaxTableStates];
};

struct TablePlan
{
  uint32_t mode, log, head_bytes; // head_bytes: what the table adds behind the modes byte
};

// hist[0, kTableSyms[kind]) of `total` sequences -> the mode, the encoding table, and the table's bytes of the
// sequences header through sink(at0 + k, byte)
template <class H, class Y, class T, class S>
constexpr TablePlan plan_table(uint32_t kind, const H& hist, uint32_t total, Y& symtt, T& states, FseScratch& w, S sink, uint32_t at0)
{
  const uint32_t nsym = kTableSyms[kind];
  uint32_t used = 0, only = 0;
  for (uint32_t s = 0; s < nsym; ++s)
    if (hist[s]) {
      ++used;
      only = s;
    }
  if (used == 1u) {
    fse_build_ctable_rle(symtt, states, only);
    sink(at0, (uint8_t)only);
    return TablePlan{kRleMode, 0u, 1u};
  }
  const uint32_t dlog = kTableDefaultLog[kind], dsyms = kTableDefaultSyms[kind];
  const uint32_t dcost = kind == kLLTable   ? fse_cost_fix8(hist, nsym, kLLDefault, dsyms, dlog)
                         : kind == kOFTable ? fse_cost_fix8(hist, nsym, kOFDefault, dsyms, dlog)
                                            : fse_cost_fix8(hist, nsym, kMLDefault, dsyms, dlog);
  const uint32_t log = pick_log(total, used, kTableMaxLog[kind]);
  normalize_counts(hist, nsym, total, log, w.norm);
  const uint32_t own = fse_cost_fix8(hist, nsym, w.norm, nsym, log);
  const uint32_t desc_bits = write_ncount(w.norm, log, NullSink{}, 0u);
  if (dcost != kCostNever && dcost <= own + (desc_bits << 8)) {
    for (uint32_t s = 0; s < nsym; ++s)
      w.norm[s] = (int16_t)(s >= dsyms ? 0 : kind == kLLTable ? kLLDefault[s] : kind == kOFTable ? kOFDefault[s] : kMLDefault[s]);
    fse_build_ctable(w.norm, nsym, dlog, symtt, states, w.spread, w.cumul);
    return TablePlan{kPredefined, dlog, 0u};
  }
  fse_build_ctable(w.norm, nsym, log, symtt, states, w.spread, w.cumul);
  write_ncount(w.norm, log, sink, at0);
  return TablePlan{kFseMode, log, (desc_bits + 7u) >> 3};
}

// ---- Huffman ---------------------------------------------------------------------------------------------------------------
// lens[0, 256) (0: no code, else 1 .. 11) -> weights[0, 256); -> (last present symbol) | (table log << 16)
template <class L, class W>
constexpr uint32_t huf_weights_of(const L& lens, W& weights)
{
  uint32_t log = 0, last = 0;
  for (uint32_t s = 0; s < 256u; ++s)
    if (lens[s]) {
      last = s;
      log = lens[s] > log ? lens[s] : log;
    }
  for (uint32_t s = 0; s < 256u; ++s)
    weights[s] = (uint8_t)(lens[s] ? log + 1u - lens[s] : 0u);
  return last | (log << 16);
}

// weights[0, 256) -> table[s] = code | bits << 16, the code as the stream takes it (its first bit the highest): the
// decoding table's order, by weight, then by symbol, the lightest first
struct HufRanks
{
  uint32_t count[16], start[16];
};

template <class W, class T>
constexpr void huf_codes_of(const W& weights, uint32_t log, T& table, HufRanks& r)
{
  for (uint32_t w = 0; w < 16u; ++w)
    r.count[w] = r.start[w] = 0;
  for (uint32_t s = 0; s < 256u; ++s)
    r.count[weights[s]] += 1u;
  uint32_t at = 0;
  for (uint32_t w = 1; w <= log; ++w) {
    r.start[w] = at;
    at += r.count[w] << (w - 1u);
  }
  for (uint32_t s = 0; s < 256u; ++s) {
    const uint32_t w = weights[s];
    if (w) {
      table[s] = (r.start[w] >> (w - 1u)) | ((log + 1u - w) << 16);
      r.start[w] += 1u << (w - 1u);
    } else {
      table[s] = 0;
    }
  }
}

// 4 bits a weight, the last present symbol's implied: -> bytes, 0 where the symbols do not fit the header byte
template <class W, class S>
constexpr uint32_t write_weights_direct(const W& weights, uint32_t last, S sink, uint32_t at0)
{
  if (last < 1u || last > 127u)
    return 0;
  sink(at0, (uint8_t)(127u + last));
  for (uint32_t i = 0; i < last; i += 2u)
    sink(at0 + 1u + i / 2u, (uint8_t)((weights[i] << 4) | (i + 1u < last ? weights[i + 1u] : 0u)));
  return 1u + (last + 1u) / 2u;
}

struct WeightScratch
{
  uint32_t hist[16];
  FseSym symtt[16];
  uint16_t states[1u << kWeightLogMax];
  FseScratch fse;
};

// FSE-compressed with two interleaved states, symbol k by state k % 2: -> bytes with the header byte, 0 where
// there is no such description (fewer than 2 weights, one weight value only) or it passes 127 bytes.  `limit`
// stands in for 127 in the tests of that refusal.
template <class W, class S>
constexpr uint32_t write_weights_fse(const W& weights, uint32_t last, WeightScratch& w, S sink, uint32_t at0,
                                     uint32_t limit = kWeightsDescMax)
{
  if (last < 2u)
    return 0;
  for (uint32_t s = 0; s < 16u; ++s)
    w.hist[s] = 0;
  for (uint32_t i = 0; i < last; ++i)
    w.hist[weights[i]] += 1u;
  uint32_t used = 0;
  for (uint32_t s = 0; s < kWeightSymbols; ++s)
    used += w.hist[s] != 0u;
  if (used < 2u)
    return 0;
  const uint32_t log = pick_log(last, used, kWeightLogMax);
  normalize_counts(w.hist, kWeightSymbols, last, log, w.fse.norm);
  fse_build_ctable(w.fse.norm, kWeightSymbols, log, w.symtt, w.states, w.fse.spread, w.fse.cumul);
  // (sized first: nothing may pass the sink's room)
  uint32_t bits = write_ncount(w.fse.norm, log, NullSink{}, 0u);
  const uint32_t nc_bytes = (bits + 7u) >> 3;
  {
    uint32_t even = 0, odd = 0, body = 2u * log + 1u;
    for (uint32_t k = last; k-- > 0u;) {
      uint32_t st = (k & 1u) ? odd : even;
      if (k + 2u >= last)
        st = fse_init(w.symtt, w.states, weights[k]);
      else
        body += fse_encode(w.symtt, w.states, st, weights[k]) >> 16;
      if (k & 1u)
        odd = st;
      else
        even = st;
    }
    if (nc_bytes + ((body + 7u) >> 3) > limit)
      return 0;
  }
  write_ncount(w.fse.norm, log, sink, at0 + 1u);
  BitAppender<S> b{sink, at0 + 1u + nc_bytes, 0, 0};
  uint32_t even = 0, odd = 0;
  for (uint32_t k = last; k-- > 0u;) {
    uint32_t st = (k & 1u) ? odd : even;
    if (k + 2u >= last) {
      st = fse_init(w.symtt, w.states, weights[k]);
    } else {
      const uint32_t e = fse_encode(w.symtt, w.states, st, weights[k]);
      b.add(e & 0xFFFFu, e >> 16);
    }
    if (k & 1u)
      odd = st;
    else
      even = st;
  }
  b.add(odd & ((1u << log) - 1u), log);
  b.add(even & ((1u << log) - 1u), log);
  const uint32_t end = b.close_backward();
  sink(at0, (uint8_t)(end - at0 - 1u));
  return end - at0;
}

// The tree's description, the shorter of the two forms (a tie goes to the direct one): -> bytes, 0 where neither
// exists.  desc: room for 1 + 128 bytes.
template <class W, class S>
constexpr uint32_t write_weights(const W& weights, uint32_t last, WeightScratch& w, S sink, uint32_t at0)
{
  const uint32_t direct = write_weights_direct(weights, last, NullSink{}, 0u);
  const uint32_t fse = write_weights_fse(weights, last, w, NullSink{}, 0u);
  if (direct != 0u && (fse == 0u || direct <= fse))
    return write_weights_direct(weights, last, sink, at0);
  if (fse != 0u)
    return write_weights_fse(weights, last, w, sink, at0);
  return 0;
}

// ---- the literals section ----------------------------------------------------------------------------------------------------
constexpr uint32_t raw_literals_header_bytes(uint32_t n) { return n < 32u ? 1u : n < 4096u ? 2u : 3u; }

struct LiteralsPlan
{
  uint32_t type;         // kRawLit, kRleLit, kHufLit
  uint32_t streams;      // 1 or 4 (Huffman)
  uint32_t header_bytes;
  uint32_t section_bytes; // with the header
};

// stream_bits[k]: the code bits of stream k (the four quarters of (n + 3) / 4 literals, or all of them in
// stream_bits[0] .. [3] summed for one stream); desc_bytes: the tree's description, 0 where there is none (no
// tree, or fewer than 2 symbols).  By exact size; a tie goes raw, then RLE.  One stream where both sizes fit the
// 10-bit header, four otherwise; force_four (the tests') asks for four where one would do.
constexpr uint32_t huf_stream_bytes(uint32_t bits) { return (bits >> 3) + 1u; } // the marker bit, then to the byte

constexpr LiteralsPlan choose_literals(uint32_t n, bool all_equal, uint32_t desc_bytes, const uint32_t stream_bits[4],
                                       bool force_four = false)
{
  LiteralsPlan raw{kRawLit, 1u, raw_literals_header_bytes(n), raw_literals_header_bytes(n) + n};
  LiteralsPlan best = raw;
  if (all_equal && n >= 2u) {
    const LiteralsPlan rle{kRleLit, 1u, raw.header_bytes, raw.header_bytes + 1u};
    if (rle.section_bytes < best.section_bytes)
      best = rle;
  }
  if (desc_bytes != 0u && n >= 2u) {
    const uint32_t one = desc_bytes + huf_stream_bytes(stream_bits[0] + stream_bits[1] + stream_bits[2] + stream_bits[3]);
    LiteralsPlan huf{kHufLit, 1u, 3u, 3u + one};
    if (n >= 1024u || one >= 1024u || force_four) {
      // four streams need at least 6 literals for their quarters; here n >= 1024 or the single stream is long
      const uint32_t four = desc_bytes + 6u + huf_stream_bytes(stream_bits[0]) + huf_stream_bytes(stream_bits[1])
                            + huf_stream_bytes(stream_bits[2]) + huf_stream_bytes(stream_bits[3]);
      const uint32_t m = n > four ? n : four;
      huf.streams = 4u;
      huf.header_bytes = m < 1024u ? 3u : m < 16384u ? 4u : 5u;
      huf.section_bytes = huf.header_bytes + four;
      if (m >= (1u << 18) || n < 6u)
        huf.section_bytes = 0xFFFFFFFFu;
    }
    if (huf.section_bytes < best.section_bytes)
      best = huf;
  }
  return best;
}

// -> header bytes written.  comp: the bytes behind the header (Huffman only)
template <class S>
constexpr uint32_t write_literals_header(const LiteralsPlan& p, uint32_t n, S sink, uint32_t at0)
{
  if (p.type != kHufLit) {
    const uint32_t hb = p.header_bytes;
    const uint32_t v = hb == 1u ? (n << 3) | p.type : hb == 2u ? (n << 4) | (1u << 2) | p.type : (n << 4) | (3u << 2) | p.type;
    for (uint32_t b = 0; b < hb; ++b)
      sink(at0 + b, (uint8_t)(v >> (8u * b)));
    return hb;
  }
  const uint32_t hb = p.header_bytes, bits = hb == 3u ? 10u : hb == 4u ? 14u : 18u;
  const uint32_t sf = p.streams == 1u ? 0u : hb - 2u;
  const uint64_t comp = p.section_bytes - hb;
  const uint64_t v = (uint64_t)kHufLit | (sf << 2) | ((uint64_t)n << 4) | (comp << (4u + bits));
  for (uint32_t b = 0; b < hb; ++b)
    sink(at0 + b, (uint8_t)(v >> (8u * b)));
  return hb;
}

// ---- sequences, block and frame headers --------------------------------------------------------------------------------------------
template <class S>
constexpr uint32_t write_seq_count(uint32_t nseq, S sink, uint32_t at0) // nseq < 32512
{
  if (nseq < 128u) {
    sink(at0, (uint8_t)nseq);
    return 1;
  }
  sink(at0, (uint8_t)(128u + (nseq >> 8)));
  sink(at0 + 1u, (uint8_t)nseq);
  return 2;
}

template <class S>
constexpr uint32_t write_block_header(uint32_t type, uint32_t size, S sink, uint32_t at0) // the last block
{
  const uint32_t v = 1u | (type << 1) | (size << 3);
  sink(at0, (uint8_t)v);
  sink(at0 + 1u, (uint8_t)(v >> 8));
  sink(at0 + 2u, (uint8_t)(v >> 16));
  return 3;
}

constexpr uint32_t frame_header_bytes(uint32_t n) { return n < 256u ? 6u : 7u; }

// magic, Single_Segment with the content size in 1 byte (n <= 255) or 2 (256 .. 65536), no dictionary
template <class S>
constexpr uint32_t write_frame_header(uint32_t n, bool checksum, S sink, uint32_t at0)
{
  for (uint32_t b = 0; b < 4u; ++b)
    sink(at0 + b, (uint8_t)(kMagic >> (8u * b)));
  const bool two = n >= 256u;
  sink(at0 + 4u, (uint8_t)((two ? 1u << 6 : 0u) | (1u << 5) | (checksum ? 1u << 2 : 0u)));
  if (!two) {
    sink(at0 + 5u, (uint8_t)n);
    return 6;
  }
  sink(at0 + 5u, (uint8_t)(n - 256u));
  sink(at0 + 6u, (uint8_t)((n - 256u) >> 8));
  return 7;
}

// ---- the scalar encoder ----------------------------------------------------------------------------------------------------------------
struct Token
{
  uint32_t ll, ml, off; // literals, then a match of ml >= 3 bytes at offset off; the literals behind the last match are not a token
};

struct EncodeWork
{
  uint32_t lit_hist[256];
  uint8_t lens[256], weights[256];
  uint32_t huf[256];
  deflate::HuffWork huff;
  HufRanks ranks;
  WeightScratch wscratch;
  uint32_t code_hist[3][64];
  FseSym symtt[3][64];
  uint16_t states[3][kMaxTableStates];
  FseScratch fse;
  uint8_t desc[132];
  uint8_t seq_head[400];
};

// content[0, n) as one frame through out[]: tokens[0, ntok) cover the content but for the literals behind the
// last match; lits[0, nlit) are the content's literal bytes in order.  -> the frame's bytes, never more than
// frame_bound(n).  block[]: room for n bytes, where the compressed block is built before it is known to be shorter.
// The three knobs are the tests': repeat_codes = false writes every offset as offset + 3, force_four takes four
// Huffman streams where one would do, rle_block = false leaves the RLE_Block out of the block choice (the only
// way to RLE literals: literals that are all one byte make a content that is all one byte).
template <class C, class K, class L, class B, class O>
constexpr uint32_t encode_frame(const C& content, uint32_t n, const K& tokens, uint32_t ntok, const L& lits, uint32_t nlit,
                                bool checksum, bool repeat_codes, bool force_four, bool rle_block, EncodeWork& w, B& block, O& out)
{
  ByteSink<O&> os{out};
  uint32_t at = write_frame_header(n, checksum, os, 0u);
  bool all_equal = rle_block && n >= 2u;
  for (uint32_t i = 1; i < n && all_equal; ++i)
    all_equal = content[i] == content[0];
  uint32_t block_bytes = 0xFFFFFFFFu;
  if (!all_equal && n > 3u) {
    ByteSink<B&> bs{block};
    // (the block is abandoned where it reaches n bytes; `room` keeps every write inside block[0, n))
    auto fits = [&](uint32_t end) { return end < n; };
    // literals
    for (uint32_t s = 0; s < 256u; ++s)
      w.lit_hist[s] = 0;
    for (uint32_t i = 0; i < nlit; ++i)
      w.lit_hist[lits[i]] += 1u;
    uint32_t used = 0;
    for (uint32_t s = 0; s < 256u; ++s)
      used += w.lit_hist[s] != 0u;
    uint32_t desc_bytes = 0, stream_bits[4] = {0, 0, 0, 0};
    const uint32_t seg = (nlit + 3u) / 4u;
    if (used >= 2u) {
      deflate::build_lengths(w.lit_hist, 256, (int)kHufLogMax, w.huff, w.lens);
      const uint32_t ll = huf_weights_of(w.lens, w.weights);
      huf_codes_of(w.weights, ll >> 16, w.huf, w.ranks);
      desc_bytes = write_weights(w.weights, ll & 0xFFFFu, w.wscratch, ByteSink<uint8_t*>{w.desc}, 0u);
      for (uint32_t i = 0; i < nlit; ++i)
        stream_bits[i / seg] += w.huf[lits[i]] >> 16;
    }
    const LiteralsPlan lp = choose_literals(nlit, used == 1u, desc_bytes, stream_bits, force_four);
    bool ok = fits(lp.section_bytes);
    uint32_t b = 0;
    if (ok) {
      b = write_literals_header(lp, nlit, bs, 0u);
      if (lp.type == kRawLit) {
        for (uint32_t i = 0; i < nlit; ++i)
          bs(b++, lits[i]);
      } else if (lp.type == kRleLit) {
        bs(b++, lits[0]);
      } else {
        for (uint32_t i = 0; i < desc_bytes; ++i)
          bs(b++, w.desc[i]);
        const uint32_t nstreams = lp.streams;
        const uint32_t jump = b;
        if (nstreams == 4u)
          b += 6u;
        for (uint32_t k = 0; k < nstreams; ++k) {
          const uint32_t from = nstreams == 1u ? 0u : k * seg;
          const uint32_t to = nstreams == 1u ? nlit : (k == 3u ? nlit : (k + 1u) * seg);
          BitAppender<ByteSink<B&>> ba{bs, b, 0, 0};
          for (uint32_t i = to; i-- > from;)
            ba.add(w.huf[lits[i]] & 0xFFFFu, w.huf[lits[i]] >> 16);
          const uint32_t end = ba.close_backward();
          if (nstreams == 4u && k < 3u) {
            bs(jump + 2u * k, (uint8_t)(end - b));
            bs(jump + 2u * k + 1u, (uint8_t)((end - b) >> 8));
          }
          b = end;
        }
      }
    }
    // sequences
    if (ok && ntok == 0u) {
      bs(b++, 0);
    } else if (ok) {
      for (uint32_t t = 0; t < 3u; ++t)
        for (uint32_t s = 0; s < 64u; ++s)
          w.code_hist[t][s] = 0;
      uint32_t prev = 0;
      for (uint32_t i = 0; i < ntok; ++i) {
        w.code_hist[kLLTable][ll_code(tokens[i].ll)] += 1u;
        w.code_hist[kOFTable][of_code(offset_value(tokens[i].off, prev, tokens[i].ll, repeat_codes))] += 1u;
        w.code_hist[kMLTable][ml_code(tokens[i].ml)] += 1u;
        prev = tokens[i].off;
      }
      ByteSink<uint8_t*> hs{w.seq_head};
      uint32_t h = write_seq_count(ntok, hs, 0u);
      const uint32_t modes_at = h++;
      TablePlan tp[3] = {};
      for (uint32_t t = 0; t < 3u; ++t) {
        tp[t] = plan_table(t, w.code_hist[t], ntok, w.symtt[t], w.states[t], w.fse, hs, h);
        h += tp[t].head_bytes;
      }
      hs(modes_at, (uint8_t)((tp[0].mode << 6) | (tp[1].mode << 4) | (tp[2].mode << 2)));
      ok = fits(b + h);
      if (ok) {
        for (uint32_t i = 0; i < h; ++i)
          bs(b++, w.seq_head[i]);
        // sized first, then written
        for (int pass = 0; pass < 2 && ok; ++pass) {
          uint32_t st[3] = {0, 0, 0}, bits = 0;
          BitAppender<ByteSink<B&>> ba{bs, b, 0, 0};
          for (uint32_t i = ntok; i-- > 0u;) {
            const uint32_t pv = i ? tokens[i - 1u].off : 0u;
            const uint32_t ov = offset_value(tokens[i].off, pv, tokens[i].ll, repeat_codes);
            const uint32_t code[3] = {ll_code(tokens[i].ll), of_code(ov), ml_code(tokens[i].ml)};
            uint32_t e[3] = {0, 0, 0};
            for (uint32_t t = 0; t < 3u; ++t) {
              if (i + 1u == ntok)
                st[t] = fse_init(w.symtt[t], w.states[t], code[t]);
              else
                e[t] = fse_encode(w.symtt[t], w.states[t], st[t], code[t]);
            }
            const uint32_t field[6][2] = {{e[1] & 0xFFFFu, e[1] >> 16}, {e[2] & 0xFFFFu, e[2] >> 16}, {e[0] & 0xFFFFu, e[0] >> 16},
                                          {tokens[i].ll - kLLBase[code[0]], kLLBits[code[0]]},
                                          {tokens[i].ml - kMLBase[code[2]], kMLBits[code[2]]},
                                          {ov - (1u << code[1]), code[1]}};
            for (uint32_t f = 0; f < 6u; ++f) {
              bits += field[f][1];
              if (pass)
                ba.add(field[f][0], field[f][1]);
            }
          }
          const uint32_t order[3] = {kMLTable, kOFTable, kLLTable};
          for (uint32_t f = 0; f < 3u; ++f) {
            const uint32_t t = order[f];
            bits += tp[t].log;
            if (pass)
              ba.add(st[t] & ((1u << tp[t].log) - 1u), tp[t].log);
          }
          if (!pass)
            ok = fits(b + (bits >> 3) + 1u);
          else
            b = ba.close_backward();
        }
      }
    }
    if (ok && b < n)
      block_bytes = b;
  }
  if (all_equal) {
    at += write_block_header(kRleBlock, n, os, at);
    os(at++, content[0]);
  } else if (block_bytes != 0xFFFFFFFFu) {
    at += write_block_header(kCompressedBlock, block_bytes, os, at);
    for (uint32_t i = 0; i < block_bytes; ++i)
      os(at++, block[i]);
  } else {
    at += write_block_header(kRawBlock, n, os, at);
    for (uint32_t i = 0; i < n; ++i)
      os(at++, content[i]);
  }
  if (checksum) {
    const uint32_t h = (uint32_t)xxh64(content, n, 0);
    for (uint32_t b = 0; b < 4u; ++b)
      os(at++, (uint8_t)(h >> (8u * b)));
  }
  return at;
}

} // namespace zstd
} // namespace hcamd
