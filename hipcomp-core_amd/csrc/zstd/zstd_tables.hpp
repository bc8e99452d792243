// zstd_tables.hpp -- the format logic of the Zstandard decoder (RFC 8878), free of HIP.
//
// Everything here is constexpr and plain C++17: the kernel (zstd_kernels.hip) and the CPU driver
// (tests/zstd_tables_driver.cpp) include this one file, so what the tests prove about it on the CPU is what the
// GPU runs.  It holds the header parsers (frame, block, literals section, sequences section; each reads only
// p[0, n)), the constant tables, the verdict on an FSE table description with its decoding table, the Huffman
// tree description with its decoding table, the backward bitstream, one sequence's decode with the repeat-offset
// rules, and (xxh64_math.hpp) the checksum.  The arbiter of every accept / refuse below is ZSTD_decompress of
// libzstd 1.4.8; where this decoder differs on purpose, include/hipcomp/zstd.h lists it.
//
// Byte sources are templates (`P`: anything indexable that yields bytes), so the kernel passes pointers into
// global memory or LDS and the driver plain pointers.  Table fills are functions of the entry index where the
// format allows (huf_entry); the FSE spread is serial in symbol order and is filled by one walk (fse_build).
#pragma once

#include <cstdint>

#include "xxh64_math.hpp"

namespace hcamd {
namespace zstd {

constexpr uint32_t kMagic = 0xFD2FB528u;
constexpr uint32_t kSkippableMagic = 0x184D2A50u; // .. 0x184D2A5F
constexpr uint32_t kBlockMax = 128u * 1024u;
constexpr uint32_t kLLLogMax = 9, kMLLogMax = 9, kOFLogMax = 8, kWeightLogMax = 6, kHufLogMax = 11;
constexpr uint32_t kLLSymMax = 35, kMLSymMax = 52, kOFSymMax = 31;
constexpr uint32_t kLLDefaultLog = 6, kMLDefaultLog = 6, kOFDefaultLog = 5;
constexpr uint32_t kLongSeqCount = 0x7F00;
enum BlockType { kRawBlock = 0, kRleBlock = 1, kCompressedBlock = 2, kReservedBlock = 3 };
enum LitType { kRawLit = 0, kRleLit = 1, kHufLit = 2, kTreelessLit = 3 };
enum SeqMode { kPredefined = 0, kRleMode = 1, kFseMode = 2, kRepeatMode = 3 };

constexpr uint32_t kLLBase[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,   10,  11,  12,  13,   14,   15,   16,   18,
                                  20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
constexpr uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr uint32_t kMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20,
                                  21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 37, 39, 41,
                                  43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
constexpr uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
// the three predefined distributions (RFC 8878 3.1.1.3.2.2)
constexpr int16_t kLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                    2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int16_t kMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
constexpr int16_t kOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

constexpr uint32_t highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); } // v >= 1

// ---- frame and block headers ----------------------------------------------------------------------------------
enum FrameKind { kNoFrame = 0, kDataFrame = 1, kSkippableFrame = 2 };
struct FrameHeader
{
  uint32_t kind;          // kNoFrame: refused (no magic, truncated, reserved bit, a dictionary, a window past 2^31)
  uint32_t header_bytes;  // data frame: up to the first block; skippable frame: the whole frame
  bool has_size, checksum;
  uint64_t content_size;
  uint64_t window;
  uint64_t skip_bytes;    // skippable frame: header and content
  uint32_t dict_id;       // data frame: its Dictionary_ID, 0 where it has none
};

// dictionaries false: a frame with a non-zero Dictionary_ID is refused here; true: the caller applies the
// Dictionary_ID rule (zstd_dict.hpp) to dict_id
template <class P>
constexpr FrameHeader parse_frame_header(P p, uint64_t n, bool dictionaries = false)
{
  FrameHeader h{kNoFrame, 0, false, false, 0, 0, 0, 0};
  if (n < 5)   // (what libzstd asks before it looks at a magic number)
    return h;
  const uint32_t magic = (uint32_t)read_le(p, 0, 4);
  if ((magic & 0xFFFFFFF0u) == kSkippableMagic) {
    if (n < 8)
      return h;
    const uint64_t total = 8u + read_le(p, 4, 4);
    if (total > n)
      return h;
    h.kind = kSkippableFrame;
    h.skip_bytes = total;
    return h;
  }
  if (magic != kMagic)
    return h;
  const uint32_t fhd = (uint8_t)p[4];
  const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
  if (fhd & 0x08u) // the reserved bit (the unused bit 4 is ignored)
    return h;
  const uint32_t did_bytes = did_flag == 3u ? 4u : did_flag;
  const uint32_t fcs_bytes = fcs_flag == 0u ? single : 1u << fcs_flag;
  const uint32_t hb = 5u + (single ? 0u : 1u) + did_bytes + fcs_bytes;
  if (n < hb)
    return h;
  uint32_t at = 5;
  if (!single) {
    const uint32_t wd = (uint8_t)p[at++];
    const uint32_t log = 10u + (wd >> 3);
    if (log > 31u)
      return h;
    h.window = (1ull << log) + ((1ull << log) >> 3) * (wd & 7u);
  }
  const uint64_t did = read_le(p, at, did_bytes);
  h.dict_id = (uint32_t)did;
  if (did != 0 && !dictionaries)
    return h;
  at += did_bytes;
  if (fcs_bytes) {
    h.content_size = read_le(p, at, fcs_bytes) + (fcs_bytes == 2u ? 256u : 0u);
    h.has_size = true;
  }
  if (single)
    h.window = h.content_size;
  h.checksum = (fhd & 0x04u) != 0;
  h.header_bytes = hb;
  h.kind = kDataFrame;
  return h;
}

struct BlockHeader
{
  bool ok, last;
  uint32_t type;
  uint32_t size;       // Block_Size: the decoded size of an RLE block, else the bytes that follow
  uint32_t comp_bytes; // the bytes that follow the header (1 for an RLE block)
};

// n: the bytes left in the chunk
template <class P>
constexpr BlockHeader parse_block_header(P p, uint64_t n)
{
  BlockHeader b{false, false, 0, 0, 0};
  if (n < 3)
    return b;
  const uint32_t v = (uint32_t)read_le(p, 0, 3);
  b.last = v & 1u;
  b.type = (v >> 1) & 3u;
  b.size = v >> 3;
  b.comp_bytes = b.type == kRleBlock ? 1u : b.size;
  b.ok = b.type != kReservedBlock && b.comp_bytes <= n - 3;
  return b;
}

// ---- literals and sequences section headers ---------------------------------------------------------------------
struct LitHeader
{
  bool ok;
  uint32_t type, header_bytes, regen, comp, streams; // comp: the bytes after the header (raw: regen, RLE: 1)
};

// n: the block's size
template <class P>
constexpr LitHeader parse_literals_header(P p, uint32_t n)
{
  LitHeader h{false, 0, 0, 0, 0, 1};
  if (n < 3) // (libzstd: no compressed block is shorter)
    return h;
  const uint32_t b0 = (uint8_t)p[0];
  h.type = b0 & 3u;
  const uint32_t sf = (b0 >> 2) & 3u;
  if (h.type >= kHufLit) {
    if (n < 5)
      return h;
    const uint32_t lhc = (uint32_t)read_le(p, 0, 4);
    if (sf <= 1u) {
      h.header_bytes = 3;
      h.regen = (lhc >> 4) & 0x3FFu;
      h.comp = (lhc >> 14) & 0x3FFu;
    } else if (sf == 2u) {
      h.header_bytes = 4;
      h.regen = (lhc >> 4) & 0x3FFFu;
      h.comp = lhc >> 18;
    } else {
      h.header_bytes = 5;
      h.regen = (lhc >> 4) & 0x3FFFFu;
      h.comp = (lhc >> 22) + ((uint32_t)(uint8_t)p[4] << 10);
    }
    h.streams = sf == 0u ? 1u : 4u;
    h.ok = h.regen <= kBlockMax && h.comp + h.header_bytes <= n;
    return h;
  }
  if ((sf & 1u) == 0u) {
    h.header_bytes = 1;
    h.regen = b0 >> 3;
  } else if (sf == 1u) {
    h.header_bytes = 2;
    h.regen = (uint32_t)read_le(p, 0, 2) >> 4;
  } else {
    h.header_bytes = 3;
    h.regen = (uint32_t)read_le(p, 0, 3) >> 4;
  }
  h.comp = h.type == kRawLit ? h.regen : 1u;
  h.ok = h.regen <= kBlockMax && h.header_bytes + h.comp <= n && !(h.type == kRleLit && sf == 3u && n < 4);
  return h;
}

struct SeqHeader
{
  bool ok;
  uint32_t nseq, header_bytes, ll_mode, of_mode, ml_mode;
};

// n: the bytes of the block behind its literals section
template <class P>
constexpr SeqHeader parse_sequences_header(P p, uint32_t n)
{
  SeqHeader h{false, 0, 0, 0, 0, 0};
  if (n < 1)
    return h;
  const uint32_t b0 = (uint8_t)p[0];
  if (b0 == 0) { // no sequences: the section is this one byte
    h.header_bytes = 1;
    h.ok = n == 1;
    return h;
  }
  if (b0 < 128u) {
    h.nseq = b0;
    h.header_bytes = 1;
  } else if (b0 < 255u) {
    if (n < 2)
      return h;
    h.nseq = ((b0 - 128u) << 8) + (uint8_t)p[1];
    h.header_bytes = 2;
  } else {
    if (n < 3)
      return h;
    h.nseq = (uint32_t)read_le(p, 1, 2) + kLongSeqCount;
    h.header_bytes = 3;
  }
  if (n < h.header_bytes + 1u)
    return h;
  const uint32_t modes = (uint8_t)p[h.header_bytes];
  h.header_bytes += 1;
  h.ll_mode = modes >> 6;
  h.of_mode = (modes >> 4) & 3u;
  h.ml_mode = (modes >> 2) & 3u; // (the two reserved bits are not looked at, as in libzstd 1.4.8)
  h.ok = true;
  return h;
}

// ---- FSE ---------------------------------------------------------------------------------------------------------
// `cnt` <= 16 bits at bit `pos` of the forward stream p[0, n); bits behind the end read as zero
template <class P>
constexpr uint32_t forward_bits(P p, uint32_t n, uint32_t pos, uint32_t cnt)
{
  const uint32_t at = pos >> 3;
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4; ++b)
    if (at + b < n)
      v |= (uint32_t)(uint8_t)p[at + b] << (8u * b);
  return (v >> (pos & 7u)) & ((1u << cnt) - 1u);
}

struct NCount
{
  bool ok;
  uint32_t log, nsym, bytes;
};

// The table description at p[0, n) -> norm[0, nsym) (-1: the "less than 1" probability) and its verdict: the
// accuracy log within max_log, no symbol past max_sym, the probabilities sum to exactly 2^log, zero-repeat flags
// that stay inside the alphabet, and no bit read behind the description's end.
template <class P, class N>
constexpr NCount read_ncount(P p, uint32_t n, N norm, uint32_t max_sym, uint32_t max_log)
{
  NCount r{false, 0, 0, 0};
  r.log = forward_bits(p, n, 0, 4) + 5u;
  if (r.log > max_log)
    return r;
  uint32_t pos = 4, sym = 0;
  int32_t remaining = (1 << r.log) + 1, threshold = 1 << r.log;
  uint32_t nb = r.log + 1u;
  bool prev0 = false;
  while (remaining > 1 && sym <= max_sym) {
    if (prev0) {
      uint32_t n0 = sym;
      for (;;) {
        const uint32_t rep = forward_bits(p, n, pos, 2);
        pos += 2;
        n0 += rep;
        if (rep != 3u || n0 > max_sym)
          break;
      }
      if (n0 > max_sym)
        return r;
      while (sym < n0)
        norm[sym++] = 0;
    }
    const int32_t max = (2 * threshold - 1) - remaining;
    const int32_t v = (int32_t)forward_bits(p, n, pos, nb);
    int32_t count = 0;
    if ((v & (threshold - 1)) < max) {
      count = v & (threshold - 1);
      pos += nb - 1u;
    } else {
      count = v & (2 * threshold - 1);
      if (count >= threshold)
        count -= max;
      pos += nb;
    }
    count -= 1;
    remaining -= count < 0 ? -count : count;
    norm[sym++] = (int16_t)count;
    prev0 = count == 0;
    while (remaining < threshold) {
      nb -= 1;
      threshold >>= 1;
    }
  }
  r.bytes = (pos + 7u) >> 3;
  r.nsym = sym;
  r.ok = remaining == 1 && r.bytes <= n;
  return r;
}

struct FseEntry
{
  uint16_t base;
  uint8_t sym, nbits;
};

// norm[0, nsym) with sum 2^log -> table[0, 2^log); next[0, nsym) is scratch
template <class N, class T, class S>
constexpr void fse_build(N norm, uint32_t nsym, uint32_t log, T table, S next)
{
  const uint32_t size = 1u << log, mask = size - 1u;
  uint32_t high = size - 1u;
  for (uint32_t s = 0; s < nsym; ++s) {
    if (norm[s] == -1) {
      table[high--].sym = (uint8_t)s;
      next[s] = 1;
    } else {
      next[s] = (uint16_t)norm[s];
    }
  }
  const uint32_t step = (size >> 1) + (size >> 3) + 3u;
  uint32_t pos = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    const int32_t c = norm[s];
    for (int32_t i = 0; i < c; ++i) {
      table[pos].sym = (uint8_t)s;
      do
        pos = (pos + step) & mask;
      while (pos > high);
    }
  }
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t s = table[u].sym;
    const uint32_t x = next[s];
    next[s] = (uint16_t)(x + 1u);
    const uint32_t nb = log - highbit(x);
    table[u].nbits = (uint8_t)nb;
    table[u].base = (uint16_t)((x << nb) - size);
  }
}

template <class T>
constexpr void fse_build_rle(T table, uint32_t sym)
{
  table[0].base = 0;
  table[0].sym = (uint8_t)sym;
  table[0].nbits = 0;
}

// ---- the backward bitstream ---------------------------------------------------------------------------------------
// The stream p[0, n) is read from its last byte down; `left` is the count of unread bits.  A read past the
// stream's start pads with zero bits and leaves `left` negative: the caller refuses the chunk.
template <class P>
struct BackBits
{
  P p;
  uint32_t n;
  int32_t left;
  uint64_t win;   // bits [win_lo, win_lo + 64) of the stream
  int32_t win_lo; // < 0: no window yet

  constexpr bool init(P p_, uint32_t n_) // false: an empty stream, or one without its final-bit marker
  {
    p = p_;
    n = n_;
    left = 0;
    win = 0;
    win_lo = -1;
    if (n == 0)
      return false;
    const uint32_t last = (uint8_t)p[n - 1];
    if (last == 0)
      return false;
    left = (int32_t)(8u * (n - 1u) + highbit(last));
    return true;
  }
  constexpr uint32_t peek(uint32_t cnt) // cnt <= 32
  {
    if (cnt == 0 || left <= 0)
      return 0;
    int32_t lo = left - (int32_t)cnt;
    uint32_t pad = 0;
    if (lo < 0) {
      pad = (uint32_t)-lo;
      lo = 0;
    }
    if (win_lo < 0 || lo < win_lo || left > win_lo + 64) {
      const uint32_t top = ((uint32_t)left + 7u) >> 3;
      const uint32_t start = top > 8u ? top - 8u : 0u;
      win = 0;
      for (uint32_t b = 0; b < 8; ++b)
        if (start + b < n)
          win |= (uint64_t)(uint8_t)p[start + b] << (8u * b);
      win_lo = (int32_t)(8u * start);
    }
    const uint32_t width = cnt - pad;
    return (uint32_t)((win >> (lo - win_lo)) & ((1ull << width) - 1ull)) << pad;
  }
  constexpr uint32_t read(uint32_t cnt)
  {
    const uint32_t v = peek(cnt);
    left -= (int32_t)cnt;
    return v;
  }
};

// ---- the Huffman tree description ---------------------------------------------------------------------------------
struct HufDesc
{
  bool ok;
  uint32_t bytes, nsym, log; // bytes: the description's size with its header byte
};

// p[0, n): the literals section behind its header.  -> weights[0, nsym), the last one implied.  norm (int16[256]),
// wtable (FseEntry[64]) and next (uint16[256]) are scratch for FSE-compressed weights.
template <class P, class W, class N, class T, class S>
constexpr HufDesc read_huf_weights(P p, uint32_t n, W weights, N norm, T wtable, S next)
{
  HufDesc d{false, 0, 0, 0};
  if (n < 1)
    return d;
  const uint32_t hb = (uint8_t)p[0];
  uint32_t cnt = 0;
  if (hb >= 128u) { // direct: 4 bits a weight
    cnt = hb - 127u;
    d.bytes = 1u + (cnt + 1u) / 2u;
    if (d.bytes > n)
      return d;
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint32_t b = (uint8_t)p[1u + i / 2u];
      weights[i] = (uint8_t)((i & 1u) ? b & 15u : b >> 4);
    }
  } else {          // FSE-compressed, two interleaved states
    d.bytes = 1u + hb;
    if (d.bytes > n)
      return d;
    const NCount nc = read_ncount(p + 1, hb, norm, 255u, kWeightLogMax);
    if (!nc.ok)
      return d;
    fse_build(norm, nc.nsym, nc.log, wtable, next);
    BackBits<P> bs{};
    if (!bs.init(p + 1 + nc.bytes, hb - nc.bytes))
      return d;
    uint32_t s1 = bs.read(nc.log), s2 = bs.read(nc.log);
    if (bs.left < 0)
      return d;
    for (;;) {
      if (cnt > 253u)
        return d;
      weights[cnt++] = wtable[s1].sym;
      s1 = wtable[s1].base + bs.read(wtable[s1].nbits);
      if (bs.left < 0) {
        weights[cnt++] = wtable[s2].sym;
        break;
      }
      if (cnt > 253u)
        return d;
      weights[cnt++] = wtable[s2].sym;
      s2 = wtable[s2].base + bs.read(wtable[s2].nbits);
      if (bs.left < 0) {
        weights[cnt++] = wtable[s1].sym;
        break;
      }
    }
  }
  uint32_t total = 0, ones = 0;
  for (uint32_t i = 0; i < cnt; ++i) {
    const uint32_t w = weights[i];
    if (w > kHufLogMax)
      return d;
    total += (1u << w) >> 1;
    ones += w == 1u;
  }
  if (total == 0)
    return d;
  d.log = highbit(total) + 1u;
  if (d.log > kHufLogMax)
    return d;
  const uint32_t rest = (1u << d.log) - total;
  if (rest & (rest - 1u)) // the implied weight completes a power of two
    return d;
  const uint32_t last = highbit(rest) + 1u;
  weights[cnt] = (uint8_t)last;
  ones += last == 1u;
  if (ones < 2u || (ones & 1u))
    return d;
  d.nsym = cnt + 1u;
  d.ok = true;
  return d;
}

// count[w] (w in [0, 12]): symbols of weight w; sorted[]: the symbols of weight >= 1 by weight, then by symbol
template <class W, class C, class S>
constexpr void huf_sort(W weights, uint32_t nsym, C count, S sorted)
{
  for (uint32_t w = 0; w <= kHufLogMax + 1u; ++w)
    count[w] = 0;
  for (uint32_t s = 0; s < nsym; ++s)
    count[weights[s]] += 1;
  uint32_t at[kHufLogMax + 2u] = {};
  uint32_t first = 0;
  for (uint32_t w = 1; w <= kHufLogMax; ++w) {
    at[w] = first;
    first += count[w];
  }
  for (uint32_t s = 0; s < nsym; ++s) {
    const uint32_t w = weights[s];
    if (w)
      sorted[at[w]++] = (uint8_t)s;
  }
}

// entry e of the decoding table of 2^log entries, indexed by the next `log` bits: (symbol << 8) | bits
template <class C, class S>
constexpr uint32_t huf_entry(uint32_t e, C count, S sorted, uint32_t log)
{
  uint32_t start = 0, first = 0;
  for (uint32_t w = 1; w <= log; ++w) {
    const uint32_t span = (uint32_t)count[w] << (w - 1u);
    if (e < start + span)
      return ((uint32_t)(uint8_t)sorted[first + ((e - start) >> (w - 1u))] << 8) | (log + 1u - w);
    start += span;
    first += count[w];
  }
  return 0;
}

// the sizes of the four streams behind a jump table, p[0, n) being the streams with it: false where they do not fit
template <class P>
constexpr bool huf_jump_table(P p, uint32_t n, uint32_t size[4])
{
  if (n < 10)
    return false;
  size[0] = (uint32_t)read_le(p, 0, 2);
  size[1] = (uint32_t)read_le(p, 2, 2);
  size[2] = (uint32_t)read_le(p, 4, 2);
  const uint32_t three = size[0] + size[1] + size[2];
  if (6u + three > n)
    return false;
  size[3] = n - 6u - three;
  return true;
}

// ---- sequences -----------------------------------------------------------------------------------------------------
struct SeqState
{
  uint32_t ll, of, ml;
  uint32_t rep[3];
};
struct Sequence
{
  uint32_t ll, ml, off;
};

// One sequence: the offset's, the match length's and the literal length's extra bits, then (not behind the last
// sequence) the three state updates; the repeat offsets are resolved and updated (3.1.1.5).
template <class B, class T>
constexpr Sequence decode_sequence(B& bs, SeqState& st, T llt, T oft, T mlt, bool last)
{
  const uint32_t llc = llt[st.ll].sym, ofc = oft[st.of].sym, mlc = mlt[st.ml].sym;
  Sequence q{0, 0, 0};
  if (ofc > 1u) {
    q.off = ((1u << ofc) - 3u) + bs.read(ofc);
    st.rep[2] = st.rep[1];
    st.rep[1] = st.rep[0];
    st.rep[0] = q.off;
  } else {
    const uint32_t ll0 = llc == 0u; // a literal length of zero shifts the meaning of the repeat codes
    if (ofc == 0u) {
      if (!ll0) {
        q.off = st.rep[0];
      } else {
        q.off = st.rep[1];
        st.rep[1] = st.rep[0];
        st.rep[0] = q.off;
      }
    } else {
      const uint32_t idx = 1u + ll0 + bs.read(1);
      uint32_t v = idx == 3u ? st.rep[0] - 1u : st.rep[idx];
      v += v == 0u; // (libzstd: an offset of zero becomes one)
      if (idx != 1u)
        st.rep[2] = st.rep[1];
      st.rep[1] = st.rep[0];
      st.rep[0] = q.off = v;
    }
  }
  q.ml = kMLBase[mlc] + bs.read(kMLBits[mlc]);
  q.ll = kLLBase[llc] + bs.read(kLLBits[llc]);
  if (!last) {
    st.ll = llt[st.ll].base + bs.read(llt[st.ll].nbits);
    st.ml = mlt[st.ml].base + bs.read(mlt[st.ml].nbits);
    st.of = oft[st.of].base + bs.read(oft[st.of].nbits);
  }
  return q;
}

// ---- launch sizing (zstd_launch.hpp uses it, the CPU tests restate it) -----------------------------------------------
constexpr uint64_t literal_bytes_per_wave(uint64_t max_uncompressed_chunk_bytes)
{
  const uint64_t b = max_uncompressed_chunk_bytes < kBlockMax ? max_uncompressed_chunk_bytes : kBlockMax;
  return (b + 255u) / 256u * 256u;
}

} // namespace zstd
} // namespace hcamd
