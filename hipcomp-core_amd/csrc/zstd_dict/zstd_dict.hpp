// zstd_dict.hpp -- the dictionary logic of the Zstandard decoder (RFC 8878 section 5), free of HIP.
//
// Constexpr and plain C++17 like ../zstd/zstd_tables.hpp, on which it builds: the kernels
// (zstd_dict_kernels.hip, ../zstd/zstd_decode.hiph) and the CPU driver (tests/zstd_dict_driver.cpp) include
// this one file.  It holds the verdict on a dictionary with the offsets of its sections, the layout of the
// prepared blob, the Dictionary_ID rule, the bound of an offset and the one function through which a match
// reads history that may lie in the dictionary.  The arbiter is ZSTD_decompress_usingDict of libzstd 1.4.8;
// where this decoder differs on purpose, include/hipcomp/zstd_dict.h lists it.
#pragma once

#include <cstdint>

#include "zstd/zstd_tables.hpp"

namespace hcamd {
namespace zstd {

constexpr uint32_t kDictMagic = 0xEC30A437u;
constexpr uint64_t kDictBytesMax = 1ull << 30;

// ---- the dictionary ------------------------------------------------------------------------------------------------
struct DictLayout
{
  bool ok;             // false: refused
  bool formatted;      // false: raw content, [0, n) is the content
  uint32_t dict_id;
  uint32_t huf_at, of_at, ml_at, ll_at, rep_at; // the sections of a formatted dictionary
  uint32_t content_at, content_size;
  uint32_t rep[3];
};

// The verdict on the dictionary p[0, n), n <= kDictBytesMax, and where its sections lie.  weights (uint8[256]),
// norm (int16[256]), wtable (FseEntry[64]) and next (uint16[256]) are scratch, as for read_huf_weights.
// A buffer shorter than 8 bytes or without the magic number is raw content.  A formatted dictionary is refused
// where it is exactly 8 bytes, where a description is refused, where fewer than 12 bytes are left for the repeat
// offsets and where a repeat offset is 0 or above the content size (so a formatted dictionary has content).
template <class P, class W, class N, class T, class S>
constexpr DictLayout parse_dictionary(P p, uint32_t n, W weights, N norm, T wtable, S next)
{
  DictLayout d{true, false, 0, 0, 0, 0, 0, 0, 0, n, {1, 4, 8}};
  if (n < 8 || (uint32_t)read_le(p, 0, 4) != kDictMagic)
    return d;
  d.ok = false;
  d.formatted = true;
  d.dict_id = (uint32_t)read_le(p, 4, 4);
  if (n <= 8)
    return d;
  uint32_t at = 8;
  d.huf_at = at;
  const HufDesc h = read_huf_weights(p + at, n - at, weights, norm, wtable, next);
  if (!h.ok)
    return d;
  at += h.bytes;
  d.of_at = at;
  const NCount of = read_ncount(p + at, n - at, norm, kOFSymMax, kOFLogMax);
  if (!of.ok)
    return d;
  at += of.bytes;
  d.ml_at = at;
  const NCount ml = read_ncount(p + at, n - at, norm, kMLSymMax, kMLLogMax);
  if (!ml.ok)
    return d;
  at += ml.bytes;
  d.ll_at = at;
  const NCount ll = read_ncount(p + at, n - at, norm, kLLSymMax, kLLLogMax);
  if (!ll.ok)
    return d;
  at += ll.bytes;
  d.rep_at = at;
  if (n - at < 12)
    return d;
  d.content_at = at + 12u;
  d.content_size = n - d.content_at;
  for (uint32_t i = 0; i < 3; ++i) {
    d.rep[i] = (uint32_t)read_le(p, at + 4u * i, 4);
    if (d.rep[i] == 0 || d.rep[i] > d.content_size)
      return d;
  }
  d.ok = true;
  return d;
}

// ---- the prepared blob ----------------------------------------------------------------------------------------------
// header | ll[512] ml[512] of[256] of FseEntry | huf[2048] of uint16 | content.  No pointers: a copy stays valid.
constexpr uint32_t kPreparedMagic = 0x44435A48u; // "HZCD"
constexpr uint32_t kPreparedVersion = 1;
struct PreparedHeader
{
  uint32_t magic, version, valid, dict_id, has_entropy;
  uint32_t ll_log, ml_log, of_log, huf_log;
  uint32_t rep[3];
  uint32_t content_offset, content_size, total_size, reserved;
};
static_assert(sizeof(PreparedHeader) == 64, "the blob's header is 64 bytes");
static_assert(sizeof(FseEntry) == 4, "tables are stored as they lie in LDS");
constexpr uint32_t kPreparedAlign = 16;
constexpr uint32_t kPreparedLL = sizeof(PreparedHeader);
constexpr uint32_t kPreparedML = kPreparedLL + 4u * (1u << kLLLogMax);
constexpr uint32_t kPreparedOF = kPreparedML + 4u * (1u << kMLLogMax);
constexpr uint32_t kPreparedHuf = kPreparedOF + 4u * (1u << kOFLogMax);
constexpr uint32_t kPreparedContent = kPreparedHuf + 2u * (1u << kHufLogMax);
static_assert(kPreparedContent % kPreparedAlign == 0, "sections start at 16-byte boundaries");

// the size of the blob of a dictionary of dict_bytes bytes (a function of dict_bytes alone: whatever the
// dictionary's sections take, its content is no longer than the dictionary)
constexpr uint64_t prepared_bytes(uint64_t dict_bytes)
{
  return kPreparedContent + (dict_bytes + (kPreparedAlign - 1u)) / kPreparedAlign * kPreparedAlign;
}

// ---- a frame against a dictionary -----------------------------------------------------------------------------------
// A non-zero Dictionary_ID must be the ID of the dictionary given; raw content and "no dictionary" have ID 0.
constexpr bool dict_id_accepted(uint32_t frame_dict_id, uint32_t given_dict_id)
{
  return frame_dict_id == 0 || frame_dict_id == given_dict_id;
}

// An offset reaches at most over what the frame has produced and the dictionary's content before it.
constexpr bool offset_in_history(uint64_t offset, uint64_t produced_in_frame, uint64_t content_size)
{
  return offset <= produced_in_frame + content_size;
}

// Byte v of content ++ (the frame's output): the one way a match's source is read where it may begin in the
// dictionary.  A match at position pos of the frame with offset off starts at v = content_size + pos - off and
// its byte i is history_at(v + i % off) where it overruns itself, history_at(v + i) otherwise.
template <class C, class O>
constexpr uint8_t history_at(C content, uint64_t content_size, O frame_out, uint64_t v)
{
  return v < content_size ? (uint8_t)content[v] : (uint8_t)frame_out[v - content_size];
}

} // namespace zstd
} // namespace hcamd
