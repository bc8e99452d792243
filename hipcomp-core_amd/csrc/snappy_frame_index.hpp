// snappy_frame_index.hpp -- the chunk index of a seekable Snappy framed stream: one reserved skippable chunk of type
// 0xa5 that stands immediately behind a stream identifier and holds the first four bytes of every data chunk of that
// stream, so that a reader finds every chunk by a scan instead of following the chain.  The writer, the parser with
// a reason for every refusal, and the size and offset arithmetic (the framing format itself:
// snappy_frame.hpp).  All fields little-endian:
//
//    0  u8   0xa5
//    1  u24  36 + 4N                    the chunk's length field (bytes that follow)
//    4  8 B  "HCSNPIDX"
//   12  u32  version = 1
//   16  u32  flags = 0                  every bit reserved
//   20  u32  chunk_bytes                content bytes of every data chunk but the last, 1 .. 65536
//   24  u32  N                          data chunks
//   28  u64  content_bytes              N == ceil(content_bytes / chunk_bytes)
//   36  N x u32                         the first four bytes of data chunk i as they stand in the stream (type in
//                                       bits 0-7, length field in bits 8-31: szf::written_header)
//   36 + 4N  u32  mask(CRC-32C(bytes [4, 36 + 4N)))
//
// A unit: identifier, index, exactly N data chunks back to back; behind them the end of the input, padding and
// reserved skippable chunks (an index that does not stand behind an identifier is one of them), or the identifier
// of the next unit.  An input is indexed when it is such units and nothing else.
//
// The index is untrusted: it applies only if it is sound in itself and every word is found, byte for byte, where the
// scan of the words says it stands, with a type, a length and (compressed chunks) a preamble that fit the chunk's
// share of the content.  By induction that is the chain a reader without the index follows.
//
// Standard headers and constexpr only: the kernels (snappy_frame_index_kernels.hip), the manager (hlif.hip) and the
// CPU driver of tests/test_snappy_frame_index_cpu.py include this one text.
#pragma once

#include <cstddef>
#include <cstdint>

#include "crc32c_math.hpp"
#include "snappy_frame.hpp"

namespace hcamd {
namespace szf {

constexpr uint32_t kTypeIndex = 0xa5;
constexpr uint32_t kIndexFormatVersion = 1;
constexpr uint32_t kIndexFixedLength = 36; // signature .. content_bytes, and the CRC
constexpr uint32_t kIndexWordsAt = 36;     // of word 0 from the chunk's first byte
constexpr uint32_t kIndexMaxChunks = (0xFFFFFFu - kIndexFixedLength) / 4; // 4 194 294: the length field has 24 bits
constexpr uint8_t kIndexSignatureBytes[8] = {'H', 'C', 'S', 'N', 'P', 'I', 'D', 'X'};

constexpr uint64_t index_bytes(uint64_t chunks) { return 40 + 4 * chunks; }
// the most compress_frame(..., Leading) takes: the stream's bound (snappy_frame.hpp) and the index
constexpr uint64_t indexed_frame_bound(uint64_t num_chunks, uint64_t chunk_bytes)
{
  return frame_bound(num_chunks, chunk_bytes) + index_bytes(num_chunks);
}

// why an index does not apply; the numbers are the test drivers' and the tests' too
enum IndexReason : uint32_t {
  kIndexOk = 0,
  kIndexNotThere = 1,      // no identifier where a unit begins, or no chunk of type 0xa5 immediately behind it
  kIndexLength = 2,        // the length field is below 36, runs past the end of the input, or is not 36 + 4N
  kIndexSignature = 3,
  kIndexVersion = 4,
  kIndexFlags = 5,         // a reserved bit
  kIndexChunkBytes = 6,    // 0 or above 65536
  kIndexCount = 7,         // N is not ceil(content_bytes / chunk_bytes)
  kIndexCrc = 8,
  kIndexType = 9,          // a word whose type is neither 0x00 nor 0x01
  kIndexOffset = 10,       // a chunk at its scanned offset does not lie inside the input
  kIndexWord = 11,         // the four bytes found there are not the index's
  kIndexStoredLength = 12, // a stored chunk that does not hold its CRC and its share of the content
  kIndexNoPayload = 13,    // a compressed chunk without a byte behind its CRC
  kIndexPreamble = 14,     // a preamble that is no complete varint, or is not the chunk's share
  kIndexBehind = 15,       // behind the last data chunk: a data chunk, a reserved unskippable one, a cut one
  kIndexDecode = 16,       // (device) a compressed chunk did not decode to exactly its share
  kIndexTooManyUnits = 17, // (device) more units than the reader's table holds, or 2^32 data chunks
  kIndexReasons = 18
};

struct IndexHead
{
  uint32_t chunk_bytes = 0, chunks = 0;
  uint64_t content_bytes = 0;
};

constexpr uint32_t index_read32(const uint8_t* p)
{
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
constexpr uint64_t chunks_of(uint64_t content_bytes, uint32_t chunk_bytes)
{
  return content_bytes / chunk_bytes + (content_bytes % chunk_bytes ? 1 : 0);
}
// content bytes of data chunk i of N
constexpr uint32_t chunk_share(const IndexHead& h, uint64_t i)
{
  return i + 1 < h.chunks ? h.chunk_bytes : (uint32_t)(h.content_bytes - (uint64_t)h.chunk_bytes * i);
}
// bytes of the data chunk a word stands for, its header included
constexpr uint64_t indexed_chunk_bytes(uint32_t word) { return 4 + (uint64_t)(word >> 8); }

// p: the byte behind an identifier, avail: bytes from there to the end of the input.  Everything but the CRC
// (index_crc_fits): the kernels compute it with a workgroup.
constexpr uint32_t parse_index_fields(const uint8_t* p, uint64_t avail, IndexHead& h)
{
  if (avail < 4 || p[0] != kTypeIndex)
    return kIndexNotThere;
  const uint32_t length = index_read32(p) >> 8;
  if (length < kIndexFixedLength || length > avail - 4)
    return kIndexLength;
  for (int k = 0; k < 8; ++k)
    if (p[4 + k] != kIndexSignatureBytes[k])
      return kIndexSignature;
  if (index_read32(p + 12) != kIndexFormatVersion)
    return kIndexVersion;
  if (index_read32(p + 16) != 0)
    return kIndexFlags;
  h.chunk_bytes = index_read32(p + 20);
  if (h.chunk_bytes == 0 || h.chunk_bytes > kMaxContent)
    return kIndexChunkBytes;
  h.chunks = index_read32(p + 24);
  h.content_bytes = (uint64_t)index_read32(p + 28) | (uint64_t)index_read32(p + 32) << 32;
  if ((uint64_t)length != kIndexFixedLength + 4 * (uint64_t)h.chunks)
    return kIndexLength;
  if (chunks_of(h.content_bytes, h.chunk_bytes) != h.chunks)
    return kIndexCount;
  return kIndexOk;
}

// (after parse_index_fields) the masked CRC behind the words against the one of the bytes in front of it
constexpr bool index_crc_fits(const crc32c::Tables& t, const uint8_t* p, const IndexHead& h)
{
  const uint64_t body = 32 + 4 * (uint64_t)h.chunks;
  return mask_crc(crc32c::crc32c_of(t, p + 4, (size_t)body)) == index_read32(p + 4 + body);
}

// word: index word i; found: the four bytes at chunk i's scanned offset; w: the 16 bytes there (header, CRC and
// preamble; the chunk lies inside the input); share: chunk i's content bytes
constexpr uint32_t check_indexed_chunk(uint32_t word, uint32_t found, const Window& w, uint32_t share)
{
  const uint32_t type = word & 0xFFu, length = word >> 8;
  if (type != kTypeCompressed && type != kTypeStored)
    return kIndexType;
  if (found != word)
    return kIndexWord;
  if (type == kTypeStored)
    return length == 4 + share ? (uint32_t)kIndexOk : (uint32_t)kIndexStoredLength;
  if (length <= 4)
    return kIndexNoPayload;
  uint64_t value = 0;
  uint32_t used = 0;
  if (!read_varint(w, 8, length - 4, value, used) || value != share)
    return kIndexPreamble;
  return kIndexOk;
}

// What stands behind a unit's last data chunk, from pos: padding and reserved skippable chunks are stepped over.
// kIndexOk with more == false: the end of the input; with more == true: pos stands at a sound identifier.
constexpr uint32_t step_behind_unit(const uint8_t* in, uint64_t n, uint64_t& pos, bool& more)
{
  more = false;
  while (pos < n) {
    Chunk c;
    const Window w = window_of(in + pos, n - pos);
    if (parse_chunk(w, n - pos, false, c) != kOk || c.kind != kSkipped)
      return kIndexBehind;
    if (w.byte(0) == kTypeIdentifier) {
      more = true;
      return kIndexOk;
    }
    pos += c.bytes;
  }
  return kIndexOk;
}

// ---- the writer ------------------------------------------------------------------------------------------------
// bytes [0, 36): everything in front of the words
constexpr void write_index_fields(uint8_t* p, uint32_t chunks, uint32_t chunk_bytes, uint64_t content_bytes)
{
  const uint32_t words[9] = {kTypeIndex | (kIndexFixedLength + 4 * chunks) << 8, 0, 0, kIndexFormatVersion, 0, chunk_bytes,
                             chunks, (uint32_t)content_bytes, (uint32_t)(content_bytes >> 32)};
  for (int w = 0; w < 9; ++w)
    for (int k = 0; k < 4; ++k)
      p[4 * w + k] = w == 1 || w == 2 ? kIndexSignatureBytes[4 * (w - 1) + k] : (uint8_t)(words[w] >> (8 * k));
}

// the whole index of `chunks` words into p[0, index_bytes(chunks))
constexpr void write_index(const crc32c::Tables& t, uint8_t* p, const uint32_t* words, uint32_t chunks, uint32_t chunk_bytes,
                           uint64_t content_bytes)
{
  write_index_fields(p, chunks, chunk_bytes, content_bytes);
  for (uint32_t i = 0; i < chunks; ++i)
    for (int k = 0; k < 4; ++k)
      p[kIndexWordsAt + 4 * (uint64_t)i + k] = (uint8_t)(words[i] >> (8 * k));
  const uint64_t body = 32 + 4 * (uint64_t)chunks;
  const uint32_t crc = mask_crc(crc32c::crc32c_of(t, p + 4, (size_t)body));
  for (int k = 0; k < 4; ++k)
    p[4 + body + k] = (uint8_t)(crc >> (8 * k));
}

// ---- the whole test, one chunk after the other (the kernels do the chunks in parallel over a scan) ---------------
struct IndexedUnit
{
  IndexHead head;
  uint64_t words_at = 0; // of index word 0 in the input
  uint64_t data_at = 0;  // of data chunk 0: the byte behind the index
  uint64_t end = 0;      // the byte behind the last data chunk
};

// in[0, n): the input, at: where the unit's identifier may stand.  What follows the unit is input_is_indexed's.
constexpr uint32_t index_applies(const crc32c::Tables& t, const uint8_t* in, uint64_t n, uint64_t at, IndexedUnit& u)
{
  Chunk c;
  if (n - at < kIdentifierBytes || in[at] != kTypeIdentifier || parse_chunk(window_of(in + at, n - at), n - at, false, c) != kOk)
    return kIndexNotThere;
  const uint64_t index_at = at + kIdentifierBytes;
  const uint32_t r = parse_index_fields(in + index_at, n - index_at, u.head);
  if (r != kIndexOk)
    return r;
  if (!index_crc_fits(t, in + index_at, u.head))
    return kIndexCrc;
  u.words_at = index_at + kIndexWordsAt;
  u.data_at = index_at + index_bytes(u.head.chunks);
  uint64_t pos = u.data_at;
  for (uint64_t i = 0; i < u.head.chunks; ++i) {
    const uint32_t word = index_read32(in + u.words_at + 4 * i);
    const uint32_t type = word & 0xFFu;
    if (type != kTypeCompressed && type != kTypeStored)
      return kIndexType;
    if (pos > n || n - pos < indexed_chunk_bytes(word))
      return kIndexOffset;
    const uint32_t found = index_read32(in + pos);
    const uint32_t s = check_indexed_chunk(word, found, window_of(in + pos, n - pos), chunk_share(u.head, i));
    if (s != kIndexOk)
      return s;
    pos += indexed_chunk_bytes(word);
  }
  u.end = pos;
  return kIndexOk;
}

// The whole input: kIndexOk where it is indexed units and nothing else -- the inputs the indexed read takes; units /
// chunks / content_bytes: their sums.  Anything else gives the first reason met (no unit at all: kIndexNotThere),
// and the reader goes the chain's way.
constexpr uint32_t input_is_indexed(const crc32c::Tables& t, const uint8_t* in, uint64_t n, uint64_t& units, uint64_t& chunks,
                                    uint64_t& content_bytes)
{
  uint64_t pos = 0;
  units = chunks = content_bytes = 0;
  bool more = true;
  while (more) {
    IndexedUnit u;
    uint32_t r = index_applies(t, in, n, pos, u);
    if (r != kIndexOk)
      return r;
    units += 1;
    chunks += u.head.chunks;
    content_bytes += u.head.content_bytes;
    pos = u.end;
    r = step_behind_unit(in, n, pos, more);
    if (r != kIndexOk)
      return r;
  }
  return kIndexOk;
}

} // namespace szf
} // namespace hcamd
