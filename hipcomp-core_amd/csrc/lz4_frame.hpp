// lz4_frame.hpp -- the LZ4 frame format (LZ4 Frame Format Description v1.6.x, the public specification of liblz4's
// lz4frame) as the LZ4 manager reads and writes it: the descriptor parse with a reason for every refusal, the
// descriptor writer, the size-word and block-maximum arithmetic and the bound of a written frame.
//
//   magic 0x184D2204 | FLG | BD | [content size, 8] | [dictionary id, 4] | HC |
//   { size word (bit 31: stored) | data | [block checksum, 4] }* | EndMark 0 | [content checksum, 4]
//   FLG: version(7:6) = 01 | B.Indep(5) | B.Checksum(4) | C.Size(3) | C.Checksum(2) | reserved(1) | DictID(0)
//   BD:  reserved(7) | block maximum code(6:4) = 4..7 | reserved(3:0)
//   HC = (XXH32(FLG .. last descriptor byte, 0) >> 8) & 0xff
//
// Standard headers and constexpr only: the kernels (lz4_frame_kernels.hip), the manager (hlif.hip) and the CPU
// driver of tests/test_lz4_frame_cpu.py include this one text.
#pragma once

#include <cstddef>
#include <cstdint>

#include "xxh32_math.hpp"

namespace hcamd {
namespace lz4f {

constexpr uint32_t kMagic = 0x184D2204u;
constexpr uint32_t kLegacyFrameMagic = 0x184C2102u;
constexpr uint32_t kSkippableLow = 0x184D2A50u, kSkippableHigh = 0x184D2A5Fu;
constexpr uint32_t kStoredBit = 0x80000000u;
constexpr uint64_t kNoContentSize = ~uint64_t(0);
constexpr uint32_t kWrittenHeaderBytes = 15; // magic, FLG, BD, content size, HC

// why an input is refused; the numbers are the test drivers' and the tests' too
enum Reason : uint32_t {
  kOk = 0,
  kTruncated = 1,        // a header, block or trailer runs past the end of the input
  kUnknownMagic = 2,
  kLegacyMagic = 3,      // hipcompErrorNotSupported
  kBadVersion = 4,
  kReservedBit = 5,
  kBlockMaxCode = 6,     // below 4
  kHeaderChecksum = 7,
  kDictId = 8,           // hipcompErrorNotSupported
  kBlockTooLarge = 9,    // a size word above the block maximum
  kMissingEndMark = 10,  // the input ends where a size word or the EndMark should stand
  kDecodedTooLarge = 11, // a block decodes to more than the block maximum
  kBadBlock = 12,        // the block's stream is not decodable (a match before the frame's first byte included)
  kContentSize = 13,     // the decode contradicts the declared content size
  kTooManyBlocks = 14,   // more than 2^32 - 1 data blocks
  kReasons = 15
};

// 12 = hipcompErrorCannotDecompress, 11 = hipcompErrorNotSupported (hipcomp/shared_types.h)
constexpr int status_of(uint32_t reason)
{
  return reason == kOk ? 0 : (reason == kLegacyMagic || reason == kDictId) ? 11 : 12;
}

constexpr bool is_skippable(uint32_t magic) { return magic >= kSkippableLow && magic <= kSkippableHigh; }

constexpr uint32_t block_max_of_code(uint32_t code) { return code < 4 || code > 7 ? 0u : 1u << (8 + 2 * code); }
// the smallest code whose block maximum holds a chunk; 0: none does (more than 4 MiB)
constexpr uint32_t code_for_chunk(uint64_t chunk_bytes)
{
  for (uint32_t code = 4; code <= 7; ++code)
    if (block_max_of_code(code) >= chunk_bytes)
      return code;
  return 0;
}

// a written block: the chunk itself where its LZ4 stream is not smaller (LZ4F does the same)
constexpr bool stored(uint64_t stream_bytes, uint64_t chunk_bytes) { return stream_bytes >= chunk_bytes; }
constexpr uint32_t size_word(uint64_t stream_bytes, uint64_t chunk_bytes)
{
  return stored(stream_bytes, chunk_bytes) ? (uint32_t)chunk_bytes | kStoredBit : (uint32_t)stream_bytes;
}
// bytes of a written block with its size word and checksum
constexpr uint64_t block_bytes(uint64_t stream_bytes, uint64_t chunk_bytes, bool block_checksums)
{
  return 4 + (stored(stream_bytes, chunk_bytes) ? chunk_bytes : stream_bytes) + (block_checksums ? 4 : 0);
}

// The most a written frame takes: every chunk stored, the last one counted as a whole chunk too (the bound is a
// function of the chunk count alone).
constexpr uint64_t frame_bound(uint64_t num_chunks, uint64_t chunk_bytes, bool block_checksums)
{
  return kWrittenHeaderBytes + num_chunks * (chunk_bytes + 4 + (block_checksums ? 4 : 0)) + 4;
}

struct Descriptor
{
  uint32_t header_bytes = 0; // from the magic to the byte behind HC
  uint32_t block_max = 0;
  bool linked = false, block_checksums = false, content_checksum = false, has_content_size = false;
  uint64_t content_size = 0;
};

// p: where a frame's magic stands (not a skippable frame's), avail: bytes from there to the end of the input.
// The order of the tests is LZ4F_decodeHeader's; the dictionary flag is looked at last, in a header that is
// sound otherwise.
constexpr uint32_t parse_descriptor(const uint8_t* p, uint64_t avail, Descriptor& d)
{
  if (avail < 4)
    return kTruncated;
  const uint32_t magic = xxh32::read32(p);
  if (magic == kLegacyFrameMagic)
    return kLegacyMagic;
  if (magic != kMagic)
    return kUnknownMagic;
  if (avail < 5)
    return kTruncated;
  const uint32_t flg = p[4];
  if (flg & 2u)
    return kReservedBit;
  if ((flg >> 6) != 1u)
    return kBadVersion;
  d.linked = !(flg & 0x20u);
  d.block_checksums = flg & 0x10u;
  d.has_content_size = flg & 0x08u;
  d.content_checksum = flg & 0x04u;
  d.header_bytes = 7 + (d.has_content_size ? 8 : 0) + ((flg & 1u) ? 4 : 0);
  if (avail < d.header_bytes)
    return kTruncated;
  const uint32_t bd = p[5];
  if (bd & 0x80u)
    return kReservedBit;
  if (((bd >> 4) & 7u) < 4u)
    return kBlockMaxCode;
  if (bd & 0x0Fu)
    return kReservedBit;
  d.block_max = block_max_of_code((bd >> 4) & 7u);
  if (p[d.header_bytes - 1] != (uint8_t)(xxh32::hash(p + 4, d.header_bytes - 5, 0) >> 8))
    return kHeaderChecksum;
  if (flg & 1u)
    return kDictId;
  d.content_size = 0;
  if (d.has_content_size)
    for (int k = 0; k < 8; ++k)
      d.content_size |= (uint64_t)p[6 + k] << (8 * k);
  return kOk;
}

// the 15 bytes compress_frame writes: version 01, independent blocks, content size, no dictionary id
constexpr void write_descriptor(uint8_t* p, uint32_t block_max_code, uint64_t content_size, bool block_checksums)
{
  for (int k = 0; k < 4; ++k)
    p[k] = (uint8_t)(kMagic >> (8 * k));
  p[4] = (uint8_t)(0x40u | 0x20u | (block_checksums ? 0x10u : 0u) | 0x08u);
  p[5] = (uint8_t)(block_max_code << 4);
  for (int k = 0; k < 8; ++k)
    p[6 + k] = (uint8_t)(content_size >> (8 * k));
  p[14] = (uint8_t)(xxh32::hash(p + 4, 10, 0) >> 8);
}

} // namespace lz4f
} // namespace hcamd
