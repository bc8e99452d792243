// snappy_frame.hpp -- the Snappy framing format (.sz files; framing_format.txt of the Snappy distribution) as the
// Snappy manager reads and writes it: the chunk parse with a reason for every refusal, the length preamble's varint,
// the CRC mask and the bound of a written stream.
//
//   stream: { chunk }*      chunk: type (1) | length of what follows (3, little-endian) | body
//   0xff  stream identifier   length 6, body "sNaPpY"; the first chunk of an input, legal again anywhere
//   0x00  compressed data     masked CRC-32C of the UNCOMPRESSED bytes (4, little-endian) | one raw Snappy block
//   0x01  uncompressed data   the same 4 bytes | the bytes
//   0xfe  padding, 0x80-0xfd  reserved skippable: stepped over whatever they hold
//   0x02-0x7f                 reserved unskippable: refused
//   A data chunk holds at most 65536 bytes of content.  mask(c) = rotate_right(c, 15) + 0xa282ead8.
//
// Standard headers and constexpr only: the kernels (snappy_frame_kernels.hip), the manager (hlif.hip) and the CPU
// driver of tests/test_snappy_frame_cpu.py include this one text.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace szf {

constexpr uint32_t kMaxContent = 65536;
constexpr uint32_t kIdentifierBytes = 10;
constexpr uint32_t kTypeCompressed = 0x00, kTypeStored = 0x01, kTypeIdentifier = 0xff;
constexpr uint32_t kDataHeaderBytes = 8; // type, length, CRC

// why an input is refused; the numbers are the test drivers' and the tests' too
enum Reason : uint32_t {
  kOk = 0,
  kTruncated = 1,           // a header or body runs past the end of the input
  kNoIdentifier = 2,        // the first chunk is not the stream identifier
  kBadIdentifier = 3,       // an identifier of another length or body
  kReservedUnskippable = 4, // types 0x02 - 0x7f
  kShortChunk = 5,          // a data chunk of length < 4: no room for the CRC
  kNoPayload = 6,           // a compressed chunk that ends behind its CRC
  kBadPreamble = 7,         // the length preamble is no complete varint of at most 5 bytes
  kPreambleTooLarge = 8,    // it declares more than 65536 bytes
  kStoredTooLarge = 9,      // an uncompressed chunk of more than 65536 data bytes
  kBadBlock = 10,           // the block is not decodable (a match before the chunk's own first byte included)
  kSizeMismatch = 11,       // the block decodes to another size than its preamble's
  kBadChecksum = 12,        // hipcompErrorBadChecksum, where checksums are verified
  kReasons = 13
};

// 12 = hipcompErrorCannotDecompress, 13 = hipcompErrorBadChecksum (hipcomp/shared_types.h)
constexpr int status_of(uint32_t reason) { return reason == kOk ? 0 : reason == kBadChecksum ? 13 : 12; }

constexpr uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }
constexpr uint32_t unmask_crc(uint32_t m) { return ((m - 0xa282ead8u) >> 17) | ((m - 0xa282ead8u) << 15); }

// a written chunk: the block where it is strictly shorter than the chunk, else the chunk itself
constexpr bool stored(uint64_t block_bytes, uint64_t chunk_bytes) { return block_bytes >= chunk_bytes; }
// bytes of a written data chunk with its header and CRC
constexpr uint64_t written_bytes(uint64_t block_bytes, uint64_t chunk_bytes)
{
  return kDataHeaderBytes + (stored(block_bytes, chunk_bytes) ? chunk_bytes : block_bytes);
}
// the first four bytes of a written data chunk as a little-endian word
constexpr uint32_t written_header(uint64_t block_bytes, uint64_t chunk_bytes)
{
  return stored(block_bytes, chunk_bytes) ? kTypeStored | (uint32_t)(chunk_bytes + 4) << 8
                                          : kTypeCompressed | (uint32_t)(block_bytes + 4) << 8;
}
// The most a written stream takes: every chunk stored, the last one counted as a whole chunk too.
constexpr uint64_t frame_bound(uint64_t num_chunks, uint64_t chunk_bytes)
{
  return kIdentifierBytes + num_chunks * (chunk_bytes + kDataHeaderBytes);
}

// The first 16 bytes of a chunk, byte k in bits [8k, 8k + 8) of lo (k < 8) or hi: header, CRC and the longest
// preamble are 13.  Bytes past the end of the input are zero and not looked at.
struct Window
{
  uint64_t lo = 0, hi = 0;
  constexpr uint32_t byte(uint32_t k) const { return (uint32_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFFu); }
  constexpr uint32_t word(uint32_t k) const { return byte(k) | byte(k + 1) << 8 | byte(k + 2) << 16 | byte(k + 3) << 24; }
};

// the stream identifier's ten bytes: ff 06 00 00 "sNaPpY"
constexpr Window identifier()
{
  Window w;
  w.lo = 0x50614E73000006FFull;
  w.hi = 0x5970u;
  return w;
}

// the window of the chunk at p with avail bytes to the end of the input (the host's form; the walk kernel has its own)
constexpr Window window_of(const uint8_t* p, uint64_t avail)
{
  Window w;
  for (uint32_t k = 0; k < 16 && k < avail; ++k)
    (k < 8 ? w.lo : w.hi) |= (uint64_t)p[k] << (8 * (k & 7u));
  return w;
}

// A varint at bytes [at, at + room) of the window, room >= 1: false where it does not end within 5 bytes and room.
constexpr bool read_varint(const Window& w, uint32_t at, uint32_t room, uint64_t& value, uint32_t& bytes)
{
  value = 0;
  for (uint32_t k = 0; k < 5 && k < room; ++k) {
    const uint32_t b = w.byte(at + k);
    value |= (uint64_t)(b & 0x7Fu) << (7 * k);
    if (!(b & 0x80u)) {
      bytes = k + 1;
      return true;
    }
  }
  return false;
}

enum Kind : uint32_t { kSkipped = 0, kCompressed = 1, kStored = 2 };
struct Chunk
{
  uint32_t kind = kSkipped;
  uint32_t bytes = 0;      // of the whole chunk, header included: the next one stands that far on
  uint32_t payload = 0;    // data chunks: bytes behind the CRC (at offset 8 of the chunk)
  uint32_t content = 0;    // data chunks: bytes of output (the payload's own, or the preamble)
  uint32_t crc = 0;        // data chunks: the stored masked CRC-32C
};

// w: the window of a chunk, avail: bytes from its first to the end of the input (>= 1), first: it opens the input.
// Everything that shows without decoding, in this order: the header's room; the identifier's place, length, room,
// body; reserved types; a data chunk's length and (stored) size limit; the body's room; the preamble.
constexpr uint32_t parse_chunk(const Window& w, uint64_t avail, bool first, Chunk& c)
{
  if (avail < 4)
    return kTruncated;
  const uint32_t type = w.byte(0), length = w.word(0) >> 8;
  if (first && type != kTypeIdentifier)
    return kNoIdentifier;
  c.kind = kSkipped;
  c.bytes = 4 + length;
  if (type == kTypeIdentifier) {
    if (length != 6)
      return kBadIdentifier;
    if (avail < kIdentifierBytes)
      return kTruncated;
    return w.word(4) == identifier().word(4) && w.word(6) == identifier().word(6) ? kOk : kBadIdentifier;
  }
  if (type >= 0x02u && type <= 0x7Fu)
    return kReservedUnskippable;
  if (type >= 0x80u)
    return length > avail - 4 ? kTruncated : kOk;
  if (length < 4)
    return kShortChunk;
  if (type == kTypeStored && length - 4 > kMaxContent)
    return kStoredTooLarge;
  if (length > avail - 4)
    return kTruncated;
  c.payload = length - 4;
  c.crc = w.word(4);
  if (type == kTypeStored) {
    c.kind = kStored;
    c.content = c.payload;
    return kOk;
  }
  if (c.payload == 0)
    return kNoPayload;
  uint64_t value = 0;
  uint32_t used = 0;
  if (!read_varint(w, 8, c.payload, value, used))
    return kBadPreamble;
  if (value > kMaxContent)
    return kPreambleTooLarge;
  c.kind = kCompressed;
  c.content = (uint32_t)value;
  return kOk;
}

} // namespace szf
} // namespace hcamd
