// lz4_frame_index.hpp -- the block index of a seekable LZ4 frame: an LZ4 skippable frame that stands immediately in
// front of the frame it describes and holds that frame's size words, so that a reader finds every block by a scan
// instead of following the chain.  The writer, the parser with a reason for every refusal, and the size and offset
// arithmetic (the frame format itself: lz4_frame.hpp).  All fields little-endian:
//
//    0  u32  0x184D2A54                 skippable magic (nibble 4; E is Zstandard's seekable format)
//    4  u32  36 + 4N                    payload bytes
//    8  8 B  "HCLZ4IDX"
//   16  u32  version = 1
//   20  u32  flags: bit 0 = every block is followed by its checksum; all other bits 0
//   24  u32  block_bytes                content bytes of every block but the last, 1 .. 4 MiB
//   28  u32  N                          data blocks
//   32  u64  content_bytes              N == ceil(content_bytes / block_bytes)
//   40  N x u32                         the size word of block i as it stands in the frame (bit 31: stored)
//   40 + 4N  u32  XXH32(payload[0, 32 + 4N), 0)
//
// The index is untrusted: it applies only if it is sound in itself, the next byte starts a descriptor of the form
// compress_frame writes with the same numbers, and every word is found where the scan of the words says it stands,
// with the EndMark behind the last.  By induction that is the chain a reader without the index follows.
//
// Standard headers and constexpr only: the kernels (lz4_frame_index_kernels.hip), the manager (hlif.hip) and the
// CPU driver of tests/test_lz4_frame_index_cpu.py include this one text.
#pragma once

#include <cstddef>
#include <cstdint>

#include "lz4_frame.hpp"

namespace hcamd {
namespace lz4f {

constexpr uint32_t kIndexMagic = 0x184D2A54u;
constexpr uint32_t kIndexFormatVersion = 1;
constexpr uint32_t kIndexFlagBlockSums = 1;
constexpr uint32_t kIndexFixedPayload = 36; // signature .. content_bytes, and the hash
constexpr uint32_t kIndexWordsAt = 40;      // of word 0 from the magic
constexpr uint32_t kIndexMaxBlockBytes = 4u << 20;
constexpr uint8_t kIndexSignatureBytes[8] = {'H', 'C', 'L', 'Z', '4', 'I', 'D', 'X'};

constexpr uint64_t index_bytes(uint64_t blocks) { return 44 + 4 * blocks; }
// the most compress_frame(..., Leading) takes: the index and the frame's bound (lz4_frame.hpp)
constexpr uint64_t indexed_frame_bound(uint64_t num_chunks, uint64_t chunk_bytes, bool block_checksums)
{
  return index_bytes(num_chunks) + frame_bound(num_chunks, chunk_bytes, block_checksums);
}

// why an index does not apply, in the order of the tests; the numbers are the test drivers' and the tests' too
enum IndexReason : uint32_t {
  kIndexOk = 0,
  kIndexNotThere = 1,      // fewer than 8 bytes, or not the index's magic (another skippable frame, a frame)
  kIndexPayloadSize = 2,   // below 36, beyond the end of the input, or not 36 + 4N
  kIndexSignature = 3,
  kIndexVersion = 4,
  kIndexFlags = 5,         // a reserved bit
  kIndexBlockBytes = 6,    // 0 or above 4 MiB
  kIndexCount = 7,         // N is not ceil(content_bytes / block_bytes)
  kIndexHash = 8,
  kIndexNoFrame = 9,       // what follows is no descriptor parse_descriptor accepts (the end, a skippable frame, DictID)
  kIndexFrameForm = 10,    // linked blocks, C.Checksum, or no C.Size
  kIndexContentSize = 11,  // C.Size is not content_bytes
  kIndexBlockSums = 12,    // B.Checksum is not flag bit 0
  kIndexBlockMax = 13,     // block_bytes above the frame's block maximum
  kIndexOffset = 14,       // a scanned offset (a block's or the EndMark's) leaves no four bytes inside the input
  kIndexWord = 15,         // the size word found there is not the index's
  kIndexLength = 16,       // a length of 0 or above block_bytes
  kIndexStoredLength = 17, // a stored block that does not hold its content bytes
  kIndexEndMark = 18,      // no EndMark behind the last block
  kIndexDecode = 19,       // (device) a compressed block did not produce exactly its content bytes
  kIndexTooManyFrames = 20, // (device) more indexed frames than the reader's table holds, or 2^32 blocks
  kIndexReasons = 21
};

struct IndexHead
{
  uint32_t flags = 0, block_bytes = 0, blocks = 0;
  uint64_t content_bytes = 0;
  constexpr bool block_checksums() const { return flags & kIndexFlagBlockSums; }
};

constexpr uint64_t index_read64(const uint8_t* p)
{
  return (uint64_t)xxh32::read32(p) | ((uint64_t)xxh32::read32(p + 4) << 32);
}
constexpr uint64_t blocks_of(uint64_t content_bytes, uint32_t block_bytes)
{
  return content_bytes / block_bytes + (content_bytes % block_bytes ? 1 : 0);
}
// content bytes of block i of n
constexpr uint64_t block_content(const IndexHead& h, uint64_t i)
{
  return i + 1 < h.blocks ? h.block_bytes : h.content_bytes - (uint64_t)h.block_bytes * i;
}
// bytes of a block in the frame with its size word and checksum
constexpr uint64_t indexed_block_bytes(uint32_t word, bool block_checksums)
{
  return 4 + (uint64_t)(word & ~kStoredBit) + (block_checksums ? 4 : 0);
}

// p: where a skippable frame's magic may stand, avail: bytes from there to the end of the input.  Everything but
// the hash (index_hash_fits): the kernels hash with a wave.
constexpr uint32_t parse_index_fields(const uint8_t* p, uint64_t avail, IndexHead& h)
{
  if (avail < 8 || xxh32::read32(p) != kIndexMagic)
    return kIndexNotThere;
  const uint32_t payload = xxh32::read32(p + 4);
  if (payload < kIndexFixedPayload || payload > avail - 8)
    return kIndexPayloadSize;
  for (int k = 0; k < 8; ++k)
    if (p[8 + k] != kIndexSignatureBytes[k])
      return kIndexSignature;
  if (xxh32::read32(p + 16) != kIndexFormatVersion)
    return kIndexVersion;
  h.flags = xxh32::read32(p + 20);
  if (h.flags & ~kIndexFlagBlockSums)
    return kIndexFlags;
  h.block_bytes = xxh32::read32(p + 24);
  if (h.block_bytes == 0 || h.block_bytes > kIndexMaxBlockBytes)
    return kIndexBlockBytes;
  h.blocks = xxh32::read32(p + 28);
  h.content_bytes = index_read64(p + 32);
  if ((uint64_t)payload != kIndexFixedPayload + 4 * (uint64_t)h.blocks)
    return kIndexPayloadSize;
  if (blocks_of(h.content_bytes, h.block_bytes) != h.blocks)
    return kIndexCount;
  return kIndexOk;
}

// (after parse_index_fields) the hash behind the words against the one of the bytes in front of it
constexpr bool index_hash_fits(const uint8_t* p, const IndexHead& h)
{
  const uint64_t hashed = 32 + 4 * (uint64_t)h.blocks;
  return xxh32::hash(p + 8, hashed, 0) == xxh32::read32(p + 8 + hashed);
}

// p: the byte behind the index, avail: bytes from there to the end of the input
constexpr uint32_t check_indexed_descriptor(const IndexHead& h, const uint8_t* p, uint64_t avail, Descriptor& d)
{
  if (parse_descriptor(p, avail, d) != kOk)
    return kIndexNoFrame;
  if (d.linked || d.content_checksum || !d.has_content_size)
    return kIndexFrameForm;
  if (d.content_size != h.content_bytes)
    return kIndexContentSize;
  if (d.block_checksums != h.block_checksums())
    return kIndexBlockSums;
  if (h.block_bytes > d.block_max)
    return kIndexBlockMax;
  return kIndexOk;
}

// word: index word i, found: the u32 at block i's scanned offset, content: block i's content bytes
constexpr uint32_t check_indexed_block(uint32_t word, uint32_t found, uint64_t content, uint32_t block_bytes)
{
  if (found != word)
    return kIndexWord;
  const uint32_t len = word & ~kStoredBit;
  if (len < 1 || len > block_bytes)
    return kIndexLength;
  if ((word & kStoredBit) && len != content)
    return kIndexStoredLength;
  return kIndexOk;
}

// the word behind the last block (the chain's reader takes either form of a zero length for the EndMark)
constexpr bool is_end_mark(uint32_t word) { return (word & ~kStoredBit) == 0; }

// ---- the writer ------------------------------------------------------------------------------------------------
// bytes [0, 40): everything in front of the words
constexpr void write_index_fields(uint8_t* p, uint32_t blocks, uint32_t block_bytes, uint64_t content_bytes,
                                  bool block_checksums)
{
  const uint32_t words[10] = {kIndexMagic, kIndexFixedPayload + 4 * blocks, 0, 0, kIndexFormatVersion,
                              block_checksums ? kIndexFlagBlockSums : 0u, block_bytes, blocks,
                              (uint32_t)content_bytes, (uint32_t)(content_bytes >> 32)};
  for (int w = 0; w < 10; ++w)
    for (int k = 0; k < 4; ++k)
      p[4 * w + k] = w == 2 || w == 3 ? kIndexSignatureBytes[4 * (w - 2) + k] : (uint8_t)(words[w] >> (8 * k));
}

// the whole index of `blocks` size words into p[0, index_bytes(blocks))
constexpr void write_index(uint8_t* p, const uint32_t* size_words, uint32_t blocks, uint32_t block_bytes,
                           uint64_t content_bytes, bool block_checksums)
{
  write_index_fields(p, blocks, block_bytes, content_bytes, block_checksums);
  for (uint32_t i = 0; i < blocks; ++i)
    for (int k = 0; k < 4; ++k)
      p[kIndexWordsAt + 4 * (uint64_t)i + k] = (uint8_t)(size_words[i] >> (8 * k));
  const uint64_t hashed = 32 + 4 * (uint64_t)blocks;
  const uint32_t hash = xxh32::hash(p + 8, hashed, 0);
  for (int k = 0; k < 4; ++k)
    p[8 + hashed + k] = (uint8_t)(hash >> (8 * k));
}

// ---- the whole test, one block after the other (the kernels do the blocks in parallel over a scan) ---------------
struct IndexedFrame
{
  IndexHead head;
  uint64_t words_at = 0;  // of index word 0 in the input
  uint64_t blocks_at = 0; // of block 0's size word: the byte behind the descriptor
  uint64_t end = 0;       // the byte behind the EndMark
  uint32_t block_max_code = 0;
};

// in[0, n): the input, at: where the index's magic may stand
constexpr uint32_t index_applies(const uint8_t* in, uint64_t n, uint64_t at, IndexedFrame& f)
{
  uint32_t r = parse_index_fields(in + at, n - at, f.head);
  if (r != kIndexOk)
    return r;
  if (!index_hash_fits(in + at, f.head))
    return kIndexHash;
  f.words_at = at + kIndexWordsAt;
  const uint64_t frame_at = at + index_bytes(f.head.blocks);
  Descriptor d;
  r = check_indexed_descriptor(f.head, in + frame_at, n - frame_at, d);
  if (r != kIndexOk)
    return r;
  f.block_max_code = code_for_chunk(d.block_max);
  f.blocks_at = frame_at + d.header_bytes;
  uint64_t pos = f.blocks_at;
  for (uint64_t i = 0; i < f.head.blocks; ++i) {
    if (pos > n || n - pos < 4)
      return kIndexOffset;
    const uint32_t word = xxh32::read32(in + f.words_at + 4 * i);
    r = check_indexed_block(word, xxh32::read32(in + pos), block_content(f.head, i), f.head.block_bytes);
    if (r != kIndexOk)
      return r;
    pos += indexed_block_bytes(word, f.head.block_checksums());
  }
  if (pos > n || n - pos < 4)
    return kIndexOffset;
  if (!is_end_mark(xxh32::read32(in + pos)))
    return kIndexEndMark;
  f.end = pos + 4;
  return kIndexOk;
}

// The whole input: kIndexOk where it is indexed frames and nothing else but skippable frames of other magics
// between them -- the inputs the indexed read takes; frames / blocks / content_bytes: their sums.  Anything else
// gives the first reason met, and the reader goes the chain's way.
constexpr uint32_t input_is_indexed(const uint8_t* in, uint64_t n, uint64_t& frames, uint64_t& blocks, uint64_t& content_bytes)
{
  uint64_t pos = 0;
  frames = blocks = content_bytes = 0;
  while (pos < n) {
    if (n - pos >= 8 && is_skippable(xxh32::read32(in + pos)) && xxh32::read32(in + pos) != kIndexMagic) {
      const uint64_t size = xxh32::read32(in + pos + 4);
      if (size > n - pos - 8)
        return kIndexNotThere;
      pos += 8 + size;
      continue;
    }
    IndexedFrame f;
    const uint32_t r = index_applies(in, n, pos, f);
    if (r != kIndexOk)
      return r;
    frames += 1;
    blocks += f.head.blocks;
    content_bytes += f.head.content_bytes;
    pos = f.end;
  }
  return kIndexOk;
}

} // namespace lz4f
} // namespace hcamd
