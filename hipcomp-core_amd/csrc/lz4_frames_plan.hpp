// lz4_frames_plan.hpp -- the arithmetic of a read of a batch of LZ4 frames in one call (hlif.hip, decompress_frames
// and get_frames_decompressed_sizes of the LZ4 manager; the kernels: lz4_frames_kernels.hip): how the scratch space
// is laid out, how the data blocks of all items -- numbered through the batch in item order -- fall into passes, and
// what the eight bytes in front of an Arrow IPC buffer say about the item behind them.
//
// Pure arithmetic in constexpr functions: standard headers only, no HIP, no state.  The host and the kernels
// include this one copy.  tests/test_lz4_frames_plan_cpu.py compiles it with g++ alone under the address and
// undefined-behaviour sanitizers (tests/lz4_frames_plan_driver.cpp prints it) and compares it with a restatement.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace lz4fb {

constexpr uint64_t kMaxItems = uint64_t(1) << 20;

// ---- the scratch space ---------------------------------------------------------------------------------------
//   item states   kItemBytes each (the walk's state of the item, its buffers, its place in the block numbering)
//   totals        64 bytes: what the host reads after the scan of the items
//   ticket        64 bytes: the batched LZ4 decoder's chunk ticket counter
//   block lists   kEntryBytes per entry of a pass: the twelve lists of a single frame read and the item column
// every part 16-byte aligned (kItemBytes and the two 64s are multiples of 16; the lists start 16-byte aligned and
// every list of P entries is laid behind the last one as in a single frame read: 8-byte lists first).
constexpr uint64_t kItemBytes = 160;
constexpr uint64_t kReadEntryBytes = 9 * 8 + 3 * 4; // (lz4_frame_launch.hpp: the same number)
constexpr uint64_t kEntryBytes = kReadEntryBytes + 4; // + the item column
constexpr uint64_t kTotalsBytes = 64, kTicketBytes = 64;

constexpr uint64_t items_bytes(uint64_t items) { return items * kItemBytes; }
constexpr uint64_t totals_at(uint64_t items) { return items_bytes(items); }
constexpr uint64_t ticket_at(uint64_t items) { return totals_at(items) + kTotalsBytes; }
constexpr uint64_t lists_at(uint64_t items) { return ticket_at(items) + kTicketBytes; }
// a pass of P entries: the 8-byte lists, the 4-byte lists, the item column
constexpr uint64_t item_column_at(uint64_t items, uint64_t P) { return lists_at(items) + kReadEntryBytes * P; }
constexpr uint64_t scratch_bytes(uint64_t items, uint64_t P) { return lists_at(items) + kEntryBytes * P; }
// the least a scratch space has to hold: the states and two entries
constexpr uint64_t min_scratch_bytes(uint64_t items) { return scratch_bytes(items, 2); }
// entries of a pass in `room` bytes, at most `most`; 0: not even min_scratch_bytes
constexpr uint64_t pass_entries(uint64_t room, uint64_t items, uint64_t most)
{
  if (room < min_scratch_bytes(items))
    return 0;
  const uint64_t P = (room - lists_at(items)) / kEntryBytes;
  return P < most ? P : most;
}

// ---- the passes ----------------------------------------------------------------------------------------------
// Item i contributes blocks [first_i, first_i + blocks_i) to the numbering, first_i the exclusive sum of the counts
// before it; pass k takes blocks [k * P, (k + 1) * P).  An item's blocks may span passes, a pass may hold the
// blocks of many items, an item of no blocks is in no pass.
constexpr uint64_t passes_of(uint64_t total_blocks, uint64_t P) { return (total_blocks + P - 1) / P; }
constexpr uint64_t pass_count(uint64_t total_blocks, uint64_t P, uint64_t k)
{
  return total_blocks - k * P < P ? total_blocks - k * P : P;
}
// the entries of pass k that are item i's: [at, at + count) of the pass's lists
struct Slice
{
  uint64_t at = 0, count = 0;
};
constexpr Slice item_slice(uint64_t first, uint64_t blocks, uint64_t P, uint64_t k)
{
  Slice s;
  const uint64_t lo = k * P, hi = lo + P, end = first + blocks;
  const uint64_t a = first > lo ? first : lo, b = end < hi ? end : hi;
  if (a < b) {
    s.at = a - lo;
    s.count = b - a;
  }
  return s;
}

// ---- the prefix ----------------------------------------------------------------------------------------------
enum Prefix : uint32_t { kNone = 0, kArrowLength = 1 };
enum Kind : uint32_t {
  kFrames = 0, // the payload is frames (as decompress_frame reads them)
  kRaw = 1,    // the payload is the buffer itself (Arrow's -1)
  kEmpty = 2,  // nothing to do: success, size 0
  kRefused = 3 // hipcompErrorCannotDecompress before a byte is written
};
constexpr uint64_t kNoExpectedSize = ~uint64_t(0);
struct PrefixPlan
{
  uint32_t kind = kFrames;
  uint64_t payload_at = 0;                 // of the payload in the item
  uint64_t expected = kNoExpectedSize;     // the size the item has to decode to, or none
};
// prefix_word: the item's first eight bytes, little-endian (read only where item_bytes >= 8)
constexpr PrefixPlan prefix_plan(uint32_t prefix, uint64_t item_bytes, uint64_t prefix_word, uint64_t capacity)
{
  PrefixPlan p;
  if (prefix == kNone)
    return p;
  if (item_bytes == 0) {
    p.kind = kEmpty;
    p.expected = 0;
    return p;
  }
  p.kind = kRefused;
  if (item_bytes < 8)
    return p;
  p.payload_at = 8;
  if (prefix_word == ~uint64_t(0)) { // -1
    if (item_bytes - 8 > capacity)
      return p;
    p.kind = kRaw;
    p.expected = item_bytes - 8;
    return p;
  }
  if (prefix_word >> 63) // below -1
    return p;
  if (prefix_word > capacity)
    return p;
  p.kind = kFrames;
  p.expected = prefix_word;
  return p;
}
// what get_frames_decompressed_sizes says under kArrowLength: nothing behind the prefix is looked at
constexpr uint64_t prefix_size(uint64_t item_bytes, uint64_t prefix_word)
{
  if (item_bytes < 8)
    return 0;
  if (prefix_word == ~uint64_t(0))
    return item_bytes - 8;
  return (prefix_word >> 63) ? 0 : prefix_word;
}

} // namespace lz4fb
} // namespace hcamd
