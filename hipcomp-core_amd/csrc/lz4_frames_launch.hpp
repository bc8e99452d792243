// lz4_frames_launch.hpp -- host-callable launchers of the kernels of a read of a batch of LZ4 frames
// (lz4_frames_kernels.hip): what the LZ4 manager's decompress_frames and get_frames_decompressed_sizes (hlif.hip) are
// made of, next to the batched LZ4 decoder (lz4_launch.hpp).  The arithmetic: lz4_frames_plan.hpp; the passes:
// DESIGN.md 25.  Everything is asynchronous on `stream`.
#pragma once

#include "lz4_frame_launch.hpp"
#include "lz4_frames_plan.hpp"

namespace hcamd {
namespace lz4fb {

// What is kept of an item through the call (device memory, the head of the scratch space).
struct Item
{
  lz4f::ReadState st;  // the walk's, the item's own: its verdict word is the item's
  const uint8_t* in;   // the payload (behind the prefix)
  uint64_t n;          // its bytes
  uint8_t* out;
  uint64_t room;       // what may be written: the capacity, or the expected size where the prefix gives one
  uint64_t expected;   // kNoExpectedSize: none
  uint64_t first;      // the number of its first data block in the batch (the scan of the counts)
  uint32_t blocks;     // data blocks it brings to the passes
  uint32_t kind;       // lz4_frames_plan.hpp, Kind; kDeclared
  uint64_t next_cursor; // (the placing scan's: the cursor behind this pass)
};
// (size query) a kind of its own: every frame of the item declares its size, st.declared_sum is the answer
constexpr uint32_t kDeclared = 4;
static_assert(sizeof(Item) == kItemBytes, "lz4_frames_plan.hpp lays the scratch out with another size");
static_assert(kReadEntryBytes == lz4f::kReadEntryBytes, "lz4_frames_plan.hpp lays the scratch out with another size");

// what the host reads once per call
struct Totals
{
  uint64_t blocks;  // data blocks of all items
  uint64_t largest; // the most bytes one block can have: the largest payload, at most 4 MiB where it is frames
};

// the arrays of a call (device memory, the caller's)
struct Batch
{
  const uint8_t* const* item_ptrs;
  const size_t* item_bytes;
  uint8_t* const* out_ptrs;     // nullptr: the size query (room without end, nothing is written)
  const size_t* out_capacities;
  uint64_t items;
  uint32_t prefix;
};

// Walk, first time: every item's prefix rule, its state, and the count of its data blocks (a wave per item, one
// lane of it).  sizes_only: an item whose frames all declare their size brings no blocks.
hipError_t launch_begin(const Batch& b, Item* items, bool sizes_only, hipStream_t stream);
// first[] = exclusive sum of blocks[]; the totals
hipError_t launch_scan_items(Item* items, uint64_t num_items, Totals* totals, hipStream_t stream);
// Walk, pass k of P entries, `count` of them used: every item with blocks in it lists them at its place; item_col[e]
// = the item of entry e
hipError_t launch_list(Item* items, uint64_t num_items, const lz4f::ReadLists& l, uint32_t* item_col, uint64_t P, uint64_t k,
                       bool verify, hipStream_t stream);
hipError_t launch_linked_sizes(const lz4f::ReadLists& l, uint32_t count, hipStream_t stream);
// sizes[], out_ptrs[], caps[], batch_caps[]: a scan that starts anew at every item's first entry of the pass and
// continues from the item's cursor; checks block maxima, the item's room and the declared content sizes
// (pass_first: the number of the pass's first block in the batch)
hipError_t launch_place(Item* items, const lz4f::ReadLists& l, const uint32_t* item_col, uint32_t count, uint64_t pass_first,
                        hipStream_t stream);
hipError_t launch_batched_verdict(Item* items, const lz4f::ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream);
hipError_t launch_stored(const lz4f::ReadLists& l, uint32_t count, uint64_t largest_block, hipStream_t stream);
hipError_t launch_linked(Item* items, const lz4f::ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream);
hipError_t launch_block_sums(Item* items, const lz4f::ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream);
hipError_t launch_content_sums(Item* items, const lz4f::ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream);
// where the frame that runs out of this pass began, per item
hipError_t launch_pass_end(Item* items, const lz4f::ReadLists& l, const uint32_t* item_col, uint32_t count, hipStream_t stream);
// what lies behind every item's last block, then its status and size.  statuses == nullptr: the size query
// (sizes[i] = what the item decodes to, 0 where it is refused)
hipError_t launch_finish(Item* items, uint64_t num_items, bool verify, bool require_checksums, size_t* sizes,
                         hipcompStatus_t* statuses, hipStream_t stream);
// the size query under kArrowLength: the prefixes and nothing else
hipError_t launch_prefix_sizes(const Batch& b, size_t* sizes, hipStream_t stream);

} // namespace lz4fb
} // namespace hcamd
