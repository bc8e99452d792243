// lz4_frame_index_launch.hpp -- host-callable launchers of the kernels of seekable LZ4 frames
// (lz4_frame_index_kernels.hip; the index and its tests: lz4_frame_index.hpp; the passes they make up: hlif.hip,
// DESIGN.md 22).  Writing: the index in front of the frame compress_frame writes.  Reading: the entries of a pass
// from the index instead of the chain's walk and the parse-only pass -- the lists are lz4_frame_launch.hpp's, and
// the batched decoder, the stored-block copy and the block checksums work on them as they are.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "lz4_frame_index.hpp"
#include "lz4_frame_launch.hpp"
#include "range_launch.hpp"

namespace hcamd {
namespace lz4f {

// ---- writing -------------------------------------------------------------------------------------------------
// bytes [0, 40) of the index at `index`: everything in front of the words
hipError_t launch_index_write_fields(uint8_t* index, uint32_t blocks, uint32_t block_bytes, uint64_t content_bytes,
                                     bool block_checksums, hipStream_t stream);
// the size words of a pass's blocks (the ones write_blocks_kernel puts into the frame) to words first ... of the index
hipError_t launch_index_write_words(uint8_t* index, const WriteLists& l, uint64_t first, uint32_t count, hipStream_t stream);
// the hash behind the words; *frame_bytes (the frame's length, written by launch_write_end) += the index's
hipError_t launch_index_write_end(uint8_t* index, uint32_t blocks, size_t* frame_bytes, hipStream_t stream);

// ---- reading -------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxIndexedFrames = 32;

struct IndexedEntry // a frame whose index is sound in itself and stands in front of a descriptor that fits it
{
  uint64_t words_at, blocks_at; // of index word 0 / of block 0's size word in the input
  uint64_t first_block;         // data blocks of the frames before it
  uint64_t out_start;           // content bytes of the frames before it
  uint64_t content_bytes;
  uint32_t blocks, block_bytes;
  uint32_t flags, reserved;     // kBlockSum | block maximum code << 8 (lz4_frame_launch.hpp)
};

// What the indexed read keeps between the kernels of a call (device memory, the manager's scratch).
struct IndexState
{
  uint32_t ok;          // every test so far says the input is indexed frames and nothing else
  uint32_t reason;      // lz4_frame_index.hpp, the first one stored (any of the failing blocks')
  uint32_t skip;        // the indexed passes are through and held: the chain's passes have nothing to do
  uint32_t frames;
  uint64_t blocks, content_bytes; // sums over the frames
  uint64_t listed;      // blocks the passes have listed so far
  uint64_t cursor;      // where the next pass's first block stands in the input (inside frame `cur`)
  uint32_t cur;         // the frame the next pass begins in
  uint32_t bare_frames; // frames without block checksums
  uint64_t reserved;
  IndexedEntry frame[kMaxIndexedFrames];
};

// Resets *ix and hops from frame to frame: one workgroup; per frame the fields, the descriptor, the hash, the sum of
// the block lengths and the EndMark behind them.  ix->ok where the whole input is indexed frames.
hipError_t launch_index_begin(const uint8_t* in, uint64_t in_bytes, IndexState* ix, hipStream_t stream);
// The next `capacity` blocks: every block's scanned offset, the word found there and its length are tested, and
// (lists) its entry is written -- comp_ptrs .. statuses as the walk, the parse and read_scan_kernel leave them;
// st->count = capacity.  Where a test fails or *ix is not ok: ix->ok = 0, st->count = 0 and entries that ask
// nothing of the batched decoder.  lists == nullptr: tests only, all blocks that are left (capacity is ignored).
hipError_t launch_index_list(const uint8_t* in, uint64_t in_bytes, IndexState* ix, ReadState* st, const ReadLists* lists,
                             uint32_t capacity, uint8_t* out, uint64_t out_bytes, hipStream_t stream);
// a compressed block that did not decode to exactly its content bytes: ix->ok = 0
hipError_t launch_index_verdict(const ReadLists& l, const ReadState* st, IndexState* ix, uint32_t capacity, hipStream_t stream);
// After the last pass.  The index held and listed num_blocks blocks: *st is what the chain's passes would leave
// (done, blocks, out_cursor, bare_frames; the checksum verdict stays), ix->skip = 1, and the first `capacity`
// entries ask nothing of the batched decoder.  Else *st is reset for the chain's passes.
hipError_t launch_index_end(IndexState* ix, ReadState* st, const ReadLists& l, uint32_t capacity, uint64_t in_bytes,
                            uint64_t num_blocks, hipStream_t stream);

// ---- ranged reads (after launch_index_begin and a tests-only launch_index_list said the whole input is indexed) ----
// The entries of blocks [pass_first, pass_first + count) of frame `frame` for a ranged read of that frame's content
// (plan: range_plan.hpp over the frame's content and block_bytes; out: where the plan's first byte lands): a block
// wholly inside the range points into out, an edge block at its slot.  st->count = count.
hipError_t launch_index_range_list(const uint8_t* in, uint64_t in_bytes, const IndexState* ix, uint32_t frame,
                                   const range::Plan& plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                                   const RangeSlots& slots, const ReadLists& l, ReadState* st, hipStream_t stream);
// stored blocks are copied, not decoded: their statuses[] / actual[] say so for range_launch_slices
hipError_t launch_index_range_settle(const ReadLists& l, const ReadState* st, uint32_t capacity, hipStream_t stream);
// *status from st->verdict: BadChecksum > CannotDecompress > CannotVerifyChecksums (cannot_verify) > Success
hipError_t launch_index_range_finish(const ReadState* st, bool cannot_verify, hipcompStatus_t* status, hipStream_t stream);

} // namespace lz4f
} // namespace hcamd
