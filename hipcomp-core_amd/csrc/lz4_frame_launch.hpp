// lz4_frame_launch.hpp -- host-callable launchers of the LZ4 frame kernels (lz4_frame_kernels.hip): what the LZ4
// manager's compress_frame / decompress_frame (hlif.hip) are made of, next to the batched LZ4 encoder and decoder
// (lz4_launch.hpp), which they use as they are.  DESIGN.md 20 has the passes.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "lz4_frame.hpp"

namespace hcamd {
namespace lz4f {

// ---- writing -------------------------------------------------------------------------------------------------
// The lists of a pass of `count` chunks (device memory, the manager's scratch).  slots: the batched encoder's
// outputs, stream_bytes what it reports.
struct WriteLists
{
  const uint8_t** in_ptrs;
  size_t* in_bytes;
  uint8_t** slots;
  size_t* stream_bytes;
  uint64_t* offsets; // of each block's size word in the frame (the scan's result)
  uint32_t* sums;    // block checksums
};

// the 15 header bytes; *cursor = 15
hipError_t launch_write_header(uint8_t* frame, uint64_t content_size, uint32_t block_max_code, bool block_checksums,
                               unsigned long long* cursor, hipStream_t stream);
// the chunk lists of a pass: chunk first + i of the input, slot i
hipError_t launch_write_lists(const uint8_t* in, uint64_t in_size, uint64_t chunk_bytes, uint64_t first, uint32_t count,
                              uint8_t* slots, uint64_t slot_bytes, const WriteLists& l, hipStream_t stream);
// offsets[i] = *cursor + the stored bytes of the blocks before i; *cursor moves past the pass
hipError_t launch_write_scan(const WriteLists& l, uint32_t count, bool block_checksums, unsigned long long* cursor,
                             hipStream_t stream);
// sums[i] = XXH32 of block i's stored bytes
hipError_t launch_write_sums(const WriteLists& l, uint32_t count, hipStream_t stream);
// size word, bytes and checksum of every block to its place
hipError_t launch_write_blocks(uint8_t* frame, const WriteLists& l, uint32_t count, uint64_t chunk_bytes,
                               bool block_checksums, hipStream_t stream);
// the EndMark at *cursor; *frame_bytes = the frame's length
hipError_t launch_write_end(uint8_t* frame, const unsigned long long* cursor, size_t* frame_bytes, hipStream_t stream);
hipError_t launch_set_size(size_t* word, size_t value, hipStream_t stream);

// ---- reading -------------------------------------------------------------------------------------------------
constexpr uint32_t kStored = 1, kLinked = 2, kBlockSum = 4, kLast = 8, kContentSum = 16; // + block maximum code << 8
// (a batch of frames alone, lz4_frames_kernels.hip: the entry is a whole item stored as it is, Arrow's -1, which no
// block maximum bounds; the walk never sets it)
constexpr uint32_t kRawItem = 32;
constexpr uint32_t kVerdictBadChecksum = 1, kVerdictCannotDecompress = 2;

// What the walk keeps between the passes of a call (device memory; the host reads it after configure's walk).
struct ReadState
{
  uint64_t pos;             // of the walk in the input
  uint64_t blocks, frames;  // data blocks / frames met so far
  uint64_t declared_sum;    // of the content sizes the frames declare
  uint64_t cur_content;     // the current frame's, or kNoContentSize
  uint64_t out_cursor;      // decoded bytes placed so far
  uint64_t frame_out_start; // where the output of the frame that runs into this pass starts
  uint32_t in_frame, cur_flags;
  uint32_t all_declared, bare_frames; // every frame declares a size; frames that carry no checksum at all
  uint32_t reason;          // the first refusal (lz4_frame.hpp)
  uint32_t done;            // the walk stands at the end of the input
  uint32_t count;           // entries of this pass
  uint32_t verdict;         // kVerdict* bits
  uint32_t walked;          // data blocks the walk itself stepped over since the reset: every call of it adds its own, nothing else does
};

// The entries of a pass, one per data block (device memory, the manager's scratch).
struct ReadLists
{
  const uint8_t** comp_ptrs;
  size_t* comp_bytes;    // the block's bytes in the frame
  size_t* batch_bytes;   // the same for the blocks the batched decoder takes, 0 for the others
  size_t* sizes;         // decoded bytes
  uint8_t** out_ptrs;
  size_t* caps;
  size_t* batch_caps;
  size_t* actual;
  uint64_t* aux;         // kLast entries: the declared content size or kNoContentSize
  uint32_t* flags;
  int32_t* head;         // the first entry of this entry's frame in this pass; -1: it began in an earlier pass
  hipcompStatus_t* statuses;
};
constexpr size_t kReadEntryBytes = 9 * 8 + 3 * 4;

hipError_t launch_read_reset(ReadState* st, hipStream_t stream);
// Follows the chain from where the last pass stopped, for up to `capacity` blocks; lists == nullptr: to the end of
// the input, counting only.  verify: an empty frame's content checksum is compared here.  skip: a device word that
// says the indexed read (lz4_frame_index_launch.hpp) has done it all -- the walk (a kernel of its own then) returns at once.
hipError_t launch_read_walk(const uint8_t* in, uint64_t in_bytes, ReadState* st, const ReadLists* lists, uint32_t capacity,
                            bool verify, hipStream_t stream, const uint32_t* skip = nullptr);
// sizes[] of the compressed blocks of linked frames (the batched decoder's parse-only pass gives the others' in actual[])
hipError_t launch_read_linked_sizes(const ReadLists& l, const ReadState* st, uint32_t capacity, hipStream_t stream);
// sizes[], out_ptrs[], caps[], batch_caps[] from a scan that continues from st->out_cursor; checks block maxima,
// the room (out_bytes) and the declared content sizes
hipError_t launch_read_scan(const ReadLists& l, ReadState* st, uint32_t capacity, uint8_t* out, uint64_t out_bytes,
                            hipStream_t stream);
hipError_t launch_read_stored(const ReadLists& l, const ReadState* st, uint32_t capacity, uint64_t largest_block,
                              hipStream_t stream);
hipError_t launch_read_linked(const ReadLists& l, ReadState* st, uint32_t capacity, uint8_t* out, hipStream_t stream);
// the batched decoder's statuses and sizes into st->verdict
hipError_t launch_read_verdict(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream);
hipError_t launch_read_block_sums(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream);
hipError_t launch_read_content_sums(const ReadLists& l, ReadState* st, uint32_t capacity, uint8_t* out, hipStream_t stream);
hipError_t launch_read_pass_end(const ReadLists& l, ReadState* st, uint8_t* out, hipStream_t stream);
// *status from the whole call: BadChecksum > CannotDecompress / NotSupported > CannotVerifyChecksums > Success
hipError_t launch_read_finish(const ReadState* st, uint64_t num_blocks, uint64_t out_bytes, bool require_checksums,
                              hipcompStatus_t* status, hipStream_t stream);

} // namespace lz4f
} // namespace hcamd
