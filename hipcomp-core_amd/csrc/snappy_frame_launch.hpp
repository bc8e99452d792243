// snappy_frame_launch.hpp -- host-callable launchers of the Snappy framing kernels (snappy_frame_kernels.hip): what
// the Snappy manager's compress_frame / decompress_frame (hlif.hip) are made of, next to the batched Snappy encoder
// and decoder (snappy_launch.hpp), which they use as they are.  DESIGN.md 21 has the passes.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "snappy_frame.hpp"

namespace hcamd {
namespace szf {

// ---- writing -------------------------------------------------------------------------------------------------
// The lists of a pass of `count` chunks (device memory, the manager's scratch).  slots: the batched encoder's
// outputs, block_bytes what it reports.
struct WriteLists
{
  const uint8_t** in_ptrs;
  size_t* in_bytes;
  uint8_t** slots;
  size_t* block_bytes;
  uint64_t* offsets; // of each data chunk's header in the stream (the scan's result)
  uint32_t* crcs;    // masked CRC-32C of the input chunks
};
constexpr size_t kWriteEntryBytes = 5 * 8 + 4;

// the 10 identifier bytes; *cursor = 10
hipError_t launch_write_begin(uint8_t* frame, unsigned long long* cursor, hipStream_t stream);
// the chunk lists of a pass: chunk first + i of the input, slot i
hipError_t launch_write_lists(const uint8_t* in, uint64_t in_size, uint64_t chunk_bytes, uint64_t first, uint32_t count,
                              uint8_t* slots, uint64_t slot_bytes, const WriteLists& l, hipStream_t stream);
// crcs[i] = mask(CRC-32C of input chunk i)
hipError_t launch_write_crcs(const WriteLists& l, uint32_t count, hipStream_t stream);
// offsets[i] = *cursor + the written bytes of the chunks before i; *cursor moves past the pass
hipError_t launch_write_scan(const WriteLists& l, uint32_t count, unsigned long long* cursor, hipStream_t stream);
// header, CRC and bytes of every data chunk to its place
hipError_t launch_write_chunks(uint8_t* frame, const WriteLists& l, uint32_t count, uint64_t chunk_bytes, hipStream_t stream);
// *frame_bytes = *cursor
hipError_t launch_write_end(const unsigned long long* cursor, size_t* frame_bytes, hipStream_t stream);
hipError_t launch_set_size(size_t* word, size_t value, hipStream_t stream);

// ---- reading -------------------------------------------------------------------------------------------------
constexpr uint32_t kEntryStored = 1, kEntryFailed = 2;
constexpr uint32_t kVerdictBadChecksum = 1, kVerdictCannotDecompress = 2;

// What the walk keeps between the passes of a call (device memory; the host reads it after configure's walk).
struct ReadState
{
  uint64_t pos;        // of the walk in the input
  uint64_t chunks;     // data chunks met so far
  uint64_t content;    // the bytes they declare: stored lengths and preambles
  uint64_t out_cursor; // decoded bytes placed so far
  uint32_t started;    // the input's first chunk is behind the walk
  uint32_t reason;     // the first refusal (snappy_frame.hpp)
  uint32_t done;       // the walk stands at the end of the input
  uint32_t count;      // entries of this pass
  uint32_t verdict;    // kVerdict* bits
  uint32_t walked;     // data chunks the walk stepped over since the reset: each call adds its own count once
};

// The entries of a pass, one per data chunk (device memory, the manager's scratch).
struct ReadLists
{
  const uint8_t** payloads;
  size_t* batch_bytes;   // the payload's bytes for the chunks the batched decoder takes, 0 for the others
  uint8_t** out_ptrs;
  size_t* batch_caps;    // the preamble for the same chunks
  size_t* actual;
  uint32_t* content;     // bytes of output
  uint32_t* crcs;        // the stored masked CRC-32C
  uint32_t* flags;       // kEntry*
  hipcompStatus_t* statuses;
};
constexpr size_t kReadEntryBytes = 5 * 8 + 4 * 4;

hipError_t launch_read_reset(ReadState* st, hipStream_t stream);
// Follows the chain from where the last pass stopped until `capacity` data chunks are listed and the next one shows,
// or to the end of the input; lists == nullptr: to the end, counting only.  skip (device memory): where *skip is set
// the call does nothing -- the walk behind an indexed read's passes (snappy_frame_index_launch.hpp).
hipError_t launch_read_walk(const uint8_t* in, uint64_t in_bytes, ReadState* st, const ReadLists* lists, uint32_t capacity,
                            hipStream_t stream, const uint32_t* skip = nullptr);
// out_ptrs[] and batch_caps[] from a scan of content[] that continues from st->out_cursor; an entry without room in
// out[0, out_bytes) is failed and asks nothing of the decoder
hipError_t launch_read_scan(const ReadLists& l, ReadState* st, uint8_t* out, uint64_t out_bytes, hipStream_t stream);
// largest_chunk: what the workgroups per chunk are sized for (any chunk is copied whole by as many as there are)
hipError_t launch_read_stored(const ReadLists& l, const ReadState* st, uint32_t capacity, uint64_t largest_chunk,
                              hipStream_t stream);
// the batched decoder's statuses and sizes into the entries' flags and st->verdict
hipError_t launch_read_verdict(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream);
// mask(CRC-32C of the output) against crcs[], for the entries that did not fail
hipError_t launch_read_crcs(const ReadLists& l, ReadState* st, uint32_t capacity, hipStream_t stream);
// *status from the whole call: BadChecksum > CannotDecompress > Success
hipError_t launch_read_finish(const ReadState* st, uint64_t num_chunks, uint64_t out_bytes, hipcompStatus_t* status,
                              hipStream_t stream);

} // namespace szf
} // namespace hcamd
