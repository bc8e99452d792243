// snappy_frame_index_launch.hpp -- host-callable launchers of the kernels of seekable Snappy framed streams
// (snappy_frame_index_kernels.hip; the index and its tests: snappy_frame_index.hpp; the passes they make up:
// hlif.hip).  Writing: the index behind the identifier of the stream compress_frame writes.  Reading:
// the entries of a pass from the index instead of the chain's walk -- the lists are snappy_frame_launch.hpp's, and
// the placing scan, the batched decoder, the stored-chunk copy and the CRC kernel work on them as they are.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "range_launch.hpp"
#include "snappy_frame_index.hpp"
#include "snappy_frame_launch.hpp"

namespace hcamd {
namespace szf {

// ---- writing -------------------------------------------------------------------------------------------------
// the identifier and bytes [0, 36) of the index behind it; *cursor = 10 + index_bytes(chunks): data chunk 0's place
hipError_t launch_index_write_begin(uint8_t* frame, unsigned long long* cursor, uint32_t chunks, uint32_t chunk_bytes,
                                    uint64_t content_bytes, hipStream_t stream);
// the first four bytes of a pass's data chunks (the ones write_chunks_kernel puts into the stream, from the same
// lists) to words first ... of the index at `index`
hipError_t launch_index_write_words(uint8_t* index, const WriteLists& l, uint64_t first, uint32_t count, hipStream_t stream);
// the masked CRC-32C behind the words, once they all stand
hipError_t launch_index_write_end(uint8_t* index, uint32_t chunks, hipStream_t stream);

// ---- reading -------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxIndexedStreams = 32;

struct IndexedEntry // a unit whose index is sound in itself, with the sum of its words inside the input
{
  uint64_t words_at, data_at; // of index word 0 / of data chunk 0 in the input
  uint64_t first_chunk;       // data chunks of the units before it
  uint64_t out_start;         // content bytes of the units before it
  uint64_t content_bytes;
  uint32_t chunks, chunk_bytes;
};

// What the indexed read keeps between the kernels of a call (device memory, the manager's scratch).
struct IndexState
{
  uint32_t ok;     // every test so far says the input is indexed units and nothing else
  uint32_t reason; // snappy_frame_index.hpp, the first one stored (any of the failing chunks')
  uint32_t skip;   // the indexed passes are through and held: the chain's passes have nothing to do
  uint32_t units;
  uint64_t chunks, content_bytes; // sums over the units
  uint64_t listed; // chunks the passes have listed so far
  uint64_t cursor; // where the next pass's first chunk stands in the input (inside unit `cur`)
  uint32_t cur;    // the unit the next pass begins in
  uint32_t reserved;
  IndexedEntry unit[kMaxIndexedStreams];
};

// Resets *ix and hops from unit to unit: one workgroup; per unit the identifier, the fields, the CRC, the sum of the
// chunk lengths and what stands behind them.  ix->ok where the whole input is indexed units.
hipError_t launch_index_begin(const uint8_t* in, uint64_t in_bytes, IndexState* ix, hipStream_t stream);
// The next `capacity` chunks: every chunk's scanned offset, the 16 bytes found there, its type, length and preamble
// are tested, and (lists) its entry is written -- payloads, batch_bytes, content, crcs, flags as the walk leaves
// them; st->count = capacity.  Where a test fails or *ix is not ok: ix->ok = 0, st->count = 0 and entries that ask
// nothing of anyone.  lists == nullptr: tests only, all chunks that are left (capacity is ignored).
hipError_t launch_index_list(const uint8_t* in, uint64_t in_bytes, IndexState* ix, ReadState* st, const ReadLists* lists,
                             uint32_t capacity, hipStream_t stream);
// a compressed chunk that did not decode to exactly its share: ix->ok = 0
hipError_t launch_index_verdict(const ReadLists& l, const ReadState* st, IndexState* ix, uint32_t capacity, hipStream_t stream);
// After the last pass.  The index held and listed num_chunks chunks: *st is what the chain's passes would leave
// (done, chunks, content, out_cursor; the verdict stays), ix->skip = 1, and the first `capacity` entries ask nothing
// of the batched decoder.  Else *st is reset for the chain's passes.
hipError_t launch_index_end(IndexState* ix, ReadState* st, const ReadLists& l, uint32_t capacity, const uint8_t* in,
                            uint64_t in_bytes, uint64_t num_chunks, hipStream_t stream);

// ---- ranged reads (after launch_index_begin and a tests-only launch_index_list said the whole input is indexed) ----
// The entries of chunks [pass_first, pass_first + count) of unit `unit` for a ranged read of that unit's content
// (plan: range_plan.hpp over the unit's content and chunk_bytes; out: where the plan's first byte lands): a chunk
// wholly inside the range points into out, an edge chunk at its slot.  caps[i]: the chunk's share, for
// range_launch_slices.  st->count = count.
hipError_t launch_index_range_list(const uint8_t* in, uint64_t in_bytes, const IndexState* ix, uint32_t unit,
                                   const range::Plan& plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                                   const RangeSlots& slots, const ReadLists& l, size_t* caps, ReadState* st, hipStream_t stream);
// stored chunks are copied, not decoded: their statuses[] / actual[] say so for range_launch_slices (a failed one's
// say that it failed)
hipError_t launch_index_range_settle(const ReadLists& l, const size_t* caps, const ReadState* st, uint32_t capacity,
                                     hipStream_t stream);
// *status from st->verdict: BadChecksum > CannotDecompress > Success
hipError_t launch_index_range_finish(const ReadState* st, hipcompStatus_t* status, hipStream_t stream);

} // namespace szf
} // namespace hcamd
