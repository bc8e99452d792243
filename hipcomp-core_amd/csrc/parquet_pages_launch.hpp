// parquet_pages_launch.hpp -- host-callable entry points of a read of the pages of a batch of Parquet column chunks
// (parquet_pages_kernels.hip): what the Snappy manager's decompress_parquet_pages and get_parquet_pages_sizes
// (hlif.hip) are made of.  The arithmetic: parquet_pages_plan.hpp; the passes: DESIGN.md 26.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "parquet_pages_plan.hpp"

namespace hcamd {
namespace pqp {

// What is kept of an item through the call (device memory, the head of the scratch space).
struct Item
{
  const uint8_t* in;  // the column chunk
  uint64_t n;         // its bytes
  uint8_t* out;
  uint64_t capacity;
  Page* table;        // nullptr: none wanted
  uint64_t first;     // the number of its first listed page in the batch (the scan of the counts)
  uint64_t pages;     // listed pages it brings to the passes: 0 where its fate is sealed
  uint64_t total;     // what they decode to
  Walk w;             // the listing walk's: where it stands behind the passes so far
  uint32_t fate;      // parquet_pages_plan.hpp, Fate: what the counting walk made of the item
  uint32_t verdict;   // kVerdict*: what the passes found
  uint32_t bare;      // listed pages without a crc
  uint32_t pad;
  uint64_t largest;   // the most bytes a stored part of its pages has
};
static_assert(sizeof(Item) == kItemBytes, "parquet_pages_plan.hpp lays the scratch out with another size");
constexpr uint32_t kVerdictCannotDecompress = 1, kVerdictBadChecksum = 2;

// what the host reads once per call
struct Totals
{
  uint64_t pages;   // listed pages of all items that go to the passes
  uint64_t largest; // the most bytes one stored part of them has (the copy's launch is sized by it)
  uint32_t crc_sink; // (where the chunk CRC kernel's pass word goes: nobody reads it)
};
static_assert(sizeof(Totals) <= kTotalsBytes, "parquet_pages_plan.hpp lays the scratch out with another size");

// the arrays of a call (device memory, the caller's)
struct Batch
{
  const uint8_t* const* chunk_ptrs;
  const size_t* chunk_bytes;
  uint8_t* const* out_ptrs;
  const size_t* out_capacities;
  Page* const* page_ptrs; // nullptr: no tables
  const size_t* page_capacities;
  uint64_t items;
  uint32_t codec; // parquet_pages_plan.hpp, Codec
};

// The walk alone, asynchronous: per item the listed pages, what they decode to and the walk's status.
hipError_t launch_sizes(const Batch& b, size_t* num_pages, size_t* sizes, hipcompStatus_t* statuses, hipStream_t stream);

struct Stats
{
  uint64_t pages = 0, passes = 0;
};
// The read.  `scratch`: scratch_bytes(b.items, P) bytes, 16-byte aligned.  Synchronises the stream once, behind the
// counting walk and the scan of the counts, to read the Totals.  verify: the page CRCs are compared; require: an item
// with a page without one is hipcompErrorCannotVerifyChecksums.
hipError_t run(const Batch& b, size_t* actual_bytes, hipcompStatus_t* statuses, size_t* num_pages, uint8_t* scratch, uint64_t P,
               bool verify, bool require, hipStream_t stream, Stats* stats);

} // namespace pqp
} // namespace hcamd
