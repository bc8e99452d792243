// gather_launch.hpp -- host-callable launchers of the kernels of a read of many ranges (gather_kernels.hip; the
// arithmetic: gather_plan.hpp; hlif.hip, Core::decompress_ranges, says how they are driven).  Everything is
// stream-ordered.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "gather_plan.hpp"
#include "range_launch.hpp"

#include "hipcomp/shared_types.h"

namespace hcamd {

// The words of a call the device decides: the kernels behind the plan read them there, the host fetches them in
// one copy (the call's one synchronisation).
struct GatherHead
{
  uint32_t refused;     // 1: a range is invalid or the total does not fit out_bytes -- nothing is written
  uint32_t header_bad;  // 1: the container's header contradicts the configuration -- nothing is written
  uint32_t touched;     // distinct chunks the ranges touch
  uint32_t long_ranges; // ranges of more than kGatherSmallBytes bytes (entries of the long list)
  uint64_t total_bytes; // the sum of the lengths (saturated at 2^64 - 1)
  uint32_t long_span;   // the most chunks a long range touches
  uint32_t pad[9];
};
static_assert(sizeof(GatherHead) == 64, "the head is 64 bytes of the scratch space");

// a range of up to this many bytes is copied by 16 lanes, a longer one by a workgroup per piece
constexpr uint64_t kGatherSmallBytes = 4096;

// what the kernels know of the call (by value)
struct GatherCall
{
  const size_t* first = nullptr; // device: the ranges
  const size_t* num = nullptr;
  uint64_t ranges = 0;
  uint64_t decomp_bytes = 0, chunk_bytes = 0;
  uint32_t elem = 1;
  GatherHead* head = nullptr;
  uint64_t* offs = nullptr;        // ranges + 1: where each range lands in out, the total
  uint32_t* long_list = nullptr;   // the long ranges, in no particular order
  uint32_t* bitmap = nullptr;      // bit c: chunk c is touched
  uint32_t* word_rank = nullptr;   // set bits in front of word w inside its group of gather::kRankGroup words
  uint32_t* group_rank = nullptr;  // set bits in front of group g
  uint64_t words = 0;              // of the bitmap
};

// the lists of one pass (S entries each) and the slots
struct GatherLists
{
  const uint8_t** comp_ptrs = nullptr;
  size_t* comp_sizes = nullptr;
  size_t* caps = nullptr;
  uint8_t** out_ptrs = nullptr;
  size_t* actual = nullptr;
  hipcompStatus_t* statuses = nullptr;
  uint32_t* comp_sums = nullptr; // the container's stored checksums of the pass's chunks, gathered
  uint32_t* decomp_sums = nullptr;
};

// The plan, five launches: the bitmap zeroed; every range checked, the exclusive sum of the lengths, the head's
// refused / header_bad / total_bytes and *status (InvalidValue > CannotDecompress > Success); the touched chunks
// marked, the long ranges listed, `device_out_offsets` (may be null) written unless the call is refused or the
// header bad; the ranks, in two steps.  `c`: what the header is checked against, as in range_launch_list.
hipError_t gather_launch_plan(const GatherCall& g, const RangeContainer& c, uint64_t out_bytes, size_t* device_out_offsets,
                              hipcompStatus_t* status, hipStream_t stream);

// The chunk list of pass `pass` (ranks [pass * S, pass * S + count)): chunk of rank k into slot k % S.  The header
// test is range_launch_list's: a bad header gives every chunk a capacity of 0 and *status = CannotDecompress.
hipError_t gather_launch_list(const GatherCall& g, const RangeContainer& c, uint64_t sizes_at, uint64_t comp_sums_at,
                              uint64_t decomp_sums_at, uint64_t S, uint64_t pass, uint32_t count, const RangeSlots& slots,
                              const GatherLists& l, hipcompStatus_t* status, hipStream_t stream);

// Every piece a chunk of the pass gives to a range, from its slot to its place in out; nothing from a slot whose
// chunk failed.  `long_ranges`, `long_span`: the head's words, as the host fetched them.
hipError_t gather_launch_copy(const GatherCall& g, uint8_t* out, uint64_t S, uint64_t pass, uint32_t count,
                              uint32_t long_ranges, uint32_t long_span, const RangeSlots& slots, const GatherLists& l,
                              hipStream_t stream);

} // namespace hcamd
