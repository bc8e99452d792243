// range_launch.hpp -- host-callable launchers of the kernels of a ranged read (range_kernels.hip; the plan:
// range_plan.hpp; hlif.hip, Core::decompress_range, says how they are driven).  Everything is stream-ordered.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "checksum_launch.hpp"
#include "range_plan.hpp"

#include "hipcomp/shared_types.h"

namespace hcamd {

// what the list kernel checks the container's header against (as slab_streams_kernel of hlif.hip does) and where
// the container keeps its chunk offsets and its data
struct RangeContainer
{
  const uint8_t* container = nullptr;
  uint64_t offsets_at = 0, data_at = 0;
  uint64_t num_chunks = 0;
  uint32_t format = 0;
};

// the scratch slots of the edge chunks: slot k at slots + k * stride (16-byte aligned, stride >= chunk_bytes)
struct RangeSlots
{
  uint8_t* base = nullptr;
  uint64_t stride = 0;
};

// The chunk list of one pass, chunks [pass_first, pass_first + count) of the plan: interior chunks point into out
// at chunk start - first_byte, edge chunks at their slot.  A header that contradicts the manager or the
// configuration: every chunk gets a capacity of 0 (it fails in the decoder, nothing is written) and *status =
// hipcompErrorCannotDecompress.
hipError_t range_launch_list(const RangeContainer& c, const range::Plan& plan, uint64_t pass_first, uint32_t count,
                             uint8_t* out, const RangeSlots& slots, const uint8_t** comp_ptrs, uint8_t** out_ptrs,
                             size_t* caps, hipcompStatus_t* status, hipStream_t stream);

// The wanted span of every edge chunk of the pass from its slot to its place in out; nothing from a slot whose
// chunk failed (statuses[i] != hipcompSuccess or actual[i] != caps[i]).  After the pass's decode.
hipError_t range_launch_slices(const range::Plan& plan, uint64_t pass_first, uint32_t count, uint8_t* out,
                               const RangeSlots& slots, const hipcompStatus_t* statuses, const size_t* actual,
                               const size_t* caps, hipStream_t stream);

// The status of a verifying ranged read: crc_launch_finish_decompress without the two full-buffer words, which a
// partial read cannot check.  BadChecksum > CannotDecompress > CannotVerifyChecksums (`require` and a flag is
// false) > Success.
hipError_t range_launch_finish(const bool* comp_flag, const bool* decomp_flag, const CrcState* st, bool require,
                               hipcompStatus_t* status, hipStream_t stream);

} // namespace hcamd
