// parquet_plain_launch.hpp -- the host-callable entry points of the three calls that put a Parquet page's dense values
// into their rows (parquet_plain_kernels.hip): what the Cascaded manager's place_parquet_values, place_parquet_booleans
// and place_parquet_strings (hlif.hip) are made of.  The arithmetic and the rules: parquet_plain_plan.hpp; the kernels:
// DESIGN.md 30.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "parquet_plain_plan.hpp"

namespace hcamd {
namespace pqv {

// the arrays of a placing call (device memory, the caller's): the source and the rows of all three, then the outputs of each
struct PlaceBatch
{
  const uint8_t* const* src_ptrs;
  const size_t* src_bytes;    // of the whole buffer from the pointer
  const size_t* value_starts; // nullptr: every start is 0
  const size_t* num_values;
  const uint8_t* const* level_ptrs; // these three: all nullptr (dense) or all set
  const size_t* num_rows;
  const uint32_t* max_levels;
  uint8_t* const* validity_ptrs; // nullptr: not wanted
  hipcompStatus_t* statuses;
  uint64_t items;
  // fixed-width values (out_capacities in values) and booleans (in rows; out_ptrs are the values bitmaps)
  void* const* out_ptrs;
  const size_t* out_capacities;
  uint32_t value_bytes;
  uint32_t layout; // ValueLayout or StringLayout
  // strings
  const int32_t* const* value_offsets;
  int32_t* const* out_offsets;
  const size_t* offset_capacities; // elements
  uint8_t* const* out_bytes;
  const size_t* byte_capacities;
  size_t* out_byte_counts; // nullptr: not wanted
};

// One kernel each, asynchronous, no scratch: a wavefront per item.
hipError_t launch_place_values(const PlaceBatch& b, hipStream_t stream); // value_bytes: 1 to kMaxValueBytes
hipError_t launch_place_booleans(const PlaceBatch& b, hipStream_t stream);
hipError_t launch_place_strings(const PlaceBatch& b, hipStream_t stream);

} // namespace pqv
} // namespace hcamd
