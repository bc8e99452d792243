// parquet_delta_launch.hpp -- the host-callable entry point of a decode of a batch of Parquet DELTA_BINARY_PACKED
// streams (parquet_delta_kernels.hip): what the Cascaded manager's decode_parquet_delta (hlif.hip) is made of.  The
// arithmetic and the rules: parquet_delta_plan.hpp; the kernel: DESIGN.md 28.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "parquet_delta_plan.hpp"

namespace hcamd {
namespace pqd {

// the arrays of a call (device memory, the caller's)
struct Batch
{
  const uint8_t* const* stream_ptrs;
  const size_t* stream_bytes;
  const size_t* num_values; // nullptr: every item decodes its header's count
  void* const* out_ptrs;
  const size_t* out_capacities; // elements
  size_t* value_counts;         // nullptr: not wanted
  size_t* consumed_bytes;       // nullptr: not wanted
  hipcompStatus_t* statuses;
  uint64_t items;
  uint32_t output; // parquet_delta_plan.hpp, Output
};

// One kernel, asynchronous, no scratch: a wavefront per item.  element_bytes: 4 or 8.
hipError_t launch(const Batch& b, uint32_t element_bytes, hipStream_t stream);

} // namespace pqd
} // namespace hcamd
