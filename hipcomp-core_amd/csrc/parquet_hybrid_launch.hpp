// parquet_hybrid_launch.hpp -- the host-callable entry point of a decode of a batch of Parquet RLE / bit-packed
// hybrid streams (parquet_hybrid_kernels.hip): what the Cascaded manager's decode_parquet_hybrid (hlif.hip) is made
// of.  The arithmetic and the rules: parquet_hybrid_plan.hpp; the kernel: DESIGN.md 27.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "parquet_hybrid_plan.hpp"

namespace hcamd {
namespace pqh {

// the arrays of a call (device memory, the caller's)
struct Batch
{
  const uint8_t* const* stream_ptrs;
  const size_t* stream_bytes;
  const uint32_t* bit_widths; // nullptr allowed under kWidthPrefixed
  const size_t* num_values;
  void* const* out_ptrs;
  const size_t* out_capacities; // elements
  size_t* consumed_bytes;       // nullptr: not wanted
  const uint32_t* match_values; // nullptr with match_counts: not wanted
  size_t* match_counts;
  hipcompStatus_t* statuses;
  uint64_t items;
  uint32_t form; // parquet_hybrid_plan.hpp, Form
};

// One kernel, asynchronous, no scratch: a wavefront per item.  element_bytes: 1, 2 or 4.
hipError_t launch(const Batch& b, uint32_t element_bytes, hipStream_t stream);

} // namespace pqh
} // namespace hcamd
