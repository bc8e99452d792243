// parquet_dict_launch.hpp -- the host-callable entry points of the three calls that gather a Parquet dictionary's
// entries to rows (parquet_dict_kernels.hip): what the Cascaded manager's index_parquet_dictionary,
// gather_parquet_dictionary and gather_parquet_dictionary_strings (hlif.hip) are made of.  The arithmetic and the
// rules: parquet_dict_plan.hpp; the kernels: DESIGN.md 29.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "parquet_dict_plan.hpp"

namespace hcamd {
namespace pqg {

// the arrays of an index_parquet_dictionary call (device memory, the caller's)
struct IndexBatch
{
  const uint8_t* const* dict_ptrs;
  const size_t* dict_bytes;
  const size_t* num_entries;
  int32_t* const* offset_ptrs;
  const size_t* offset_capacities; // elements
  size_t* entry_counts;            // nullptr: not wanted
  hipcompStatus_t* statuses;
  uint64_t items;
};

// the arrays of a gathering call: the rows of both, then the outputs of each
struct GatherBatch
{
  const uint8_t* const* dict_ptrs;
  const size_t* dict_bytes;
  const size_t* dict_entries;
  const uint32_t* const* index_ptrs;
  const size_t* num_indices;
  const uint8_t* const* level_ptrs; // these three: all nullptr (dense) or all set
  const size_t* num_rows;
  const uint32_t* max_levels;
  uint8_t* const* validity_ptrs; // nullptr: not wanted
  hipcompStatus_t* statuses;
  uint64_t items;
  // fixed-width entries
  void* const* out_ptrs;
  const size_t* out_capacities; // entries
  uint32_t entry_bytes;
  // strings
  const int32_t* const* dict_offsets;
  int32_t* const* out_offsets;
  const size_t* offset_capacities; // elements
  uint8_t* const* out_bytes;
  const size_t* byte_capacities;
  size_t* out_byte_counts; // nullptr: not wanted
};

// One kernel each, asynchronous, no scratch: a wavefront per item.
hipError_t launch_index(const IndexBatch& b, hipStream_t stream);
hipError_t launch_gather(const GatherBatch& b, hipStream_t stream);         // entry_bytes: 1 to kMaxEntryBytes
hipError_t launch_gather_strings(const GatherBatch& b, hipStream_t stream);

} // namespace pqg
} // namespace hcamd
