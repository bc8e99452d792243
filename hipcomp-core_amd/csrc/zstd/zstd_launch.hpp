// zstd_launch.hpp -- host-callable launchers of the Zstandard kernels (zstd_kernels.hip) and, through
// zstd_sizing.hpp, the temp-space formula that the C ABI's size query and the launch share.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "zstd_sizing.hpp"

namespace hcamd {

// One launch on `stream`.  temp: zstd::waves_for(batch) literal buffers of literal_bytes_per_wave bytes each
// (a multiple of 256, at most 128 KiB); actual_bytes and statuses may be null.
void zstd_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps, size_t batch,
    size_t literal_bytes_per_wave, void* temp, uint8_t* const* out_ptrs, size_t* actual_bytes, hipcompStatus_t* statuses,
    hipStream_t stream);

// The size query: the declared sizes, or the decode without an output; 0 for a chunk that is refused.
void zstd_launch_get_sizes(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t* out_sizes, size_t batch, hipStream_t stream);

} // namespace hcamd
