// deflate_launch.hpp -- host-callable launchers of the Deflate kernels (deflate_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"

namespace hcamd {

// One launch on `stream`, no temp space; actual_bytes and statuses may be null.
void deflate_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps, size_t batch,
    uint8_t* const* out_ptrs, size_t* actual_bytes, hipcompStatus_t* statuses, hipStream_t stream);

// The same decode without an output: the size, or 0 for a stream that is refused.
void deflate_launch_get_sizes(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t* out_sizes, size_t batch, hipStream_t stream);

} // namespace hcamd
