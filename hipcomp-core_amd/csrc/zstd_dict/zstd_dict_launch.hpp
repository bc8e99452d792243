// zstd_dict_launch.hpp -- host-callable launchers of the dictionary kernels (zstd_dict_kernels.hip).  The temp
// space is that of the decoder without dictionaries: ../zstd/zstd_sizing.hpp, shared and not restated.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"
#include "zstd/zstd_sizing.hpp"
#include "zstd_dict.hpp"

namespace hcamd {

// One launch on `stream`, one wave per dictionary; every array is device memory, statuses is required.
void zstd_dict_launch_prepare(
    const uint8_t* const* dict_ptrs, const size_t* dict_bytes, size_t count, uint8_t* const* prepared_ptrs,
    const size_t* prepared_caps, hipcompStatus_t* statuses, hipStream_t stream);

// As zstd_launch_decompress, chunk i with the prepared dictionary prepared[i] (null: none).
void zstd_dict_launch_decompress(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps, size_t batch,
    size_t literal_bytes_per_wave, void* temp, uint8_t* const* out_ptrs, size_t* actual_bytes, hipcompStatus_t* statuses,
    const uint8_t* const* prepared, hipStream_t stream);

// As zstd_launch_get_sizes.
void zstd_dict_launch_get_sizes(
    const uint8_t* const* comp_ptrs, const size_t* comp_bytes, const uint8_t* const* prepared, size_t* out_sizes, size_t batch,
    hipStream_t stream);

} // namespace hcamd
