// zstd_dict_compress_launch.hpp -- host-callable launchers of the Zstandard encoder with dictionaries
// (zstd_dict_compress_kernels.hip).  The compress launch has the shape, the temp space and the chunk-per-wave grid of
// ../zstd_compress/zstd_compress_launch.hpp; the prepare launch takes one wave per dictionary.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp.h"
#include "zstd_compress_sizing.hpp"
#include "zstd_dict_codes.hpp"

namespace hcamd {

// One launch on `stream`: dictionary i -> its blob (zstd_dict_codes.hpp), statuses[i] says how it went.
void zstd_dict_compress_launch_prepare(
    const uint8_t* const* dict_ptrs, const size_t* dict_bytes, size_t count, uint8_t* const* prepared_ptrs,
    const size_t* prepared_caps, hipcompStatus_t* statuses, hipStream_t stream);

// One launch on `stream`.  temp: zstd::enc_temp_bytes(batch, max_chunk_bytes) bytes, 4-byte aligned.
// max_chunk_bytes <= 32768; a larger chunk, and one whose blob is not valid, leaves with size 0.
void zstd_dict_compress_launch(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t max_chunk_bytes, size_t batch, void* temp,
    uint8_t* const* out_ptrs, size_t* out_bytes, const uint8_t* const* prepared, bool checksum, hipStream_t stream);

} // namespace hcamd
