// zstd_compress_launch.hpp -- host-callable launcher of the Zstandard encoder (zstd_compress_kernels.hip) and,
// through zstd_compress_sizing.hpp, the temp-space formula that the C ABI's size query and the launch share.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "zstd_compress_sizing.hpp"

namespace hcamd {

// The launch is sized from what the build reports for zstd_compress_kernel (build/zstd_compress_kernels.gfx950.s,
// DESIGN.md section 17): 12 KiB of LDS per one-wave workgroup admit 12 workgroups per CU (zstd::kEncLdsPerWave
// asserts it), its registers (under 128 VGPRs, no scratch) 4 waves per SIMD, that is 16 per CU: LDS binds, and
// zstd::kEncMaxWaves = 256 CUs x 12 is what an MI355X holds at once.  On a device that holds fewer the rest of the
// grid waits its turn; that is correct, only temp space unused.
//
// One launch on `stream`.  temp: zstd::enc_temp_bytes(batch, max_chunk_bytes) bytes, 4-byte aligned.
// max_chunk_bytes <= 65536; a larger chunk leaves with size 0.
void zstd_launch_compress(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t max_chunk_bytes, size_t batch, void* temp,
    uint8_t* const* out_ptrs, size_t* out_bytes, bool checksum, hipStream_t stream);

} // namespace hcamd
