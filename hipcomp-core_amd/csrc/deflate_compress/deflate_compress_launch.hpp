// deflate_compress_launch.hpp -- host-callable launcher of the Deflate encoder (deflate_compress_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace hcamd {

// One wave per workgroup and at most this many of them: a larger batch is walked grid-stride.  It is what an
// MI355X holds at once -- 256 CUs x 12 workgroups: the kernel's registers (over 128 VGPRs) admit 3 waves per SIMD,
// its 10.4 KiB of LDS would admit 15 workgroups per CU -- so no token buffer belongs to a
// wave that only waits.  On a device that holds fewer the rest of the grid waits its turn; that is correct, only
// temp space unused.
constexpr size_t kDeflateCompressMaxWaves = 256 * 12;

// the wave's token buffer in 32-bit records, for chunks of at most max_chunk_bytes
size_t deflate_compress_records_per_wave(size_t max_chunk_bytes);
// waves the launch uses for `batch` chunks
size_t deflate_compress_waves(size_t batch);

// One launch on `stream`.  temp: deflate_compress_waves(batch) * deflate_compress_records_per_wave(max) * 4
// bytes, 4-byte aligned.  max_chunk_bytes <= 65536; a larger chunk leaves with size 0.
void deflate_launch_compress(
    const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t max_chunk_bytes, size_t batch, void* temp,
    uint8_t* const* out_ptrs, size_t* out_bytes, hipStream_t stream);

} // namespace hcamd
