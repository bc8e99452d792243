// zstd_batch.cpp -- C ABI of the batched Zstandard decoder (include/hipcomp/zstd.h).
//
// A format of this library's own, like Deflate (deflate_batch.cpp): the same argument order, null checks and
// status codes, in a library of its own, lib/libhipcomp_zstd.so.  Unlike Deflate the decoder takes temp space:
// one literal buffer per resident wave (zstd_sizing.hpp).
#include "hipcomp/zstd.h"

#include "host_common.hpp"
#include "zstd_launch.hpp"

using namespace hcamd;

extern "C" {

hipcompStatus_t hipcompBatchedZstdDecompressGetTempSize(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedZstdDecompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  *temp_bytes = zstd::temp_bytes(num_chunks, max_uncompressed_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes, size_t batch_size, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdGetDecompressSizeAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  if (batch_size == 0)
    return hipcompSuccess;
  zstd_launch_get_sizes(
      reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
      device_uncompressed_bytes, batch_size, stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard size HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDecompressAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes, size_t* device_actual_uncompressed_bytes, size_t batch_size,
    void* device_temp_ptr, size_t temp_bytes, void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdDecompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  if (batch_size == 0)
    return hipcompSuccess;
  HCAMD_REQUIRE_NOT_NULL(fn, device_temp_ptr);
  // The call does not know the largest chunk (the capacities are on the device): the temp space is shared out
  // evenly among the launch's waves, in units of 256 bytes up to 128 KiB, and has to hold the smallest size
  // the query returns for this batch.  A chunk whose literals outgrow its wave's share is refused.
  if (temp_bytes < zstd::temp_bytes(batch_size, 1))
    return fail(fn, "'temp_bytes' is smaller than hipcompBatchedZstdDecompressGetTempSize() asks for.");
  size_t per_wave = temp_bytes / zstd::waves_for(batch_size) / 256u * 256u;
  if (per_wave > zstd::kBlockMax)
    per_wave = zstd::kBlockMax;
  zstd_launch_decompress(
      reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
      device_uncompressed_bytes, batch_size, per_wave, device_temp_ptr,
      reinterpret_cast<uint8_t* const*>(device_uncompressed_ptrs), device_actual_uncompressed_bytes, device_statuses,
      stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard decompression HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

} // extern "C"
