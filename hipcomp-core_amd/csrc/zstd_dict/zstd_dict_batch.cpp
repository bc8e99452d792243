// zstd_dict_batch.cpp -- C ABI of the batched Zstandard decoder with dictionaries (include/hipcomp/zstd_dict.h).
//
// The sibling of ../zstd/zstd_batch.cpp in a library of its own, lib/libhipcomp_zstd_dict.so: the same argument
// order, null checks and status codes, the same temp space (zstd_sizing.hpp), and one more array per call, the
// chunks' prepared dictionaries.
#include "hipcomp/zstd_dict.h"

#include "host_common.hpp"
#include "zstd_dict_launch.hpp"

using namespace hcamd;

extern "C" {

hipcompStatus_t hipcompBatchedZstdDictGetPreparedSize(size_t dict_bytes, size_t* prepared_bytes)
{
  static const char* fn = "hipcompBatchedZstdDictGetPreparedSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, prepared_bytes);
  if (dict_bytes > zstd::kDictBytesMax)
    return fail(fn, "'dict_bytes' is larger than 2^30.");
  *prepared_bytes = zstd::prepared_bytes(dict_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictPrepareAsync(
    const void* const* device_dict_ptrs, const size_t* device_dict_bytes, size_t num_dicts,
    void* const* device_prepared_ptrs, const size_t* device_prepared_capacities, hipcompStatus_t* device_statuses,
    hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdDictPrepareAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_dict_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_dict_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_capacities);
  HCAMD_REQUIRE_NOT_NULL(fn, device_statuses);
  if (num_dicts == 0)
    return hipcompSuccess;
  zstd_dict_launch_prepare(
      reinterpret_cast<const uint8_t* const*>(device_dict_ptrs), device_dict_bytes, num_dicts,
      reinterpret_cast<uint8_t* const*>(device_prepared_ptrs), device_prepared_capacities, device_statuses, stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard dictionary prepare HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictDecompressGetTempSize(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedZstdDictDecompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  *temp_bytes = zstd::temp_bytes(num_chunks, max_uncompressed_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    const void* const* device_prepared_dicts, size_t* device_uncompressed_bytes, size_t batch_size, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdDictGetDecompressSizeAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_dicts);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  if (batch_size == 0)
    return hipcompSuccess;
  zstd_dict_launch_get_sizes(
      reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
      reinterpret_cast<const uint8_t* const*>(device_prepared_dicts), device_uncompressed_bytes, batch_size, stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard dictionary size HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictDecompressAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes, size_t* device_actual_uncompressed_bytes, size_t batch_size,
    void* device_temp_ptr, size_t temp_bytes, void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses, const void* const* device_prepared_dicts, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdDictDecompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_dicts);
  if (batch_size == 0)
    return hipcompSuccess;
  HCAMD_REQUIRE_NOT_NULL(fn, device_temp_ptr);
  // the temp space is shared out among the launch's waves as in zstd_batch.cpp
  if (temp_bytes < zstd::temp_bytes(batch_size, 1))
    return fail(fn, "'temp_bytes' is smaller than hipcompBatchedZstdDictDecompressGetTempSize() asks for.");
  size_t per_wave = temp_bytes / zstd::waves_for(batch_size) / 256u * 256u;
  if (per_wave > zstd::kBlockMax)
    per_wave = zstd::kBlockMax;
  zstd_dict_launch_decompress(
      reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
      device_uncompressed_bytes, batch_size, per_wave, device_temp_ptr,
      reinterpret_cast<uint8_t* const*>(device_uncompressed_ptrs), device_actual_uncompressed_bytes, device_statuses,
      reinterpret_cast<const uint8_t* const*>(device_prepared_dicts), stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard dictionary decompression HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

} // extern "C"
