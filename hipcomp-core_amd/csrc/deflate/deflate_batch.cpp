// deflate_batch.cpp -- C ABI of the batched Deflate decoder (include/hipcomp/deflate.h).
//
// A format of this library's own (the reference has no open Deflate): the entry points follow the decode
// calls of the other three codecs in argument order, null checks and status codes (snappy_batch.cpp), and
// ship in a library of their own, lib/libhipcomp_deflate.so.
#include "hipcomp/deflate.h"

#include "deflate_launch.hpp"
#include "host_common.hpp"

using namespace hcamd;

extern "C" {

hipcompStatus_t hipcompBatchedDeflateDecompressGetTempSize(
    size_t /*num_chunks*/, size_t /*max_uncompressed_chunk_bytes*/, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedDeflateDecompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  *temp_bytes = 0;
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedDeflateGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes, size_t batch_size, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedDeflateGetDecompressSizeAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  if (batch_size == 0)
    return hipcompSuccess;
  deflate_launch_get_sizes(
      reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
      device_uncompressed_bytes, batch_size, stream);
  std::string why;
  if (!launch_ok("Failed to launch Deflate size HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedDeflateDecompressAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes, size_t* device_actual_uncompressed_bytes, size_t batch_size,
    void* /*device_temp_ptr*/, size_t /*temp_bytes*/, void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedDeflateDecompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  if (batch_size == 0)
    return hipcompSuccess;
  deflate_launch_decompress(
      reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
      device_uncompressed_bytes, batch_size, reinterpret_cast<uint8_t* const*>(device_uncompressed_ptrs),
      device_actual_uncompressed_bytes, device_statuses, stream);
  std::string why;
  if (!launch_ok("Failed to launch Deflate decompression HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

} // extern "C"
