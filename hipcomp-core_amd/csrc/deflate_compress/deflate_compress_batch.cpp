// deflate_compress_batch.cpp -- C ABI of the batched Deflate encoder (include/hipcomp/deflate_compress.h).
//
// The entry points follow the compress calls of the other codecs in argument order, null checks and status
// codes (snappy_batch.cpp), and ship in a library of their own, lib/libhipcomp_deflate_compress.so.
#include "hipcomp/deflate_compress.h"

#include "deflate_codes.hpp"
#include "deflate_compress_launch.hpp"
#include "host_common.hpp"

using namespace hcamd;

namespace {

bool opts_ok(const char* fn, hipcompBatchedDeflateOpts_t opts, size_t max_chunk_bytes, hipcompStatus_t& st)
{
  if (opts.algo != 0) {
    st = fail(fn, "'format_opts.algo' must be 0.");
    return false;
  }
  if (max_chunk_bytes > HIPCOMP_DEFLATE_COMPRESS_MAX_CHUNK_BYTES) {
    st = fail(fn, "the chunk size must not exceed 65536 bytes.");
    return false;
  }
  return true;
}

size_t temp_size(size_t batch_size, size_t max_chunk_bytes)
{
  return deflate_compress_waves(batch_size) * deflate_compress_records_per_wave(max_chunk_bytes) * sizeof(uint32_t);
}

} // namespace

extern "C" {

hipcompStatus_t hipcompBatchedDeflateCompressGetTempSize(
    size_t batch_size, size_t max_chunk_bytes, hipcompBatchedDeflateOpts_t format_opts, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedDeflateCompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  *temp_bytes = temp_size(batch_size, max_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedDeflateCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes, hipcompBatchedDeflateOpts_t format_opts, size_t* max_compressed_bytes)
{
  static const char* fn = "hipcompBatchedDeflateCompressGetMaxOutputChunkSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, max_compressed_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  *max_compressed_bytes = deflate::stored_bytes((uint32_t)max_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedDeflateCompressAsync(
    const void* const* device_uncompressed_ptrs, const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes, size_t batch_size, void* device_temp_ptr, size_t temp_bytes,
    void* const* device_compressed_ptrs, size_t* device_compressed_bytes, hipcompBatchedDeflateOpts_t format_opts,
    hipStream_t stream)
{
  static const char* fn = "hipcompBatchedDeflateCompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_uncompressed_chunk_bytes, st))
    return st;
  if (batch_size == 0)
    return hipcompSuccess;
  HCAMD_REQUIRE_NOT_NULL(fn, device_temp_ptr);
  if (temp_bytes < temp_size(batch_size, max_uncompressed_chunk_bytes))
    return fail(fn, "'temp_bytes' is smaller than hipcompBatchedDeflateCompressGetTempSize() asks for.");
  if ((reinterpret_cast<uintptr_t>(device_temp_ptr) & 3u) != 0)
    return fail(fn, "'device_temp_ptr' must be aligned to 4 bytes.");
  deflate_launch_compress(
      reinterpret_cast<const uint8_t* const*>(device_uncompressed_ptrs), device_uncompressed_bytes,
      max_uncompressed_chunk_bytes, batch_size, device_temp_ptr,
      reinterpret_cast<uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes, stream);
  std::string why;
  if (!launch_ok("Failed to launch Deflate compression HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

} // extern "C"
