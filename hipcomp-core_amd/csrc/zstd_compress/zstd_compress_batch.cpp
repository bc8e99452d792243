// zstd_compress_batch.cpp -- C ABI of the batched Zstandard encoder (include/hipcomp/zstd_compress.h).
//
// The entry points follow the compress calls of the other codecs in argument order, null checks and status
// codes (deflate_compress_batch.cpp), and ship in a library of their own, lib/libhipcomp_zstd_compress.so.
#include "hipcomp/zstd_compress.h"

#include "host_common.hpp"
#include "zstd_compress_launch.hpp"

using namespace hcamd;

namespace {

// (the check that both Zstandard encoders make, zstd_compress_sizing.hpp, with this library's limit)
bool opts_ok(const char* fn, hipcompBatchedZstdOpts_t opts, size_t max_chunk_bytes, hipcompStatus_t& st)
{
  const std::string bad = zstd::enc_opts_error(opts.level, opts.checksum, max_chunk_bytes, HIPCOMP_ZSTD_COMPRESS_MAX_CHUNK_BYTES);
  if (!bad.empty())
    st = fail(fn, bad);
  return bad.empty();
}

} // namespace

extern "C" {

hipcompStatus_t hipcompBatchedZstdCompressGetTempSize(
    size_t batch_size, size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedZstdCompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  *temp_bytes = zstd::enc_temp_bytes(batch_size, max_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* max_compressed_bytes)
{
  static const char* fn = "hipcompBatchedZstdCompressGetMaxOutputChunkSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, max_compressed_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  *max_compressed_bytes = zstd::frame_bound((uint32_t)max_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdCompressAsync(
    const void* const* device_uncompressed_ptrs, const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes, size_t batch_size, void* device_temp_ptr, size_t temp_bytes,
    void* const* device_compressed_ptrs, size_t* device_compressed_bytes, hipcompBatchedZstdOpts_t format_opts,
    hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdCompressAsync()";
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
  if (temp_bytes < zstd::enc_temp_bytes(batch_size, max_uncompressed_chunk_bytes))
    return fail(fn, "'temp_bytes' is smaller than hipcompBatchedZstdCompressGetTempSize() asks for.");
  if ((reinterpret_cast<uintptr_t>(device_temp_ptr) & 3u) != 0)
    return fail(fn, "'device_temp_ptr' must be aligned to 4 bytes.");
  zstd_launch_compress(
      reinterpret_cast<const uint8_t* const*>(device_uncompressed_ptrs), device_uncompressed_bytes,
      max_uncompressed_chunk_bytes, batch_size, device_temp_ptr,
      reinterpret_cast<uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes, format_opts.checksum != 0, stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard compression HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

} // extern "C"
