// zstd_dict_compress_batch.cpp -- C ABI of the batched Zstandard encoder with dictionaries
// (include/hipcomp/zstd_dict_compress.h).
//
// The sibling of ../zstd_compress/zstd_compress_batch.cpp in a library of its own,
// lib/libhipcomp_zstd_dict_compress.so: the same argument order, null checks and status codes, the same temp space
// (zstd_compress_sizing.hpp), one more array per compress call, the chunks' prepared dictionaries, and the prepare
// calls in the shape of ../zstd_dict/zstd_dict_batch.cpp.
#include "hipcomp/zstd_dict_compress.h"

#include "host_common.hpp"
#include "zstd_dict_compress_launch.hpp"

using namespace hcamd;

namespace {

// (the check that both Zstandard encoders make, zstd_compress_sizing.hpp, with this library's limit)
bool opts_ok(const char* fn, hipcompBatchedZstdOpts_t opts, size_t max_chunk_bytes, hipcompStatus_t& st)
{
  const std::string bad = zstd::enc_opts_error(opts.level, opts.checksum, max_chunk_bytes, HIPCOMP_ZSTD_DICT_COMPRESS_MAX_CHUNK_BYTES);
  if (!bad.empty())
    st = fail(fn, bad);
  return bad.empty();
}

static_assert(HIPCOMP_ZSTD_DICT_COMPRESS_MAX_CHUNK_BYTES == zstd::kDictEncMaxChunk, "the header's limit");
static_assert(HIPCOMP_ZSTD_DICT_COMPRESS_PREPARED_BASE_BYTES == zstd::kEncBlobTail, "the header's constant");

} // namespace

extern "C" {

hipcompStatus_t hipcompBatchedZstdDictCompressGetPreparedSize(size_t dict_bytes, size_t* prepared_bytes)
{
  static const char* fn = "hipcompBatchedZstdDictCompressGetPreparedSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, prepared_bytes);
  if (dict_bytes > zstd::kDictBytesMax)
    return fail(fn, "'dict_bytes' is larger than 2^30.");
  *prepared_bytes = zstd::enc_prepared_bytes(dict_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictCompressPrepareAsync(
    const void* const* device_dict_ptrs, const size_t* device_dict_bytes, size_t num_dicts,
    void* const* device_prepared_ptrs, const size_t* device_prepared_capacities, hipcompStatus_t* device_statuses,
    hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdDictCompressPrepareAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_dict_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_dict_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_capacities);
  HCAMD_REQUIRE_NOT_NULL(fn, device_statuses);
  if (num_dicts == 0)
    return hipcompSuccess;
  zstd_dict_compress_launch_prepare(
      reinterpret_cast<const uint8_t* const*>(device_dict_ptrs), device_dict_bytes, num_dicts,
      reinterpret_cast<uint8_t* const*>(device_prepared_ptrs), device_prepared_capacities, device_statuses, stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard dictionary compression prepare HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictCompressGetTempSize(
    size_t batch_size, size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedZstdDictCompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  *temp_bytes = zstd::enc_temp_bytes(batch_size, max_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes, hipcompBatchedZstdOpts_t format_opts, size_t* max_compressed_bytes)
{
  static const char* fn = "hipcompBatchedZstdDictCompressGetMaxOutputChunkSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, max_compressed_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  *max_compressed_bytes = zstd::dict_frame_bound((uint32_t)max_chunk_bytes);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedZstdDictCompressAsync(
    const void* const* device_uncompressed_ptrs, const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes, size_t batch_size, void* device_temp_ptr, size_t temp_bytes,
    void* const* device_compressed_ptrs, size_t* device_compressed_bytes, const void* const* device_prepared_dicts,
    hipcompBatchedZstdOpts_t format_opts, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedZstdDictCompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_prepared_dicts);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_uncompressed_chunk_bytes, st))
    return st;
  if (batch_size == 0)
    return hipcompSuccess;
  HCAMD_REQUIRE_NOT_NULL(fn, device_temp_ptr);
  if (temp_bytes < zstd::enc_temp_bytes(batch_size, max_uncompressed_chunk_bytes))
    return fail(fn, "'temp_bytes' is smaller than hipcompBatchedZstdDictCompressGetTempSize() asks for.");
  if ((reinterpret_cast<uintptr_t>(device_temp_ptr) & 3u) != 0)
    return fail(fn, "'device_temp_ptr' must be aligned to 4 bytes.");
  zstd_dict_compress_launch(
      reinterpret_cast<const uint8_t* const*>(device_uncompressed_ptrs), device_uncompressed_bytes,
      max_uncompressed_chunk_bytes, batch_size, device_temp_ptr, reinterpret_cast<uint8_t* const*>(device_compressed_ptrs),
      device_compressed_bytes, reinterpret_cast<const uint8_t* const*>(device_prepared_dicts), format_opts.checksum != 0, stream);
  std::string why;
  if (!launch_ok("Failed to launch Zstandard dictionary compression HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

} // extern "C"
