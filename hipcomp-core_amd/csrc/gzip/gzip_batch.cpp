// gzip_batch.cpp -- C ABI of the gzip / zlib / BGZF entry points (include/hipcomp/gzip.h).
//
// The entry points follow hipcomp/deflate.h and hipcomp/deflate_compress.h in argument order, null checks and
// status codes, and ship in a library of their own, lib/libhipcomp_gzip.so.  The Deflate work is done by the two
// Deflate libraries through their C ABI (this library links them, it compiles none of their sources):
//   decode:    gzip_parse_kernel -> hipcompBatchedDeflateDecompressAsync -> gzip_verify_kernel
//   size:      gzip_parse_kernel -> hipcompBatchedDeflateGetDecompressSizeAsync
//   compress:  gzip_list_kernel  -> hipcompBatchedDeflateCompressAsync   -> gzip_frame_kernel
// all on the caller's stream, so the order is the stream's.
#include "hipcomp/gzip.h"

#include "hipcomp/deflate.h"
#include "hipcomp/deflate_compress.h"

#include "gzip_frame.hpp"
#include "gzip_launch.hpp"
#include "host_common.hpp"

using namespace hcamd;

namespace {

constexpr size_t kTempAlign = 8;

bool opts_ok(const char* fn, hipcompBatchedGzipOpts_t opts, size_t max_chunk_bytes, hipcompStatus_t& st)
{
  if (!gzipframe::wrapper_known(opts.wrapper)) {
    st = fail(fn, "'format_opts.wrapper' must be a hipcompDeflateWrapper_t.");
    return false;
  }
  if (max_chunk_bytes > HIPCOMP_DEFLATE_COMPRESS_MAX_CHUNK_BYTES) {
    st = fail(fn, "the chunk size must not exceed 65536 bytes.");
    return false;
  }
  if (opts.wrapper == HIPCOMP_WRAPPER_BGZF && max_chunk_bytes > HIPCOMP_BGZF_MAX_CHUNK_BYTES) {
    st = fail(fn, "the chunk size of a BGZF block must not exceed 65280 bytes.");
    return false;
  }
  return true;
}

// the raw encoder's temp space, rounded up so that the pointer list behind it is aligned
bool raw_compress_temp(size_t batch_size, size_t max_chunk_bytes, size_t& bytes)
{
  size_t raw = 0;
  if (hipcompBatchedDeflateCompressGetTempSize(batch_size, max_chunk_bytes, hipcompBatchedDeflateDefaultOpts, &raw)
      != hipcompSuccess)
    return false;
  bytes = round_up_to(raw, kTempAlign);
  return true;
}

bool temp_ok(const char* fn, const void* temp, size_t temp_bytes, size_t need, hipcompStatus_t& st)
{
  if (temp == nullptr) {
    st = fail(fn, "'device_temp_ptr' must not be null.");
    return false;
  }
  if (temp_bytes < need) {
    st = fail(fn, "'temp_bytes' is smaller than the temp size query asks for.");
    return false;
  }
  if ((reinterpret_cast<uintptr_t>(temp) & (kTempAlign - 1)) != 0) {
    st = fail(fn, "'device_temp_ptr' must be aligned to 8 bytes.");
    return false;
  }
  return true;
}

} // namespace

extern "C" {

hipcompStatus_t hipcompBatchedGzipDecompressGetTempSize(
    size_t num_chunks, size_t /*max_uncompressed_chunk_bytes*/, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedGzipDecompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  *temp_bytes = num_chunks * kGzipDecodeTempPerMember;
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedGzipGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes, size_t batch_size, hipcompDeflateWrapper_t wrapper, void* device_temp_ptr,
    size_t temp_bytes, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedGzipGetDecompressSizeAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  if (!gzipframe::wrapper_known((int)wrapper))
    return fail(fn, "'wrapper' must be a hipcompDeflateWrapper_t.");
  if (batch_size == 0)
    return hipcompSuccess;
  hipcompStatus_t st = hipcompSuccess;
  if (!temp_ok(fn, device_temp_ptr, temp_bytes, batch_size * kGzipDecodeTempPerMember, st))
    return st;
  const GzipDecodeTemp t = gzip_decode_temp(device_temp_ptr, batch_size);
  gzip_launch_parse(reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
                    batch_size, (int)wrapper, t, stream);
  std::string why;
  if (!launch_ok("Failed to launch gzip header HIP kernel", why))
    return fail(fn, why);
  return hipcompBatchedDeflateGetDecompressSizeAsync(
      reinterpret_cast<const void* const*>(t.payload_ptrs), t.payload_bytes, device_uncompressed_bytes, batch_size,
      stream);
}

hipcompStatus_t hipcompBatchedGzipDecompressAsync(
    const void* const* device_compressed_ptrs, const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes, size_t* device_actual_uncompressed_bytes, size_t batch_size,
    void* device_temp_ptr, size_t temp_bytes, void* const* device_uncompressed_ptrs,
    hipcompStatus_t* device_statuses, hipcompDeflateWrapper_t wrapper, hipStream_t stream)
{
  static const char* fn = "hipcompBatchedGzipDecompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  if (!gzipframe::wrapper_known((int)wrapper))
    return fail(fn, "'wrapper' must be a hipcompDeflateWrapper_t.");
  if (batch_size == 0)
    return hipcompSuccess;
  hipcompStatus_t st = hipcompSuccess;
  if (!temp_ok(fn, device_temp_ptr, temp_bytes, batch_size * kGzipDecodeTempPerMember, st))
    return st;
  const GzipDecodeTemp t = gzip_decode_temp(device_temp_ptr, batch_size);
  gzip_launch_parse(reinterpret_cast<const uint8_t* const*>(device_compressed_ptrs), device_compressed_bytes,
                    batch_size, (int)wrapper, t, stream);
  std::string why;
  if (!launch_ok("Failed to launch gzip header HIP kernel", why))
    return fail(fn, why);
  st = hipcompBatchedDeflateDecompressAsync(
      reinterpret_cast<const void* const*>(t.payload_ptrs), t.payload_bytes, device_uncompressed_bytes,
      t.raw_actual, batch_size, nullptr, 0, device_uncompressed_ptrs, t.raw_statuses, stream);
  if (st != hipcompSuccess)
    return st;
  gzip_launch_verify(reinterpret_cast<const uint8_t* const*>(device_uncompressed_ptrs), batch_size, (int)wrapper, t,
                     device_actual_uncompressed_bytes, device_statuses, stream);
  if (!launch_ok("Failed to launch gzip checksum HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedGzipCompressGetTempSize(
    size_t batch_size, size_t max_chunk_bytes, hipcompBatchedGzipOpts_t format_opts, size_t* temp_bytes)
{
  static const char* fn = "hipcompBatchedGzipCompressGetTempSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, temp_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  size_t raw = 0;
  if (!raw_compress_temp(batch_size, max_chunk_bytes, raw))
    return fail(fn, "the Deflate encoder's temp size query failed.", hipcompErrorInternal);
  *temp_bytes = raw + batch_size * sizeof(uint8_t*);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedGzipCompressGetMaxOutputChunkSize(
    size_t max_chunk_bytes, hipcompBatchedGzipOpts_t format_opts, size_t* max_member_bytes)
{
  static const char* fn = "hipcompBatchedGzipCompressGetMaxOutputChunkSize()";
  HCAMD_REQUIRE_NOT_NULL(fn, max_member_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_chunk_bytes, st))
    return st;
  size_t raw = 0;
  if (hipcompBatchedDeflateCompressGetMaxOutputChunkSize(max_chunk_bytes, hipcompBatchedDeflateDefaultOpts, &raw)
      != hipcompSuccess)
    return fail(fn, "the Deflate encoder's output bound query failed.", hipcompErrorInternal);
  *max_member_bytes = raw + gzipframe::header_bytes(format_opts.wrapper) + gzipframe::trailer_bytes(format_opts.wrapper);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBatchedGzipCompressAsync(
    const void* const* device_uncompressed_ptrs, const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes, size_t batch_size, void* device_temp_ptr, size_t temp_bytes,
    void* const* device_compressed_ptrs, size_t* device_compressed_bytes, hipcompBatchedGzipOpts_t format_opts,
    hipStream_t stream)
{
  static const char* fn = "hipcompBatchedGzipCompressAsync()";
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_uncompressed_bytes);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_ptrs);
  HCAMD_REQUIRE_NOT_NULL(fn, device_compressed_bytes);
  hipcompStatus_t st = hipcompSuccess;
  if (!opts_ok(fn, format_opts, max_uncompressed_chunk_bytes, st))
    return st;
  if (batch_size == 0)
    return hipcompSuccess;
  size_t raw = 0;
  if (!raw_compress_temp(batch_size, max_uncompressed_chunk_bytes, raw))
    return fail(fn, "the Deflate encoder's temp size query failed.", hipcompErrorInternal);
  if (!temp_ok(fn, device_temp_ptr, temp_bytes, raw + batch_size * sizeof(uint8_t*), st))
    return st;
  uint8_t** payload_ptrs = reinterpret_cast<uint8_t**>(static_cast<uint8_t*>(device_temp_ptr) + raw);
  const int wrapper = format_opts.wrapper;
  gzip_launch_list(reinterpret_cast<uint8_t* const*>(device_compressed_ptrs), batch_size, wrapper, payload_ptrs, stream);
  std::string why;
  if (!launch_ok("Failed to launch gzip pointer list HIP kernel", why))
    return fail(fn, why);
  st = hipcompBatchedDeflateCompressAsync(
      device_uncompressed_ptrs, device_uncompressed_bytes, max_uncompressed_chunk_bytes, batch_size, device_temp_ptr,
      raw, reinterpret_cast<void* const*>(payload_ptrs), device_compressed_bytes, hipcompBatchedDeflateDefaultOpts,
      stream);
  if (st != hipcompSuccess)
    return st;
  gzip_launch_frame(reinterpret_cast<const uint8_t* const*>(device_uncompressed_ptrs), device_uncompressed_bytes,
                    batch_size, wrapper, reinterpret_cast<uint8_t* const*>(device_compressed_ptrs),
                    device_compressed_bytes, stream);
  if (!launch_ok("Failed to launch gzip framing HIP kernel", why))
    return fail(fn, why);
  return hipcompSuccess;
}

hipcompStatus_t hipcompBgzfSplitHost(
    const void* host_bytes, size_t n, size_t* offsets, size_t capacity, size_t* count, size_t* stopped_at)
{
  static const char* fn = "hipcompBgzfSplitHost()";
  HCAMD_REQUIRE_NOT_NULL(fn, count);
  HCAMD_REQUIRE_NOT_NULL(fn, stopped_at);
  if (n != 0)
    HCAMD_REQUIRE_NOT_NULL(fn, host_bytes);
  if (capacity != 0)
    HCAMD_REQUIRE_NOT_NULL(fn, offsets);
  *stopped_at = gzipframe::bgzf_split(static_cast<const uint8_t*>(host_bytes), n, offsets, capacity, count);
  return hipcompSuccess;
}

} // extern "C"
