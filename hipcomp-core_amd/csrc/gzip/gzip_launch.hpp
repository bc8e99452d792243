// gzip_launch.hpp -- host-callable launchers of the framing kernels (gzip_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hipcomp/shared_types.h"

namespace hcamd {

// What the decode side keeps per member between its launches, as arrays of `batch` entries in the call's temp
// space (the 8-byte arrays first: temp is 8-byte aligned).
struct GzipDecodeTemp
{
  const uint8_t** payload_ptrs;   // the raw Deflate stream of member i ...
  size_t* payload_bytes;          // ... and its length: 0 for a refused header, which the raw decoder refuses
  size_t* raw_actual;             // the raw decoder's own results
  hipcompStatus_t* raw_statuses;
  uint32_t* checks;               // the trailer's CRC-32 / Adler-32
  uint32_t* isizes;               // the trailer's ISIZE (gzip)
  uint32_t* header_ok;
};

constexpr size_t kGzipDecodeTempPerMember = 3 * 8 + 4 * 4;

inline GzipDecodeTemp gzip_decode_temp(void* temp, size_t batch)
{
  GzipDecodeTemp t;
  uint8_t* at = static_cast<uint8_t*>(temp);
  t.payload_ptrs = reinterpret_cast<const uint8_t**>(at);
  t.payload_bytes = reinterpret_cast<size_t*>(at + 8 * batch);
  t.raw_actual = reinterpret_cast<size_t*>(at + 16 * batch);
  t.raw_statuses = reinterpret_cast<hipcompStatus_t*>(at + 24 * batch);
  t.checks = reinterpret_cast<uint32_t*>(at + 28 * batch);
  t.isizes = reinterpret_cast<uint32_t*>(at + 32 * batch);
  t.header_ok = reinterpret_cast<uint32_t*>(at + 36 * batch);
  return t;
}

// one thread per member: gzipframe::parse_member into t
void gzip_launch_parse(const uint8_t* const* comp_ptrs, const size_t* comp_bytes, size_t batch, int wrapper,
                       const GzipDecodeTemp& t, hipStream_t stream);

// one wave per member, after the raw decoder: the checksum of what was decoded against the trailer, and the
// caller's actual / statuses (each may be NULL)
void gzip_launch_verify(const uint8_t* const* out_ptrs, size_t batch, int wrapper, const GzipDecodeTemp& t,
                        size_t* actual, hipcompStatus_t* statuses, hipStream_t stream);

// payload_ptrs[i] = out_ptrs[i] + the wrapper's header length: where the raw encoder writes
void gzip_launch_list(uint8_t* const* out_ptrs, size_t batch, int wrapper, uint8_t** payload_ptrs, hipStream_t stream);

// one wave per chunk, after the raw encoder: header and trailer around the stream of out_bytes[i] bytes that
// starts header_bytes behind out_ptrs[i], and out_bytes[i] made the member's length; a chunk of size 0 stays 0
void gzip_launch_frame(const uint8_t* const* in_ptrs, const size_t* in_bytes, size_t batch, int wrapper,
                       uint8_t* const* out_ptrs, size_t* out_bytes, hipStream_t stream);

} // namespace hcamd
