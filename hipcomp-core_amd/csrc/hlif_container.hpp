// hlif_container.hpp -- the common header of a container of the high-level managers (hlif.hip writes and reads
// it; the ranged read's list kernel, range_kernels.hip, tests it too).
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace hlif {

// reference src/hipcomp_common_deps/hlif_shared_types.hpp:58-84 (layout by the C++ ABI: 64 bytes)
enum FormatType : uint8_t { kLZ4 = 0, kSnappy = 1, kANS = 2, kGDeflate = 3, kCascaded = 4, kBitcomp = 5 };
struct CommonHeader
{
  uint32_t magic_number;
  uint8_t major_version;
  uint8_t minor_version;
  uint8_t format;
  uint64_t comp_data_size;
  uint64_t decomp_data_size;
  uint64_t num_chunks;
  bool include_chunk_starts;
  uint32_t full_comp_buffer_checksum;
  uint32_t decomp_buffer_checksum;
  bool include_per_chunk_comp_buffer_checksums;
  bool include_per_chunk_decomp_buffer_checksums;
  uint64_t uncomp_chunk_size;
  uint32_t comp_data_offset;
};
static_assert(sizeof(CommonHeader) == 64, "container header layout");
static_assert(offsetof(CommonHeader, comp_data_size) == 8 && offsetof(CommonHeader, num_chunks) == 24
                  && offsetof(CommonHeader, full_comp_buffer_checksum) == 36
                  && offsetof(CommonHeader, uncomp_chunk_size) == 48 && offsetof(CommonHeader, comp_data_offset) == 56,
              "container header layout");

} // namespace hlif
} // namespace hcamd
