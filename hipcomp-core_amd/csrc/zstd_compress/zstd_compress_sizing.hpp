// zstd_compress_sizing.hpp -- the temp-space formula of the Zstandard encoder, free of HIP: the C ABI's size query
// and the launch (zstd_compress_launch.hpp) use these functions, tests/zstd_codes_driver.cpp prints them for the CPU
// tests.  Also the check of the options that the entry points of both Zstandard encoders make.
#pragma once

#include <cstdint>
#include <string>

#include "zstd_codes.hpp"

namespace hcamd {
namespace zstd {

// One wave per workgroup and at most this many of them: a larger batch is walked grid-stride.  It is what an MI355X
// holds at once -- 256 CUs x 12 workgroups by the kernel's LDS (zstd_compress_kernels.hip asserts its struct against
// kEncLdsPerWave) -- so no buffer belongs to a wave that only waits.
constexpr uint32_t kEncLdsPerWave = 13u * 1024u;
constexpr uint64_t kEncMaxWaves = 256ull * 12ull;
static_assert(12u * kEncLdsPerWave <= 160u * 1024u, "12 workgroups share a CU's 160 KiB of LDS");

constexpr uint64_t enc_waves_for(uint64_t num_chunks) { return num_chunks < kEncMaxWaves ? num_chunks : kEncMaxWaves; }

// a record per match of at least 4 bytes, stored 64 at a time
constexpr uint64_t enc_records_per_wave(uint64_t max_chunk_bytes) { return (max_chunk_bytes / kEncMinMatch + 64u) / 64u * 64u; }
// the literals of a chunk, gathered
constexpr uint64_t enc_literal_bytes_per_wave(uint64_t max_chunk_bytes) { return (max_chunk_bytes + 256u) / 256u * 256u; }

// Every wave in flight owns two arrays of 32-bit records (literal run | offset << 16; match length) and one
// literal buffer.
constexpr uint64_t enc_temp_bytes_per_wave(uint64_t max_chunk_bytes)
{
  return 8u * enc_records_per_wave(max_chunk_bytes) + enc_literal_bytes_per_wave(max_chunk_bytes);
}
constexpr uint64_t enc_temp_bytes(uint64_t num_chunks, uint64_t max_chunk_bytes)
{
  return enc_waves_for(num_chunks) * enc_temp_bytes_per_wave(max_chunk_bytes);
}

// What an entry point of zstd_compress_batch.cpp or ../zstd_dict_compress/zstd_dict_compress_batch.cpp refuses in its
// format_opts and chunk size, as the text for its stderr line; empty where it refuses nothing.  `limit` is the
// library's HIPCOMP_..._MAX_CHUNK_BYTES.
inline std::string enc_opts_error(int level, int checksum, uint64_t max_chunk_bytes, uint64_t limit)
{
  if (level != 0)
    return "'format_opts.level' must be 0.";
  if (checksum != 0 && checksum != 1)
    return "'format_opts.checksum' must be 0 or 1.";
  if (max_chunk_bytes > limit)
    return "the chunk size must not exceed " + std::to_string(limit) + " bytes.";
  return {};
}

} // namespace zstd
} // namespace hcamd
