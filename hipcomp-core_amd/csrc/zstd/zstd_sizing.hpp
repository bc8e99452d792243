// zstd_sizing.hpp -- the temp-space formula of the Zstandard decoder, free of HIP: the C ABI's size query and
// the launch (zstd_launch.hpp) use this one function, tests/zstd_tables_driver.cpp prints it for the CPU tests.
#pragma once

#include <cstdint>

#include "device_facts.hpp"
#include "zstd_tables.hpp"

namespace hcamd {
namespace zstd {

constexpr uint32_t kWavesPerBlock = 4;
// the LDS of one wave (zstd_kernels.hip asserts that its struct fits)
constexpr uint32_t kLdsPerWave = 12u * 1024u;
// waves a launch can have: what 256 CUs hold at once by the kernel's LDS (device_facts.hpp); a larger batch is
// walked grid-stride, on a smaller device the rest of the grid waits its turn
constexpr uint64_t kMaxWaves = 256ull * groups_by_lds(kWavesPerBlock * kLdsPerWave) * kWavesPerBlock;

constexpr uint64_t waves_for(uint64_t num_chunks, uint64_t max_waves = kMaxWaves)
{
  return num_chunks < max_waves ? num_chunks : max_waves;
}

// Every resident wave owns one literal buffer: min(128 KiB, the largest chunk) bytes rounded up to 256.  The
// sequences are staged in registers and LDS and take no temp space.
constexpr uint64_t temp_bytes(uint64_t num_chunks, uint64_t max_uncompressed_chunk_bytes, uint64_t max_waves = kMaxWaves)
{
  return waves_for(num_chunks, max_waves) * literal_bytes_per_wave(max_uncompressed_chunk_bytes);
}

} // namespace zstd
} // namespace hcamd
