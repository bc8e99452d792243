// byte_window.hpp -- 64 bytes of an item in registers, for a parser whose state is wave-uniform (the Parquet kernels:
// parquet_hybrid_kernels.hip, parquet_delta_kernels.hip).  One coalesced load, lane l keeping byte
// l; every byte the parser asks for is read from the window's lane with a uniform index (v_readlane), and the window is
// loaded anew where the parser leaves it.  No byte outside the item is read.  It is the `Src` of the plan headers.
#pragma once

#include "wave_utils.hpp"

namespace hcamd {

// The register window.  `at` is asked with a wave-uniform position inside the item.
struct WindowSrc
{
  cgptr p;
  uint64_t n;
  int lane;
  uint32_t mine = 0;                 // this lane's byte
  uint64_t base = uint64_t(1) << 63; // (no position is within 64 of it: the first byte loads the window)
  __device__ __forceinline__ WindowSrc(cgptr p_, uint64_t n_, int lane_) : p(p_), n(n_), lane(lane_) {}
  __device__ __forceinline__ uint32_t at(uint64_t pos)
  {
    if (pos - base >= (uint64_t)kWave) {
      base = pos;
      const uint64_t a = pos + (uint64_t)lane;
      mine = a < n ? (uint32_t)p[a] : 0u;
    }
    return read_lane(mine, (int)uniform((uint32_t)(pos - base)));
  }
};

} // namespace hcamd
