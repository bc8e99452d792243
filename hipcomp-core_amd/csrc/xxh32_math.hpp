// xxh32_math.hpp -- XXH32 as the xxHash specification defines it (the hash of the LZ4 frame format: header
// checksum, block checksums, content checksum).
//
// The hash of n bytes: four accumulators take the 16-byte stripes (accumulator k the dword at 4k of every stripe,
// each a chain of its own), they are merged once the stripes are through, the length is added, the up to 15 bytes
// that are left go in as dwords and then as single bytes, and the avalanche mixes the result.  The pieces are
// separate functions because the kernels (lz4_frame_kernels.hip) give the four accumulators to four lanes.
//
// Standard headers and constexpr only: hipcc compiles these as host+device code, the CPU test drivers and
// lz4_interop.cpp compile this header alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace xxh32 {

constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u, kP4 = 668265263u, kP5 = 374761393u;

constexpr uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
constexpr uint32_t read32(const uint8_t* p)
{
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// accumulator k (0..3) before the first stripe
constexpr uint32_t acc_init(int k, uint32_t seed)
{
  return k == 0 ? seed + kP1 + kP2 : k == 1 ? seed + kP2 : k == 2 ? seed : seed - kP1;
}
// one dword of a stripe into its accumulator
constexpr uint32_t round(uint32_t acc, uint32_t word) { return rotl(acc + word * kP2, 13) * kP1; }
// the four accumulators after the last stripe (len >= 16)
constexpr uint32_t merge(uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4)
{
  return rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
}
// what a hash of fewer than 16 bytes starts from in place of merge()
constexpr uint32_t short_init(uint32_t seed) { return seed + kP5; }
constexpr uint32_t tail_word(uint32_t h, uint32_t word) { return rotl(h + word * kP3, 17) * kP4; }
constexpr uint32_t tail_byte(uint32_t h, uint32_t byte) { return rotl(h + byte * kP5, 11) * kP1; }
constexpr uint32_t avalanche(uint32_t h)
{
  h ^= h >> 15;
  h *= kP2;
  h ^= h >> 13;
  h *= kP3;
  h ^= h >> 16;
  return h;
}

// h: merge(...) or short_init(seed); p: the len % 16 bytes behind the last stripe; len: of the whole input
constexpr uint32_t finish(uint32_t h, const uint8_t* p, uint64_t len)
{
  h += (uint32_t)len;
  uint32_t rest = (uint32_t)(len & 15u);
  for (; rest >= 4; rest -= 4, p += 4)
    h = tail_word(h, read32(p));
  for (; rest; --rest, ++p)
    h = tail_byte(h, *p);
  return avalanche(h);
}

constexpr uint32_t hash(const uint8_t* p, uint64_t len, uint32_t seed)
{
  uint32_t h = short_init(seed);
  if (len >= 16) {
    uint32_t v[4] = {acc_init(0, seed), acc_init(1, seed), acc_init(2, seed), acc_init(3, seed)};
    for (uint64_t s = 0; s < len / 16; ++s, p += 16)
      for (int k = 0; k < 4; ++k)
        v[k] = round(v[k], read32(p + 4 * k));
    h = merge(v[0], v[1], v[2], v[3]);
  }
  return finish(h, p, len);
}

} // namespace xxh32
} // namespace hcamd
