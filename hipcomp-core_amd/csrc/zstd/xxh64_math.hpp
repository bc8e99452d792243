// xxh64_math.hpp -- XXH64 (the checksum of a Zstandard frame is its low 32 bits, seed 0), free of HIP.
//
// Plain constexpr C++17: the kernel (zstd_kernels.hip) and the CPU driver (tests/zstd_tables_driver.cpp) include
// this one file.  The hash is serial in 32-byte stripes with four accumulators; the kernel keeps one accumulator
// in each of four lanes and uses xxh64_round / xxh64_converge / xxh64_finish, xxh64() is the same in a loop.
#pragma once

#include <cstdint>

namespace hcamd {
namespace zstd {

constexpr uint64_t kXxhP1 = 0x9E3779B185EBCA87ull, kXxhP2 = 0xC2B2AE3D27D4EB4Full, kXxhP3 = 0x165667B19E3779F9ull,
                   kXxhP4 = 0x85EBCA77C2B2AE63ull, kXxhP5 = 0x27D4EB2F165667C5ull;

constexpr uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

template <class P>
constexpr uint64_t read_le(P p, uint64_t at, uint32_t nbytes)
{
  uint64_t v = 0;
  for (uint32_t b = 0; b < nbytes; ++b)
    v |= (uint64_t)(uint8_t)p[at + b] << (8u * b);
  return v;
}

// accumulator j (0..3) before the first stripe
constexpr uint64_t xxh64_acc_init(uint32_t j, uint64_t seed)
{
  return j == 0 ? seed + kXxhP1 + kXxhP2 : j == 1 ? seed + kXxhP2 : j == 2 ? seed : seed - kXxhP1;
}
constexpr uint64_t xxh64_round(uint64_t acc, uint64_t input) { return rotl64(acc + input * kXxhP2, 31) * kXxhP1; }
constexpr uint64_t xxh64_merge(uint64_t h, uint64_t acc) { return (h ^ xxh64_round(0, acc)) * kXxhP1 + kXxhP4; }
constexpr uint64_t xxh64_converge(uint64_t v1, uint64_t v2, uint64_t v3, uint64_t v4)
{
  uint64_t h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
  h = xxh64_merge(h, v1);
  h = xxh64_merge(h, v2);
  h = xxh64_merge(h, v3);
  return xxh64_merge(h, v4);
}
// h: the converged accumulators (n >= 32) or seed + P5 (n < 32); the tail is p[at, at + (n & 31))
template <class P>
constexpr uint64_t xxh64_finish(uint64_t h, P p, uint64_t at, uint64_t n)
{
  h += n;
  uint32_t left = (uint32_t)(n & 31u);
  for (; left >= 8; left -= 8, at += 8)
    h = rotl64(h ^ xxh64_round(0, read_le(p, at, 8)), 27) * kXxhP1 + kXxhP4;
  if (left >= 4) {
    h = rotl64(h ^ (read_le(p, at, 4) * kXxhP1), 23) * kXxhP2 + kXxhP3;
    at += 4;
    left -= 4;
  }
  for (; left > 0; --left, ++at)
    h = rotl64(h ^ ((uint64_t)(uint8_t)p[at] * kXxhP5), 11) * kXxhP1;
  h ^= h >> 33;
  h *= kXxhP2;
  h ^= h >> 29;
  h *= kXxhP3;
  h ^= h >> 32;
  return h;
}

template <class P>
constexpr uint64_t xxh64(P p, uint64_t n, uint64_t seed)
{
  if (n < 32)
    return xxh64_finish(seed + kXxhP5, p, 0, n);
  uint64_t v[4] = {xxh64_acc_init(0, seed), xxh64_acc_init(1, seed), xxh64_acc_init(2, seed), xxh64_acc_init(3, seed)};
  const uint64_t stripes = n >> 5;
  for (uint64_t s = 0; s < stripes; ++s)
    for (uint32_t j = 0; j < 4; ++j)
      v[j] = xxh64_round(v[j], read_le(p, 32u * s + 8u * j, 8));
  return xxh64_finish(xxh64_converge(v[0], v[1], v[2], v[3]), p, stripes << 5, n);
}

} // namespace zstd
} // namespace hcamd
