// crc32c_math.hpp -- CRC-32C (Castagnoli: reflected polynomial 0x82F63B78, initial value and final XOR 0xFFFFFFFF;
// RFC 3720 appendix B.4 has test vectors), the checksum of the Snappy framing format (snappy_frame.hpp), and the
// algebra that joins the CRCs of pieces.  The construction is crc32_math.hpp's, which explains it, over the other
// polynomial:
//     crc(A || B) = crc32c_shift(crc(A), |B|) ^ crc(B),   crc32c_shift(c, n) = c * x^(8n) mod P
//
// Standard headers and constexpr only: hipcc compiles these as host+device code (snappy_frame_kernels.hip), and
// tests/test_snappy_frame_cpu.py compiles this header with g++ alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace crc32c {

constexpr uint32_t kPoly = 0x82F63B78u;

// Slice-by-16 tables: t[0] is the byte table; t[k][b] is the CRC register after byte b followed by k zero bytes
constexpr int kSlices = 16;
struct alignas(16) Tables
{
  uint32_t t[kSlices][256];
};

constexpr Tables make_tables()
{
  Tables s{};
  for (uint32_t b = 0; b < 256; ++b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k)
      c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
    s.t[0][b] = c;
  }
  for (int k = 1; k < kSlices; ++k)
    for (uint32_t b = 0; b < 256; ++b)
      s.t[k][b] = (s.t[k - 1][b] >> 8) ^ s.t[0][s.t[k - 1][b] & 0xFFu];
  return s;
}

// a * b mod P: the same 32 steps for every input
constexpr uint32_t multmodp(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (int k = 31; k >= 0; --k) {
    p ^= b & (0u - ((a >> k) & 1u));
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

// x2n[k] = x^(8 * 2^k) mod P: shifting by 2^k bytes.  A data chunk of the format holds at most 2^16 bytes.
constexpr int kShiftBits = 17;
struct ShiftTable
{
  uint32_t x2n[kShiftBits];
};

constexpr ShiftTable make_shift_table()
{
  ShiftTable s{};
  uint32_t p = 1u << 30; // x^1
  for (int k = 0; k < 3; ++k)
    p = multmodp(p, p); // x^8
  for (int k = 0; k < kShiftBits; ++k) {
    s.x2n[k] = p;
    p = multmodp(p, p);
  }
  return s;
}

// crc * x^(8 * nbytes) mod P, nbytes < 2^kShiftBits: the CRC of a piece moved nbytes to the front
constexpr uint32_t crc32c_shift(const uint32_t (&x2n)[kShiftBits], uint32_t crc, uint32_t nbytes)
{
  for (int k = 0; nbytes; ++k, nbytes >>= 1)
    if (nbytes & 1u)
      crc = multmodp(x2n[k], crc);
  return crc;
}

// The CRC register (not conditioned) after the bytes p[0, n), one at a time
constexpr uint32_t crc32c_update_bytes(const uint32_t (&t0)[256], uint32_t reg, const uint8_t* p, size_t n)
{
  for (size_t i = 0; i < n; ++i)
    reg = (reg >> 8) ^ t0[(reg ^ p[i]) & 0xFFu];
  return reg;
}

// The register after 16 more bytes, given as four little-endian words (slice-by-16)
constexpr uint32_t crc32c_update_16(const Tables& s, uint32_t reg, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
  w0 ^= reg;
  return s.t[15][w0 & 0xFFu] ^ s.t[14][(w0 >> 8) & 0xFFu] ^ s.t[13][(w0 >> 16) & 0xFFu] ^ s.t[12][w0 >> 24]
         ^ s.t[11][w1 & 0xFFu] ^ s.t[10][(w1 >> 8) & 0xFFu] ^ s.t[9][(w1 >> 16) & 0xFFu] ^ s.t[8][w1 >> 24]
         ^ s.t[7][w2 & 0xFFu] ^ s.t[6][(w2 >> 8) & 0xFFu] ^ s.t[5][(w2 >> 16) & 0xFFu] ^ s.t[4][w2 >> 24]
         ^ s.t[3][w3 & 0xFFu] ^ s.t[2][(w3 >> 8) & 0xFFu] ^ s.t[1][(w3 >> 16) & 0xFFu] ^ s.t[0][w3 >> 24];
}

// CRC-32C of p[0, n), the plain form
constexpr uint32_t crc32c_of(const Tables& s, const uint8_t* p, size_t n)
{
  return ~crc32c_update_bytes(s.t[0], 0xFFFFFFFFu, p, n);
}

} // namespace crc32c
} // namespace hcamd
