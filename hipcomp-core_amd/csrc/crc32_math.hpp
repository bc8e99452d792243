// crc32_math.hpp -- CRC-32 as IEEE 802.3 / zlib define it (reflected polynomial 0xEDB88320, initial value and
// final XOR 0xFFFFFFFF; zlib.crc32 gives the same numbers), and the algebra that joins the CRCs of pieces.
//
// Bit-reflected, a 32-bit word is a polynomial of degree < 32 with bit 31 the coefficient of x^0.  The CRC of
// a message M of n bytes is then linear up to its conditioning, and for two messages
//     crc(A || B) = crc32_shift(crc(A), |B|) ^ crc(B),   crc32_shift(c, n) = c * x^(8n) mod P
// (zlib's crc32_combine).  Unrolled over many parts: crc(P_0 || ... || P_k) = XOR_i crc32_shift(crc(P_i), bytes
// after P_i) -- a sum in any order, which the kernels (checksum_kernels.hip) build with atomicXor.  An empty
// part has CRC 0 and adds nothing.
//
// Standard headers and constexpr only: hipcc compiles these as host+device code, and tests/test_crc32_cpu.py
// compiles this header with g++ alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace crc32 {

constexpr uint32_t kPoly = 0xEDB88320u;

// Slice-by-16 tables: t[0] is the byte table; t[k][b] is the CRC register after byte b followed by k zero
// bytes, so that 16 bytes are folded in with 16 independent lookups (checksum_kernels.hip).
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

// a * b mod P (zlib's multmodp, without its early exit: the same 32 steps for every input)
constexpr uint32_t multmodp(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (int k = 31; k >= 0; --k) {
    p ^= b & (0u - ((a >> k) & 1u));
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

// x2n[k] = x^(8 * 2^k) mod P: shifting by 2^k bytes
constexpr int kShiftBits = 64;
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

// crc * x^(8 * nbytes) mod P: the CRC of a piece moved nbytes to the front (square and multiply over the bits
// of nbytes, one multmodp per set bit)
constexpr uint32_t crc32_shift(const uint32_t (&x2n)[kShiftBits], uint32_t crc, uint64_t nbytes)
{
  for (int k = 0; nbytes; ++k, nbytes >>= 1)
    if (nbytes & 1u)
      crc = multmodp(x2n[k], crc);
  return crc;
}

// The CRC register (not conditioned) after the bytes p[0, n), one at a time
constexpr uint32_t crc32_update_bytes(const uint32_t (&t0)[256], uint32_t reg, const uint8_t* p, size_t n)
{
  for (size_t i = 0; i < n; ++i)
    reg = (reg >> 8) ^ t0[(reg ^ p[i]) & 0xFFu];
  return reg;
}

// The register after 16 more bytes, given as four little-endian words (slice-by-16)
constexpr uint32_t crc32_update_16(const Tables& s, uint32_t reg, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
  w0 ^= reg;
  return s.t[15][w0 & 0xFFu] ^ s.t[14][(w0 >> 8) & 0xFFu] ^ s.t[13][(w0 >> 16) & 0xFFu] ^ s.t[12][w0 >> 24]
         ^ s.t[11][w1 & 0xFFu] ^ s.t[10][(w1 >> 8) & 0xFFu] ^ s.t[9][(w1 >> 16) & 0xFFu] ^ s.t[8][w1 >> 24]
         ^ s.t[7][w2 & 0xFFu] ^ s.t[6][(w2 >> 8) & 0xFFu] ^ s.t[5][(w2 >> 16) & 0xFFu] ^ s.t[4][w2 >> 24]
         ^ s.t[3][w3 & 0xFFu] ^ s.t[2][(w3 >> 8) & 0xFFu] ^ s.t[1][(w3 >> 16) & 0xFFu] ^ s.t[0][w3 >> 24];
}

// CRC-32 of p[0, n) (the host's plain form; zlib.crc32(p))
constexpr uint32_t crc32_of(const Tables& s, const uint8_t* p, size_t n)
{
  return ~crc32_update_bytes(s.t[0], 0xFFFFFFFFu, p, n);
}

} // namespace crc32
} // namespace hcamd
