// adler32_math.hpp -- Adler-32 as RFC 1950 / zlib define it (zlib.adler32 gives the same numbers), and the algebra
// that joins the sums of pieces.
//
// Over the bytes d_0 .. d_(n-1):  A = 1 + sum d_j,  B = n + sum (n - j) * d_j,  both mod 65521; the value is
// (B << 16) | A.  Cut into pieces, piece k of len_k bytes with `after_k` bytes behind it has
//     a_k = sum d_j,   b_k = sum (len_k - j) * d_j        (j from 0 inside the piece)
// and a byte of piece k counts (len_k - j) + after_k times in B, so
//     A = 1 + sum_k a_k,   B = n + sum_k (b_k + a_k * after_k)          (mod 65521)
// -- a sum in any order, which the kernels (gzip_kernels.hip) build one piece per lane.  An empty piece adds nothing.
//
// Where to reduce.  The running sums are 32-bit.  From a < 65521 and b < 65521, n more bytes of 255 leave
// b <= 65520 + n * 65520 + 255 * n * (n + 1) / 2, which stays below 2^32 up to n = 5552 (zlib's NMAX): both sums
// are reduced after 5552 bytes at the latest (347 blocks of 16).  a_k and after_k mod 65521 are below 65521, so
// their product is below 65520^2 < 2^32; after_k has no bound of its own (a decoded chunk has no size limit) and
// is reduced BEFORE it is multiplied.
//
// Standard headers and constexpr only: hipcc compiles these as host+device code, and tests/test_gzip_frame_cpu.py
// compiles this header with g++ alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace hcamd {
namespace adler32 {

constexpr uint32_t kMod = 65521u;
constexpr uint32_t kNmax = 5552u;               // bytes between two reductions, at most
constexpr uint32_t kBlocksPerReduce = kNmax / 16; // 347 blocks of 16 bytes are exactly 5552 bytes

static_assert(kBlocksPerReduce * 16 == kNmax, "347 * 16");
// the bound above, at n = 5552, in 64 bits
static_assert(65520ull + 5552ull * 65520ull + 255ull * 5552ull * 5553ull / 2 < (1ull << 32), "NMAX");
static_assert(65520ull * 65520ull < (1ull << 32), "a * (after mod 65521)");

// the sums of one piece, both below 65521
struct Piece
{
  uint32_t a, b;
};

// the running sums (a, b) after the bytes p[0, n); n <= kNmax, the caller reduces
constexpr void update_bytes(uint32_t& a, uint32_t& b, const uint8_t* p, size_t n)
{
  for (size_t i = 0; i < n; ++i) {
    a += p[i];
    b += a;
  }
}

// the running sums after 16 more bytes, given as four little-endian words:
// b grows by 16 * a (the bytes so far count 16 times more) and by sum (16 - j) * d_j
constexpr void update_16(uint32_t& a, uint32_t& b, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
  const uint32_t w[4] = {w0, w1, w2, w3};
  uint32_t s = 0, t = 0;
  for (int k = 0; k < 4; ++k) {
    const uint32_t d0 = w[k] & 0xFFu, d1 = (w[k] >> 8) & 0xFFu, d2 = (w[k] >> 16) & 0xFFu, d3 = w[k] >> 24;
    s += d0 + d1 + d2 + d3;
    t += (16u - 4u * k) * d0 + (15u - 4u * k) * d1 + (14u - 4u * k) * d2 + (13u - 4u * k) * d3;
  }
  b += 16u * a + t;
  a += s;
}

// the sums of the piece p[0, n), any n
constexpr Piece piece_of(const uint8_t* p, size_t n)
{
  uint32_t a = 0, b = 0;
  while (n) {
    const size_t step = n < kNmax ? n : kNmax;
    update_bytes(a, b, p, step);
    a %= kMod;
    b %= kMod;
    p += step;
    n -= step;
  }
  return Piece{a, b};
}

// what a piece with `after` bytes behind it adds to B (below 65521); to A it adds piece.a
constexpr uint32_t b_share(Piece piece, uint64_t after)
{
  return (piece.b + piece.a * (uint32_t)(after % kMod)) % kMod;
}

// the value from the sums over all pieces (each sum may be unreduced, below 2^32) and the total length
constexpr uint32_t finish(uint32_t sum_a, uint32_t sum_b_shares, uint64_t n)
{
  const uint32_t a = (1u + sum_a % kMod) % kMod;
  const uint32_t b = ((uint32_t)(n % kMod) + sum_b_shares % kMod) % kMod;
  return (b << 16) | a;
}

// Adler-32 of p[0, n) (the host's plain form; zlib.adler32(p))
constexpr uint32_t adler32_of(const uint8_t* p, size_t n)
{
  const Piece whole = piece_of(p, n);
  return finish(whole.a, b_share(whole, 0), n);
}

} // namespace adler32
} // namespace hcamd
