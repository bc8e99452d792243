// gzip_frame.hpp -- the framing of a Deflate stream as a gzip member (RFC 1952), a zlib stream (RFC 1950) or a
// BGZF block (a gzip member with a 'BC' extra field that holds its own length): the header parser of the decode
// side, the header and trailer bytes of the encode side, the output bound and the host's BGZF splitter.
//
// Standard headers and constexpr only.  The kernels (gzip_kernels.hip) and tests/gzip_frame_driver.cpp include
// this very file, so that what the CPU test proves about parse_member -- it reads only p[0, n), and its payload
// span lies inside the member -- holds for the thread that runs it on the device.
#pragma once

#include <cstddef>
#include <cstdint>

#include "crc32_math.hpp"

namespace hcamd {
namespace gzipframe {

// the values of hipcompDeflateWrapper_t (include/hipcomp/gzip.h)
constexpr int kGzip = 0, kZlib = 1, kBgzf = 2;

constexpr bool wrapper_known(int w) { return w == kGzip || w == kZlib || w == kBgzf; }

constexpr uint32_t header_bytes(int w) { return w == kZlib ? 2u : w == kBgzf ? 18u : 10u; }
constexpr uint32_t trailer_bytes(int w) { return w == kZlib ? 4u : 8u; }

// the smallest members parse_member looks at: a gzip header, no payload and the trailer; the zlib header and trailer
constexpr size_t kGzipMinBytes = 18, kZlibMinBytes = 6;

struct Member
{
  bool ok;              // the header is one this library takes
  size_t payload_at;    // the raw Deflate stream is p[payload_at, payload_at + payload_bytes)
  size_t payload_bytes;
  uint32_t check;       // the trailer's CRC-32 (gzip) or Adler-32 (zlib)
  uint32_t isize;       // gzip: the trailer's ISIZE; zlib: 0
};

constexpr Member refused() { return Member{false, 0, 0, 0, 0}; }

constexpr uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
constexpr uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }
constexpr uint32_t be32(const uint8_t* p)
{
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// CRC-32 of p[0, n) bit by bit, without a table: FHCRC covers a header of a few bytes
constexpr uint32_t crc32_bitwise(const uint8_t* p, size_t n)
{
  uint32_t reg = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    reg ^= p[i];
    for (int k = 0; k < 8; ++k)
      reg = (reg >> 1) ^ (crc32::kPoly & (0u - (reg & 1u)));
  }
  return ~reg;
}

// the end of the NUL-terminated field that starts at `at`, or 0 if no NUL lies in front of `limit`
constexpr size_t skip_string(const uint8_t* p, size_t at, size_t limit)
{
  for (; at < limit; ++at)
    if (p[at] == 0)
      return at + 1;
  return 0;
}

constexpr Member parse_gzip(const uint8_t* p, size_t n)
{
  if (n < kGzipMinBytes)
    return refused();
  const size_t limit = n - 8;   // where the trailer starts: no header field may pass it
  if (p[0] != 0x1F || p[1] != 0x8B || p[2] != 8)
    return refused();
  const uint32_t flg = p[3];
  if (flg & 0xE0u)
    return refused();
  size_t at = 10;               // MTIME (4), XFL and OS are not looked at
  if (flg & 4u) {               // FEXTRA
    if (at + 2 > limit)
      return refused();
    const size_t xlen = le16(p + at);
    at += 2;
    if (xlen > limit - at)
      return refused();
    at += xlen;
  }
  if (flg & 8u) {               // FNAME
    at = skip_string(p, at, limit);
    if (at == 0)
      return refused();
  }
  if (flg & 16u) {              // FCOMMENT
    at = skip_string(p, at, limit);
    if (at == 0)
      return refused();
  }
  if (flg & 2u) {               // FHCRC: the low 16 bits of the CRC-32 of the header in front of it
    if (at + 2 > limit)
      return refused();
    if (le16(p + at) != (crc32_bitwise(p, at) & 0xFFFFu))
      return refused();
    at += 2;
  }
  return Member{true, at, limit - at, le32(p + limit), le32(p + limit + 4)};
}

constexpr Member parse_zlib(const uint8_t* p, size_t n)
{
  if (n < kZlibMinBytes)
    return refused();
  const uint32_t cmf = p[0], flg = p[1];
  if ((cmf & 0x0Fu) != 8 || (cmf >> 4) > 7)   // CM = 8, a window of at most 32 KiB
    return refused();
  if ((cmf * 256u + flg) % 31u != 0)          // FCHECK
    return refused();
  if (flg & 0x20u)                            // FDICT: a preset dictionary is not taken
    return refused();
  return Member{true, 2, n - 6, be32(p + n - 4), 0};
}

// One member in p[0, n): kBgzf is parsed as the gzip member it is.  Reads only p[0, n).
constexpr Member parse_member(const uint8_t* p, size_t n, int wrapper)
{
  return wrapper == kZlib ? parse_zlib(p, n) : parse_gzip(p, n);
}

// ---------------------------------------------------------------------------------------------------- encode side

// Byte k of the header the encoder writes, k < header_bytes(w).  member_bytes is the whole member's length
// (only BGZF stores it: BSIZE = member_bytes - 1, in the last two header bytes).
//   gzip  1f 8b 08 00 00000000 00 ff                      no flags, no MTIME, XFL 0, OS unknown
//   zlib  78 01                                            a 32 KiB window, the fastest level, FCHECK
//   BGZF  1f 8b 08 04 00000000 00 ff 06 00 42 43 02 00 <BSIZE>
constexpr uint8_t header_byte(int w, uint32_t k, uint32_t member_bytes)
{
  if (w == kZlib)
    return k == 0 ? 0x78 : 0x01;
  const uint8_t gz[16] = {0x1F, 0x8B, 0x08, 0x00, 0, 0, 0, 0, 0x00, 0xFF, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00};
  if (w == kBgzf) {
    if (k == 3)
      return 0x04;
    if (k >= 16)
      return (uint8_t)((member_bytes - 1u) >> (8u * (k - 16u)));
  }
  return gz[k & 15u];
}

// Byte k of the trailer, k < trailer_bytes(w): gzip and BGZF CRC-32 then ISIZE, little endian; zlib Adler-32, big endian
constexpr uint8_t trailer_byte(int w, uint32_t k, uint32_t check, uint32_t isize)
{
  if (w == kZlib)
    return (uint8_t)(check >> (24u - 8u * k));
  return (uint8_t)((k < 4 ? check : isize) >> (8u * (k & 3u)));
}

// the raw encoder's bound (include/hipcomp/deflate_compress.h): the chunk as stored blocks
constexpr size_t raw_bound(size_t n)
{
  const size_t blocks = (n + 65534) / 65535;
  return n + 5 * (blocks ? blocks : 1);
}

constexpr size_t max_member_bytes(size_t n, int w)
{
  return raw_bound(n) + header_bytes(w) + trailer_bytes(w);
}

// the empty BGZF block that ends a file (the SAM specification's end-of-file marker)
constexpr uint8_t kBgzfEof[28] = {0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xFF, 0x06, 0x00, 0x42, 0x43,
                                  0x02, 0x00, 0x1B, 0x00, 0x03, 0x00, 0, 0, 0, 0, 0, 0, 0, 0};

// ------------------------------------------------------------------------------------------------ BGZF splitter

// The length of the BGZF block at p[at, n), from the BSIZE of its 'BC' extra subfield, or 0 where there is no
// whole BGZF block: the fixed header does not fit, it is no gzip member with FEXTRA, the extra field holds no
// 'BC' subfield of 2 bytes, or the block would pass n or be shorter than its own header and trailer.
constexpr size_t bgzf_block_bytes(const uint8_t* p, size_t at, size_t n)
{
  if (n - at < 12)
    return 0;
  const uint8_t* h = p + at;
  if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || !(h[3] & 4u))
    return 0;
  const size_t xlen = le16(h + 10);
  if (xlen > n - at - 12)
    return 0;
  size_t f = 12;
  const size_t fend = 12 + xlen;
  while (f + 4 <= fend) {
    const size_t slen = le16(h + f + 2);
    if (slen > fend - f - 4)
      return 0;
    if (h[f] == 0x42 && h[f + 1] == 0x43 && slen == 2) {
      const size_t total = le16(h + f + 4) + (size_t)1;
      if (total < fend + 8 || total > n - at)
        return 0;
      return total;
    }
    f += 4 + slen;
  }
  return 0;
}

// Walks the BSIZE chain of a BGZF file in host memory: offsets[i] is where block i starts, *count how many were
// found (at most cap), and the return value where the walk stopped -- n for a whole file, else the offset of the
// first block that is not whole (or of block `cap`).  Block i is [offsets[i], offsets[i + 1]), the last one ends
// where the walk stopped.  The chain is serial (each length stands in the block before), so this is host work,
// done once before the file is copied.
constexpr size_t bgzf_split(const uint8_t* host, size_t n, size_t* offsets, size_t cap, size_t* count)
{
  size_t at = 0, k = 0;
  while (at < n && k < cap) {
    const size_t len = bgzf_block_bytes(host, at, n);
    if (len == 0)
      break;
    offsets[k++] = at;
    at += len;
  }
  *count = k;
  return at;
}

} // namespace gzipframe
} // namespace hcamd
