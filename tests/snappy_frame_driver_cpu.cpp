// The host logic of the Snappy framed-stream path (csrc/snappy_frame.hpp, csrc/crc32c_math.hpp) as a plain C++
// program, for tests/test_snappy_frame_cpu.py; built once as it is and once with -fsanitize=address,undefined.
//   snappy_frame_driver_cpu parse FILE    FILE: records of a u8 (1: the chunk opens the input), a u32 length and that
//                                         many bytes, each an input from a chunk's first byte to the input's end; per
//                                         record "reason kind bytes payload content crc" (the record's bytes are copied
//                                         to a heap block of exactly that size)
//   snappy_frame_driver_cpu walk FILE     FILE: records of a u32 length and that many bytes, each a whole input; the
//                                         chunk chain as the walk kernel follows it; per record "reason chunks content pos"
//   snappy_frame_driver_cpu crc FILE      the CRC-32C of every prefix of FILE, one per line, from length 0 on, slice-by-16
//                                         and bytewise (exit 5 where the two differ)
//   snappy_frame_driver_cpu join FILE     per split point 0, 1, 15, 16, 17, 1000, 2048, 4095, |FILE| of FILE:
//                                         "crc(A||B) shift(crc(A), |B|) ^ crc(B)"
//   snappy_frame_driver_cpu mask VALUE    "mask(VALUE) unmask(mask(VALUE))"
//   snappy_frame_driver_cpu arith CHUNK BLOCK N   "stored written_bytes written_header bound"
#include "crc32c_math.hpp"
#include "snappy_frame.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace hcamd;

static constexpr crc32c::Tables kTables = crc32c::make_tables();
static constexpr crc32c::ShiftTable kShift = crc32c::make_shift_table();

constexpr uint32_t crc_of_text(const char* s, size_t n)
{
  uint32_t reg = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i)
    reg = (reg >> 8) ^ kTables.t[0][(reg ^ (uint8_t)s[i]) & 0xFFu];
  return ~reg;
}
// (what the headers promise: usable in constant expressions; the format's own vectors)
static_assert(crc_of_text("123456789", 9) == 0xE3069283u, "CRC-32C check value");
static_assert(szf::mask_crc(0xE3069283u) == 0xC78AB0E5u, "the mask");
static_assert(szf::mask_crc(crc_of_text("", 0)) == 0xA282EAD8u, "the masked CRC of no bytes");
static_assert(szf::unmask_crc(0xC78AB0E5u) == 0xE3069283u, "");
static_assert(szf::frame_bound(0, 65536) == 10 && szf::frame_bound(3, 1024) == 10 + 3 * 1032, "");
static_assert(szf::identifier().byte(0) == 0xff && szf::identifier().byte(4) == 's' && szf::identifier().byte(9) == 'Y', "");

static std::vector<uint8_t> read_file(const char* path)
{
  FILE* f = std::fopen(path, "rb");
  if (!f)
    std::exit(2);
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> v((size_t)n);
  if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n)
    std::exit(2);
  std::fclose(f);
  return v;
}

// slice-by-16 over whole 16-byte blocks, the rest bytewise: the kernels' per-lane loop
static uint32_t crc_sliced(const uint8_t* p, size_t n)
{
  uint32_t reg = 0xFFFFFFFFu;
  size_t i = 0;
  for (; i + 16 <= n; i += 16) {
    uint32_t w[4];
    std::memcpy(w, p + i, 16);
    reg = crc32c::crc32c_update_16(kTables, reg, w[0], w[1], w[2], w[3]);
  }
  return ~crc32c::crc32c_update_bytes(kTables.t[0], reg, p + i, n - i);
}

int main(int argc, char** argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  if ((cmd == "parse" || cmd == "walk") && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    size_t at = 0;
    while (at + (cmd == "parse" ? 5 : 4) <= d.size()) {
      const bool first = cmd == "parse" ? d[at++] != 0 : true;
      uint32_t n;
      std::memcpy(&n, &d[at], 4);
      at += 4;
      uint8_t* p = (uint8_t*)std::malloc(n ? n : 1); // (a block of exactly n bytes: a read behind it is caught)
      std::memcpy(p, d.data() + at, n);
      at += n;
      if (cmd == "parse") {
        szf::Chunk c;
        const uint32_t r = n ? szf::parse_chunk(szf::window_of(p, n), n, first, c) : (uint32_t)szf::kTruncated;
        std::printf("%u %u %u %u %u %u\n", r, c.kind, c.bytes, c.payload, c.content, c.crc);
      } else {
        uint64_t pos = 0, chunks = 0, content = 0;
        uint32_t r = szf::kOk;
        while (pos < n) {
          szf::Chunk c;
          r = szf::parse_chunk(szf::window_of(p + pos, n - pos), n - pos, pos == 0, c);
          if (r != szf::kOk)
            break;
          if (c.kind != szf::kSkipped) {
            chunks += 1;
            content += c.content;
          }
          pos += c.bytes;
        }
        std::printf("%u %llu %llu %llu\n", r, (unsigned long long)chunks, (unsigned long long)content, (unsigned long long)pos);
      }
      std::free(p);
    }
    return 0;
  }
  if (cmd == "crc" && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    for (size_t n = 0; n <= d.size(); ++n) {
      uint8_t* p = (uint8_t*)std::malloc(n ? n : 1);
      std::memcpy(p, d.data(), n);
      const uint32_t a = crc_sliced(p, n), b = crc32c::crc32c_of(kTables, p, n);
      std::free(p);
      if (a != b)
        return 5;
      std::printf("%u\n", a);
    }
    return 0;
  }
  if (cmd == "join" && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    for (size_t cut : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)1000, (size_t)2048, (size_t)4095, d.size()}) {
      if (cut > d.size())
        continue;
      const uint32_t a = crc_sliced(d.data(), cut), b = crc_sliced(d.data() + cut, d.size() - cut);
      // (an empty piece has CRC 0 and adds nothing)
      const uint32_t joined = crc32c::crc32c_shift(kShift.x2n, a, (uint32_t)(d.size() - cut)) ^ b;
      std::printf("%u %u\n", crc_sliced(d.data(), d.size()), joined);
    }
    return 0;
  }
  if (cmd == "mask" && argc == 3) {
    const uint32_t v = (uint32_t)std::strtoull(argv[2], nullptr, 0);
    std::printf("%u %u\n", szf::mask_crc(v), szf::unmask_crc(szf::mask_crc(v)));
    return 0;
  }
  if (cmd == "arith" && argc == 5) {
    const uint64_t chunk = std::strtoull(argv[2], nullptr, 0), block = std::strtoull(argv[3], nullptr, 0),
                   n = std::strtoull(argv[4], nullptr, 0);
    std::printf("%d %llu %u %llu\n", (int)szf::stored(block, chunk), (unsigned long long)szf::written_bytes(block, chunk),
                szf::written_header(block, chunk), (unsigned long long)szf::frame_bound(n, chunk));
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of snappy_frame_driver_cpu.cpp\n");
  return 2;
}
