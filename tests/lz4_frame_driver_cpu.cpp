// The host logic of the LZ4 frame path (csrc/lz4_frame.hpp, csrc/xxh32_math.hpp) as a plain C++ program, for
// tests/test_lz4_frame_cpu.py and tests/test_lz4_framegen_cpu.py; built once as it is and once with
// -fsanitize=address,undefined.
//   lz4_frame_driver_cpu xxh32 FILE       the XXH32 (seed 0) of every prefix of FILE, one per line, from length 0 on
//   lz4_frame_driver_cpu parse FILE       FILE: records of a u32 length and that many bytes, each the front of an input;
//                                         per record "reason header_bytes block_max linked bsum csum has_size size"
//                                         (the record's bytes are copied to a heap block of exactly that size)
//   lz4_frame_driver_cpu write CODE SIZE SUMS      the 15 descriptor bytes in hex
//   lz4_frame_driver_cpu arith CHUNK STREAM N SUMS "code block_max stored size_word block_bytes bound"
#include "lz4_frame.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace hcamd;

// (what the header promises: usable in constant expressions)
static_assert(lz4f::code_for_chunk(65536) == 4 && lz4f::code_for_chunk(65537) == 5 && lz4f::code_for_chunk((4u << 20) + 1) == 0, "");
static_assert(lz4f::frame_bound(0, 65536, false) == 19, "header and EndMark");
static_assert(xxh32::avalanche(xxh32::short_init(0)) == 0x02CC5D05u, "XXH32 of no bytes");

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

int main(int argc, char** argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "xxh32" && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    for (size_t n = 0; n <= d.size(); ++n) {
      uint8_t* p = (uint8_t*)std::malloc(n ? n : 1); // (a block of exactly n bytes: a read behind it is caught)
      std::memcpy(p, d.data(), n);
      std::printf("%u\n", xxh32::hash(p, n, 0));
      std::free(p);
    }
    return 0;
  }
  if (cmd == "parse" && argc == 3) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    size_t at = 0;
    while (at + 4 <= d.size()) {
      uint32_t n;
      std::memcpy(&n, &d[at], 4);
      at += 4;
      uint8_t* p = (uint8_t*)std::malloc(n ? n : 1);
      std::memcpy(p, d.data() + at, n);
      at += n;
      lz4f::Descriptor h;
      const uint32_t r = lz4f::parse_descriptor(p, n, h);
      std::printf("%u %u %u %d %d %d %d %llu\n", r, h.header_bytes, h.block_max, (int)h.linked, (int)h.block_checksums,
                  (int)h.content_checksum, (int)h.has_content_size, (unsigned long long)h.content_size);
      std::free(p);
    }
    return 0;
  }
  if (cmd == "write" && argc == 5) {
    uint8_t h[lz4f::kWrittenHeaderBytes];
    lz4f::write_descriptor(h, (uint32_t)std::atoi(argv[2]), std::strtoull(argv[3], nullptr, 0), std::atoi(argv[4]) != 0);
    for (uint8_t b : h)
      std::printf("%02x", b);
    std::printf("\n");
    return 0;
  }
  if (cmd == "arith" && argc == 6) {
    const uint64_t chunk = std::strtoull(argv[2], nullptr, 0), stream = std::strtoull(argv[3], nullptr, 0),
                   n = std::strtoull(argv[4], nullptr, 0);
    const bool sums = std::atoi(argv[5]) != 0;
    const uint32_t code = lz4f::code_for_chunk(chunk);
    std::printf("%u %u %d %u %llu %llu\n", code, lz4f::block_max_of_code(code), (int)lz4f::stored(stream, chunk),
                lz4f::size_word(stream, chunk), (unsigned long long)lz4f::block_bytes(stream, chunk, sums),
                (unsigned long long)lz4f::frame_bound(n, chunk, sums));
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of lz4_frame_driver_cpu.cpp\n");
  return 2;
}
