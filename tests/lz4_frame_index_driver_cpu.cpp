// The host logic of seekable LZ4 frames (csrc/lz4_frame_index.hpp: the index writer, the parser with a reason per
// refusal, the tests an index has to pass) as a plain C++ program for tests/test_lz4_frame_index_cpu.py -- built
// once as it is and once with -fsanitize=address,undefined.
//   lz4_frame_index_driver_cpu check RECORDS
//       RECORDS: per input a u32 length and the bytes.  Every input is copied to a heap block of exactly its length
//       (so that a read behind it is a sanitizer's finding) and given to input_is_indexed and, from its first byte,
//       to index_applies.  prints per input "REASON FRAMES BLOCKS CONTENT FIRST_REASON FIRST_END"
//   lz4_frame_index_driver_cpu write RECORDS
//       RECORDS: per index u32 N, u32 block_bytes, u64 content_bytes, u32 block checksums, N u32 size words.
//       prints per index the bytes write_index writes, in hex, and checks index_bytes against their number
//   lz4_frame_index_driver_cpu arith
//       prints "blocks_of block_content..." lines for a fixed list of sizes (see the test)
#include "lz4_frame_index.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace hcamd::lz4f;

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

static uint32_t u32_at(const std::vector<uint8_t>& v, size_t at)
{
  if (at + 4 > v.size())
    std::exit(2);
  uint32_t x;
  std::memcpy(&x, v.data() + at, 4);
  return x;
}

static int check(const char* path)
{
  const std::vector<uint8_t> all = read_file(path);
  size_t at = 0;
  while (at < all.size()) {
    const uint32_t n = u32_at(all, at);
    at += 4;
    if (at + n > all.size())
      return 2;
    std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
    std::memcpy(in.get(), all.data() + at, n);
    at += n;
    uint64_t frames = 0, blocks = 0, content = 0;
    const uint32_t whole = input_is_indexed(in.get(), n, frames, blocks, content);
    IndexedFrame f;
    const uint32_t first = index_applies(in.get(), n, 0, f);
    std::printf("%u %llu %llu %llu %u %llu\n", whole, (unsigned long long)frames, (unsigned long long)blocks,
                (unsigned long long)content, first, (unsigned long long)(first == kIndexOk ? f.end : 0));
  }
  return 0;
}

static int write(const char* path)
{
  const std::vector<uint8_t> all = read_file(path);
  size_t at = 0;
  while (at < all.size()) {
    const uint32_t n = u32_at(all, at), block_bytes = u32_at(all, at + 4);
    const uint64_t content = (uint64_t)u32_at(all, at + 8) | ((uint64_t)u32_at(all, at + 12) << 32);
    const uint32_t sums = u32_at(all, at + 16);
    at += 20;
    std::vector<uint32_t> words(n);
    for (uint32_t i = 0; i < n; ++i, at += 4)
      words[i] = u32_at(all, at);
    std::unique_ptr<uint8_t[]> out(new uint8_t[index_bytes(n)]);
    write_index(out.get(), words.data(), n, block_bytes, content, sums != 0);
    for (uint64_t k = 0; k < index_bytes(n); ++k)
      std::printf("%02x", out[k]);
    std::printf("\n");
  }
  return 0;
}

static int arith()
{
  const uint64_t contents[] = {0, 1, 255, 256, 257, 65535, 65536, 65537, (1ull << 32) + 5, ~0ull};
  const uint32_t block_sizes[] = {1, 256, 65536, 4u << 20};
  for (uint64_t c : contents)
    for (uint32_t b : block_sizes) {
      IndexHead h;
      h.block_bytes = b;
      h.content_bytes = c;
      const uint64_t n = blocks_of(c, b);
      h.blocks = (uint32_t)n;
      // (block_content is asked only where N fits the field)
      const bool fits = n <= 0xFFFFFFFFull && n > 0;
      std::printf("%llu %u %llu %llu %llu %llu %llu %llu\n", (unsigned long long)c, b, (unsigned long long)n,
                  (unsigned long long)index_bytes(n <= 0xFFFFFFFFull ? n : 0), (unsigned long long)(fits ? block_content(h, 0) : 0),
                  (unsigned long long)(fits ? block_content(h, n - 1) : 0), (unsigned long long)indexed_block_bytes(0x80000000u | b, true),
                  (unsigned long long)indexed_frame_bound(7, b, c & 1));
    }
  return 0;
}

int main(int argc, char** argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "check" && argc == 3)
    return check(argv[2]);
  if (cmd == "write" && argc == 3)
    return write(argv[2]);
  if (cmd == "arith" && argc == 2)
    return arith();
  std::fprintf(stderr, "usage: see the head of lz4_frame_index_driver_cpu.cpp\n");
  return 2;
}
