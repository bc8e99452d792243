// The host logic of seekable Snappy framed streams (csrc/snappy_frame_index.hpp: the index writer, the parser with a
// reason per refusal, the tests an index has to pass) as a plain C++ program for
// tests/test_snappy_frame_index_cpu.py -- built once as it is and once with -fsanitize=address,undefined.
//   snappy_frame_index_driver_cpu check RECORDS
//       RECORDS: per input a u32 length and the bytes.  Every input is copied to a heap block of exactly its length
//       (so that a read behind it is a sanitizer's finding) and given to input_is_indexed and, from its first byte,
//       to index_applies.  prints per input "REASON UNITS CHUNKS CONTENT FIRST_REASON FIRST_END"
//   snappy_frame_index_driver_cpu write RECORDS
//       RECORDS: per index u32 N, u32 chunk_bytes, u64 content_bytes, N u32 words.
//       prints per index the bytes write_index writes, in hex
//   snappy_frame_index_driver_cpu arith
//       prints "content chunk_bytes chunks_of index_bytes first_share last_share chunk_bytes_of_word bound" lines for
//       a fixed list of sizes (see the test)
#include "snappy_frame_index.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace hcamd;
using namespace hcamd::szf;

static constexpr crc32c::Tables kTables = crc32c::make_tables();

static_assert(index_bytes(0) == 40 && index_bytes(7) == 68, "");
static_assert(kIndexMaxChunks == 4194294, "what a 24-bit length field holds");
static_assert(indexed_frame_bound(3, 1024) == 10 + 3 * 1032 + 52, "");
static_assert(indexed_chunk_bytes(written_header(10, 100)) == written_bytes(10, 100), "a word says where the next chunk stands");

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
    uint64_t units = 0, chunks = 0, content = 0;
    const uint32_t whole = input_is_indexed(kTables, in.get(), n, units, chunks, content);
    IndexedUnit u;
    const uint32_t first = index_applies(kTables, in.get(), n, 0, u);
    std::printf("%u %llu %llu %llu %u %llu\n", whole, (unsigned long long)units, (unsigned long long)chunks,
                (unsigned long long)content, first, (unsigned long long)(first == kIndexOk ? u.end : 0));
  }
  return 0;
}

static int write(const char* path)
{
  const std::vector<uint8_t> all = read_file(path);
  size_t at = 0;
  while (at < all.size()) {
    const uint32_t n = u32_at(all, at), chunk_bytes = u32_at(all, at + 4);
    const uint64_t content = (uint64_t)u32_at(all, at + 8) | ((uint64_t)u32_at(all, at + 12) << 32);
    at += 16;
    std::vector<uint32_t> words(n);
    for (uint32_t i = 0; i < n; ++i, at += 4)
      words[i] = u32_at(all, at);
    std::unique_ptr<uint8_t[]> out(new uint8_t[index_bytes(n)]);
    write_index(kTables, out.get(), words.data(), n, chunk_bytes, content);
    for (uint64_t k = 0; k < index_bytes(n); ++k)
      std::printf("%02x", out[k]);
    std::printf("\n");
  }
  return 0;
}

static int arith()
{
  const uint64_t contents[] = {0, 1, 255, 256, 257, 65535, 65536, 65537, (1ull << 32) + 5};
  const uint32_t chunk_sizes[] = {1, 256, 1000, 65536};
  for (uint64_t c : contents)
    for (uint32_t b : chunk_sizes) {
      IndexHead h;
      h.chunk_bytes = b;
      h.content_bytes = c;
      const uint64_t n = chunks_of(c, b);
      h.chunks = (uint32_t)n;
      // (chunk_share is asked only where N fits the field)
      const bool fits = n <= 0xFFFFFFFFull && n > 0;
      std::printf("%llu %u %llu %llu %u %u %llu %llu\n", (unsigned long long)c, b, (unsigned long long)n,
                  (unsigned long long)index_bytes(n), fits ? chunk_share(h, 0) : 0, fits ? chunk_share(h, n - 1) : 0,
                  (unsigned long long)indexed_chunk_bytes(written_header(b, b)), (unsigned long long)indexed_frame_bound(7, b));
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
  std::fprintf(stderr, "usage: see the head of snappy_frame_index_driver_cpu.cpp\n");
  return 2;
}
