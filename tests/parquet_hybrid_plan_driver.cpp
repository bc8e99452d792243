// parquet_hybrid_plan_driver.cpp -- prints what hipcomp-core_amd/csrc/parquet_hybrid_plan.hpp makes of a list of items,
// for tests/test_parquet_hybrid_plan_cpu.py: a program of its own, compiled with g++ alone (no HIP) under the address
// and undefined-behaviour sanitizers.  Every stream is decoded in a heap buffer of exactly its length into a heap
// buffer of exactly its capacity, so a read or a write outside either is the sanitizer's to report.
//
//   parquet_hybrid_plan_driver LIST OUT
// LIST: a line per item, "file offset length form bit_width wanted capacity element_bytes match".  Per item a line
// "item k ok 0|1 consumed c matches m size s untouched 0|1"; OUT gets the s elements of every item, back to back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "parquet_hybrid_plan.hpp"

using namespace hcamd::pqh;

// the header's functions are constexpr in earnest: a stream decoded by the compiler
struct Fixed
{
  uint8_t b[6] = {0x03, 0x8D, 0x06, 0x27, 0x00, 0x00}; // a group of width 3, then 3 x 0 (cut: refused where wanted)
  constexpr uint32_t at(uint64_t pos) const { return b[pos]; }
};
constexpr uint32_t third_of_fixed()
{
  Fixed f;
  return extract(f, 1, 2, 3);
}
static_assert(third_of_fixed() == ((0x27068Du >> 6) & 7u), "extract");
static_assert(where_of(7, 25).byte == 21 && where_of(7, 25).shift == 7 && where_of(7, 25).bytes == 4, "where_of");
static_assert(where_of(1, 31).bytes == 5 && where_of(3, 32).bytes == 4 && where_of(5, 0).bytes == 0, "where_of");

template <class T>
static void item(size_t k, const std::vector<uint8_t>& pool, uint64_t n, uint32_t form, uint32_t bit_width, uint64_t wanted,
                 uint64_t capacity, uint32_t match, std::ofstream& out)
{
  uint8_t* const in = new uint8_t[n]; // (exactly its length)
  if (n)
    std::memcpy(in, pool.data(), n);
  T* const values = new T[capacity];
  const T fill = (T)0xA5A5A5A5u;
  for (uint64_t i = 0; i < capacity; ++i)
    values[i] = fill;
  uint64_t matches = 0;
  const Verdict v = decode_item(in, n, form, bit_width, wanted, capacity, values, match, matches);
  bool untouched = true;
  for (uint64_t i = v.ok ? wanted : 0; i < capacity; ++i)
    untouched = untouched && values[i] == fill;
  const uint64_t size = v.ok ? wanted : 0;
  std::printf("item %zu ok %d consumed %llu matches %llu size %llu untouched %d\n", k, (int)v.ok, (unsigned long long)v.consumed,
              (unsigned long long)matches, (unsigned long long)size, (int)untouched);
  out.write(reinterpret_cast<const char*>(values), (std::streamsize)(size * sizeof(T)));
  delete[] values;
  delete[] in;
}

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s LIST OUT\n", argv[0]);
    return 2;
  }
  std::ifstream list(argv[1]);
  std::ofstream out(argv[2], std::ios::binary);
  std::string line, cached;
  std::vector<uint8_t> file;
  size_t k = 0;
  while (std::getline(list, line)) {
    std::istringstream ls(line);
    std::string path;
    uint64_t offset, length, wanted, capacity;
    uint32_t form, bit_width, element, match;
    if (!(ls >> path >> offset >> length >> form >> bit_width >> wanted >> capacity >> element >> match)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    if (path != cached) {
      std::ifstream f(path, std::ios::binary);
      file.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
      cached = path;
    }
    if (offset + length > file.size()) {
      std::fprintf(stderr, "item %zu lies outside %s\n", k, path.c_str());
      return 2;
    }
    const std::vector<uint8_t> bytes(file.begin() + (std::ptrdiff_t)offset, file.begin() + (std::ptrdiff_t)(offset + length));
    switch (element) {
    case 1: item<uint8_t>(k, bytes, length, form, bit_width, wanted, capacity, match, out); break;
    case 2: item<uint16_t>(k, bytes, length, form, bit_width, wanted, capacity, match, out); break;
    case 4: item<uint32_t>(k, bytes, length, form, bit_width, wanted, capacity, match, out); break;
    default: std::fprintf(stderr, "element of %u bytes\n", element); return 2;
    }
    ++k;
  }
  return 0;
}
